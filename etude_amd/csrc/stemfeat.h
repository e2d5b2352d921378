// Stem mel-dB features (csrc/stemfeat.hip): the layout constants the kernels and the host side share.
#pragma once
#include "host_util.h"
#include "lds_rfft.h"
#include "../../include/etude_hip.h"

#define SF_THREADS 256
#define SF_FRAMES 4                 // frames one workgroup of pass 1 computes (one twiddle-table load into LDS serves them all)
// dynamic LDS of pass 1 in floats, M complex points: the two buffer pairs of the FFT, then the float2 twiddle table padded the same way
#define SF_LDS_FLOATS(M) (6 * RFFT_PM(M))

// one song of a call (device table, built per call)
struct SfSong {
  const float* wav;                 // [instr][channels][N]
  long long N, T;
  long long feat_off;               // floats before this song's [instr][T][n_mels] block
  long long blk0;                   // first workgroup of pass 1 (= first entry of the per-workgroup maxima)
  long long cps;                    // workgroups per stem = ceil(T / SF_FRAMES)
};
