// Tuning estimation (csrc/tuning.hip): the layout constants the kernels and the host side share.  DESIGN.md 4g is the contract.
#pragma once
#include "host_util.h"
#include "lds_rfft.h"
#include "../../include/etude_hip.h"
#include "../../include/etude_hip_debug.h"

#define TN_FS 22050
#define TN_NFFT 16384
#define TN_HOP 8192
#define TN_M 8192                   // complex points of the packed real frame
#define TN_LGM 13
#define TN_BINS 8193                // k = 0 .. n_fft / 2
#define TN_GROUP 8                  // consecutive frames one workgroup of the frame kernel sums
#define TN_THREADS 1024             // the frame kernel: 2 radix-4 butterflies per thread and stage
#define TN_BPT 9                    // bins a thread of the frame kernel owns: k = tid + 1024 j, j < 9 (j = 8 is bin 8192, thread 0 alone)
#define TN_TAIL_THREADS 256
#define TN_LOGF 8400                // 1-cent steps from MIDI 24 up to, not including, MIDI 108
#define TN_THETA 100                // theta = -50 .. 49
#define TN_AVG 50                   // half width of the local average
#define TN_COMB 84                  // teeth of the comb: semitones 24 .. 107
#define TN_MIN_N 32768              // two windows
#define TN_MAX_N (1LL << 27)        // samples per song, the limit of etd_alignfeat_*
#define TN_MAX_SONGS 4096
#define TN_MAX_TAPS 8               // frames whose power one call of the debug hook can tap
// dynamic LDS of the frame kernel: the two buffer pairs of the FFT (4 x 8 449 floats; the twiddles stay in global memory)
#define TN_LDS_BYTES (4 * RFFT_PM(TN_M) * (int)sizeof(float))

// one song of a call (device table at the head of the workspace, built per call); the off_* are BYTE offsets into the workspace
struct TnSong {
  const float* wav;                 // [N]
  long long N;
  long long F;                      // frames = 1 + N / 8192
  long long G;                      // groups = ceil(F / 8)
  long long blk0;                   // first workgroup of the frame launch
  long long off_part;               // [G][8193] fp32: the groups' partial sums of C
  long long off_Y;                  // [8193] fp32
  long long off_Yi;                 // [8400] fp64
  long long off_R;                  // [8400] fp64
  long long off_sim;                // [100] fp64
};
