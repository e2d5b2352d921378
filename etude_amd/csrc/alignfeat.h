// Alignment features (csrc/alignfeat.hip): the layout constants the kernels and the host side share.  DESIGN.md 4f is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"
#include "../../include/etude_hip_debug.h"

#define AF_L 256                    // samples of a chunk of the filter's time axis, on every tier
#define AF_MAX_SEC 6                // second-order sections per band
#define AF_NS (2 * AF_MAX_SEC)      // state of a band's cascade: z0, z1 per section
#define AF_BANDS 88                 // pitches 21 .. 108; band b = p - 21: 0 .. 38 on tier 2, 39 .. 74 on tier 1, 75 .. 87 on tier 0
#define AF_B2 39
#define AF_B1 36
#define AF_B0 13
#define AF_TAPS 481
#define AF_HALF 240
#define AF_DEC 5
#define AF_HOP 441
#define AF_THREADS 256
#define AF_IIR_THREADS 64           // one wave per workgroup of the filter launches: 64 consecutive chunks of ONE band, so the coefficients are wave-uniform
#define AF_MAX_SONGS 4096
#define AF_MAX_BANKS 64
#define AF_MAX_N (1LL << 27)        // samples per song (101 minutes)

// one song of a call (device table at the head of the workspace, built per call); the off_* are BYTE offsets into the workspace.  Index t of n / nc / nm is the tier:
// 0 = 22 050 Hz, 1 = 4 410 Hz, 2 = 882 Hz.  Per-band arrays hold the bands in ascending order, each with its tier's count (af_boff).
struct AfSong {
  const float* wav;                 // [n[0]]
  long long n[3];                   // samples
  long long nc[3];                  // chunks = ceil(n / AF_L)
  long long nm[3];                  // novelty frames = ceil(n / hop_tier)
  long long T;                      // feature frames = ceil(n[0] / 441)
  long long blk0;                   // first workgroup of a filter launch
  long long bpb[3];                 // workgroups per band = ceil(nc / AF_IIR_THREADS)
  long long off_x1, off_x2;         // tier signals, fp32
  long long off_u;                  // forward-filtered bands, fp64
  long long off_y;                  // zero-phase bands, fp32
  long long off_st;                 // [chunks of all bands][12] fp64: a chunk's end state from zero, then its true start state
  long long off_E;                  // [88][T] fp32
  long long off_nov, off_ph, off_pf;// per band [nm]: novelty fp32, peak height fp32 (0 = no peak), frame int32
  long long off_co;                 // [12][T] fp32: CO, then L = log(1 + 10000 CO)
  long long off_g, off_G;           // [T] fp32
  long long off_D;                  // [12][T] fp32
  long long out_off;                // floats before this song's [12][T] block in chroma_out and dlnco_out
  int bank, pad;
};
