// Exact DTW alignment (csrc/dtw.hip): the layout constants the kernels and the host side share.  DESIGN.md 4e is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"

#define DTW_LANES 64                // one wave per problem: lane t hands its last row to lane t + 1 by a lane move, so a step has no barrier at all
#define DTW_R 8                     // consecutive rows of a row block one lane owns (their features stay in registers)
#define DTW_B (DTW_LANES * DTW_R)   // rows of a row block
#define DTW_BPW 16                  // cells per backpointer word: 2 bits each, 16 consecutive columns of ONE row -- 16 consecutive steps of the owning lane
#define DTW_MAX_FRAMES (1 << 16)    // frames per side
#define DTW_MAX_PAIRS 4096          // pairs per call (12 x that many workgroups in the transposition launch)
#define DTW_HDR 8                   // int32 header of a pair's result: L, opt shift, pitch_shift, points of the unfiltered path, D[-1,-1] (a double in ints 4..5), 0, 0
#define DTW_MAX_DEBUG_CELLS (1LL << 22)

// one pair of a call (device table at the head of the workspace, built per call); the off_* are BYTE offsets into the workspace
struct DtwPair {
  const float *c1, *o1, *c2, *o2;   // cover chroma / DLNCO [12][N1], origin chroma / DLNCO [12][N2]
  int N1, N2, M1, M2;               // frames, CENS frames
  int cap;                          // path columns reserved in the result: min(N1, N2) + 1
  int opt;                          // the chroma shift of the final DTW: written by k_dtw_argmin (or the host, for the debug hooks)
  long long off_f1, off_f2;         // [N][24] fp32: normalised chroma, DLNCO of frame n side by side
  long long off_cens1, off_cens2;   // [M][12] fp32
  long long off_top;                // [N2] fp64: the last D row of the previous row block
  long long off_top12, top12_stride;// 12 x [M2] fp64 of the shift problems, stride in bytes
  long long off_totals;             // [12] fp64
  long long off_bp, bp_stride;      // [N1][bp_stride] uint32, bp_stride = ceil(N2 / 16)
  long long off_tmp;                // [cap][2] int32: the kept points, last to first
  long long off_raw;                // [N1 + N2][2] int32: every point of the unfiltered path, last to first (the debug hook reads it)
  long long res_off;                // int32 offset of this pair's block in the result buffer
};
