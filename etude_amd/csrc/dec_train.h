// Training engine of the EtudeDecoder (etd_dtrain_*): forward with saved activations, backward of the reference's cross-entropy loss for every parameter,
// global-norm clipping and AdamW, all in fp32.  These are the launchers of the decoder's own attention; the kernels every trainer shares are
// train_kernels.h's.  Both families are also reachable on their own through include/etude_hip_debug.h.
// Nothing here uses a floating-point atomic: every sum runs in an order fixed by the shapes alone, so a call's bits do not depend on which workgroup ran first.
#pragma once
#include "common.h"

// Causal attention over packed ragged sequences, head_dim 64, the HF layout of the fused projection: row r of qkv is [head][q | k | v][64] (row stride 3 * nh * 64).
// Sequence s is rows [row0[s], row0[s] + len[s]).  Forward: O [M][nh * 64] and one log-sum-exp per (row, head); no T x T matrix leaves the chip.
int launch_tattn_fwd(const float* qkv, int nh, const int* row0, const int* len, int n_seq, int max_len, float* O, float* lse, hipStream_t st);
// Backward: dqkv (same layout as qkv) from dO, with P recomputed from q, k and the saved lse and D = rowsum(dO * O) (written to Dbuf [M][nh]).
// One kernel walks query tiles (dQ, D), a second walks key tiles (dK, dV), each adding its terms in ascending order of the other index.
int launch_tattn_bwd(const float* qkv, const float* O, const float* lse, const float* dO, int nh, const int* row0, const int* len, int n_seq, int max_len,
                     float* Dbuf, float* dqkv, hipStream_t st);
