// Training engine of the EtudeDecoder (etd_dtrain_*): forward with saved activations, backward of the reference's cross-entropy loss for every parameter,
// global-norm clipping and AdamW, all in fp32.  These are the launchers the engine is made of; the two that can go wrong at a tile edge are
// also reachable on their own through include/etude_hip_debug.h.
// Nothing here uses a floating-point atomic: every sum runs in an order fixed by the shapes alone, so a call's bits do not depend on which workgroup ran first.
#pragma once
#include "common.h"

// C[M][N] (row stride ldc) = (accumulate ? C : 0) + sum_k A(i, k) B(k, j) (+ bias[j]), fp32 operands on v_mfma_f32_32x32x2_f32.  One workgroup owns a 64 x 64 tile of C for the
// whole of K; an element's sum is 8 interleaved chains in ascending k, added pairwise: fixed by the shape alone.  The three forms of a linear layer and its backward pass:
enum {
  ETD_TG_NT = 0,   // Y  = X W^T   A = X  [M][K] (lda),  B = W [N][K] (ldb)              forward (bias allowed)
  ETD_TG_NN = 1,   // dX = dY W    A = dY [M][K] (lda),  B = W [K][N] (ldb)              input gradient
  ETD_TG_TN = 2,   // dW += dY^T X A = dY [K][M] (lda),  B = X [K][N] (ldb)              weight gradient: the reduction runs over the batch rows in ascending order
};
int launch_tgemm(int form, int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, bool accumulate,
                 hipStream_t st);

// ---- row, elementwise and optimizer launchers shared with the Beat-Transformer trainer (beat_train.hip); the kernels are dec_train.hip's
// LayerNorm statistics of each row + up to two normalised outputs; mean / rstd (both or neither) and the second output may be NULL
void launch_tln_fwd(const float* x, int M, int H, float eps, float* mean, float* rstd, const float* g1, const float* b1, float* y1, const float* g2,
                    const float* b2, float* y2, hipStream_t st);
// dx += the LayerNorm input gradient of dy
void launch_tln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, int M, int H, float* dx, hipStream_t st);
void launch_tgelu(const float* x, float* y, long long n, hipStream_t st);
void launch_tgelu_bwd(const float* x, float* dy, long long n, hipStream_t st);      // dy *= gelu'(x)
// column sums over the batch rows, added to g0 (mode 0: a bias) or to g0 / g1 (mode 1: LayerNorm bias / gain; mode 0 reads no x, mean, rstd, g1)
void launch_tcolred(int mode, const float* dy, int ld, int M, int N, const float* x, const float* mean, const float* rstd, float* g0, float* g1, hipStream_t st);
// clip_grad_norm_'s coefficient and torch.optim.AdamW's step `step` (1-based) as k_tadamw takes them
struct AdamwArgs { float coef, decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps; };
int adamw_check(const char* who, double lr, double beta1, double beta2, double eps, double weight_decay);
AdamwArgs adamw_args(double max_norm, double norm, double lr, double beta1, double beta2, double eps, double weight_decay, long long step);
void launch_tadamw(float* p, float* g, float* m, float* v, long long n, const AdamwArgs& a, hipStream_t st);

// Causal attention over packed ragged sequences, head_dim 64, the HF layout of the fused projection: row r of qkv is [head][q | k | v][64] (row stride 3 * nh * 64).
// Sequence s is rows [row0[s], row0[s] + len[s]).  Forward: O [M][nh * 64] and one log-sum-exp per (row, head); no T x T matrix leaves the chip.
int launch_tattn_fwd(const float* qkv, int nh, const int* row0, const int* len, int n_seq, int max_len, float* O, float* lse, hipStream_t st);
// Backward: dqkv (same layout as qkv) from dO, with P recomputed from q, k and the saved lse and D = rowsum(dO * O) (written to Dbuf [M][nh]).
// One kernel walks query tiles (dQ, D), a second walks key tiles (dK, dV), each adding its terms in ascending order of the other index.
int launch_tattn_bwd(const float* qkv, const float* O, const float* lse, const float* dO, int nh, const int* row0, const int* len, int n_seq, int max_len,
                     float* Dbuf, float* dqkv, hipStream_t st);
