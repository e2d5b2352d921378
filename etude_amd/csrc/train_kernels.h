// The kernels every trainer is made of (train_kernels.hip): the fp32 GEMM family, LayerNorm and GELU with their backward passes, the column reductions, the
// gradient norm and the AdamW update, with the scalars of an optimizer step.  Each trainer adds its model's own kernels (dec_train.h, beat_train.h,
// separator_train.hip); the parameter store they share is train_store.h ("trainer skeleton").
// Nothing here uses a floating-point atomic: every sum runs in an order fixed by the shapes alone, so a call's bits do not depend on which workgroup ran first.
#pragma once
#include <algorithm>
#include <cmath>

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

// LayerNorm statistics of each row + up to two normalised outputs; mean / rstd (both or neither) and the second output may be NULL
void launch_tln_fwd(const float* x, int M, int H, float eps, float* mean, float* rstd, const float* g1, const float* b1, float* y1, const float* g2,
                    const float* b2, float* y2, hipStream_t st);
// dx += the LayerNorm input gradient of dy
void launch_tln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, int M, int H, float* dx, hipStream_t st);
void launch_tgelu(const float* x, float* y, long long n, hipStream_t st);
void launch_tgelu_bwd(const float* x, float* dy, long long n, hipStream_t st);      // dy *= gelu'(x)
// column sums over the batch rows, added to g0 (mode 0: a bias) or to g0 / g1 (mode 1: LayerNorm bias / gain; mode 0 reads no x, mean, rstd, g1)
void launch_tcolred(int mode, const float* dy, int ld, int M, int N, const float* x, const float* mean, const float* rstd, float* g0, float* g1, hipStream_t st);

// the grid of an elementwise kernel of 256 threads over n elements
static inline dim3 ew_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

// ---- optimizer
#define TN_BLOCKS 256
// the l2 norm of g [n] (k_tsumsq): the blocks' fp64 partials (partial_dev [TN_BLOCKS]) are added on the host in block order, one square root
int grad_norm(const float* g, long long n, double* partial_dev, hipStream_t st, double* out);

// a v_mul_f32 of its own: left to itself the SLP vectoriser pairs an update kernel's independent multiplies into v_pk_mul_f32 with a crossed op_sel, the packed form
// tests/test_isa_guard.py keeps out of the library (merge_sum in dec_kernels.hip)
__device__ __forceinline__ float mul_scalar(float a, float b) {
  float r;
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// The scalars of step `step` (1-based), formed in double and rounded once: clip_grad_norm_'s coefficient (1 when max_norm <= 0: no clipping) and the two bias
// corrections as the update kernels take them.  The two update kernels stay in their files: they differ on purpose (k_tadamw: decay, multiply-then-add; k_st_adam:
// torch.optim.Adam's trailing fma forms), each pinned bit for bit by its CPU restatement.
struct StepScalars { float coef, step_size, bc2_sqrt; };
static inline StepScalars step_scalars(double max_norm, double norm, double lr, double beta1, double beta2, long long step) {
  const double coef = max_norm > 0.0 ? std::min(1.0, max_norm / (norm + 1e-6)) : 1.0;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  return {(float)coef, (float)(lr / bc1), (float)sqrt(bc2)};
}

// clip_grad_norm_'s coefficient and torch.optim.AdamW's step `step` (1-based) as k_tadamw takes them
struct AdamwArgs { float coef, decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps; };
int adamw_check(const char* who, double lr, double beta1, double beta2, double eps, double weight_decay);
AdamwArgs adamw_args(double max_norm, double norm, double lr, double beta1, double beta2, double eps, double weight_decay, long long step);
void launch_tadamw(float* p, float* g, float* m, float* v, long long n, const AdamwArgs& a, hipStream_t st);
