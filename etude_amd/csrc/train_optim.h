// What the two trainers' optimizers share (dec_train.hip: AdamW, separator_train.hip: Adam): the gradient norm, the scalars of a step and the host's access to the
// flat [P | G | M1 | M2] buffers.  The two update kernels stay in their files: they differ on purpose (k_tadamw: decay, multiply-then-add; k_st_adam: torch.optim.Adam's
// trailing fma forms), each pinned bit for bit by its CPU restatement.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"

#define TN_BLOCKS 256
// fp64 partial sums of squares: block b owns elements [b * chunk, (b + 1) * chunk), thread t every 256th of them; the 256 thread sums are added in thread order
static __global__ __launch_bounds__(256) void k_tsumsq(const float* __restrict__ g, long long n, long long chunk, double* __restrict__ partial) {
  __shared__ double ps[256];
  const long long b0 = (long long)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  double a = 0.0;
  for (long long i = b0 + threadIdx.x; i < b1; i += 256) { const double v = (double)g[i]; a += v * v; }
  ps[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += ps[i];
    partial[blockIdx.x] = tot;
  }
}

// the l2 norm of g [n]: the blocks' partials (partial_dev [TN_BLOCKS]) are added on the host in block order, one square root
static inline int grad_norm(const float* g, long long n, double* partial_dev, hipStream_t st, double* out) {
  const long long chunk = (n + TN_BLOCKS - 1) / TN_BLOCKS;
  hipLaunchKernelGGL(k_tsumsq, dim3(TN_BLOCKS), dim3(256), 0, st, g, n, chunk, partial_dev);
  HIP_TRY(hipGetLastError());
  double part[TN_BLOCKS];
  HIP_TRY(hipMemcpyAsync(part, partial_dev, sizeof(part), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double tot = 0.0;
  for (int i = 0; i < TN_BLOCKS; ++i) tot += part[i];
  *out = sqrt(tot);
  return ETD_OK;
}

// a v_mul_f32 of its own: left to itself the SLP vectoriser pairs an update kernel's independent multiplies into v_pk_mul_f32 with a crossed op_sel, the packed form
// tests/test_isa_guard.py keeps out of the library (merge_sum in dec_kernels.hip)
__device__ __forceinline__ float mul_scalar(float a, float b) {
  float r;
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// The scalars of step `step` (1-based), formed in double and rounded once: clip_grad_norm_'s coefficient (1 when max_norm <= 0: no clipping) and the two bias
// corrections as the update kernels take them
struct StepScalars { float coef, step_size, bc2_sqrt; };
static inline StepScalars step_scalars(double max_norm, double norm, double lr, double beta1, double beta2, long long step) {
  const double coef = max_norm > 0.0 ? std::min(1.0, max_norm / (norm + 1e-6)) : 1.0;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  return {(float)coef, (float)(lr / bc1), (float)sqrt(bc2)};
}

// n floats at `off` of one of the flat buffers, to the host (`out`) or from it (`in`).  which: 0 parameter (state), 1 gradient, 2 exp_avg, 3 exp_avg_sq
static inline int flat_io(float* P, float* G, float* M1, float* M2, int which, long long off, long long n, float* out, const float* in, hipStream_t st) {
  float* base = which == 0 ? P : which == 1 ? G : which == 2 ? M1 : M2;
  if (out) HIP_TRY(hipMemcpyAsync(out, base + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
  else HIP_TRY(hipMemcpyAsync(base + off, in, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
