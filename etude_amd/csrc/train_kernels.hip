// The kernels the trainers share (train_kernels.h).  fp32 operands and fp32 accumulation everywhere; the products run on v_mfma_f32_32x32x2_f32 (the
// f16-split planes of gemm3.h need a proven bound of their operands, which gradients do not have).  No floating-point atomics: every sum -- a GEMM's K chain, a
// column reduction over the batch rows, the norm -- runs in an order fixed by the shapes of the call, so the same call on the same inputs gives the same bits.
#include "train_kernels.h"

#include <math.h>

#include "etude_hip.h"

// ================================================================================================ the GEMM family
#define TG_BK 32
#define TG_CH 8      // accumulator chains per output element
#define TG_LD 65     // 64 + 1: a wave that stores 32 consecutive k of two rows hits 64 distinct (bank, half) pairs

// AKC / BKC: k is the contiguous index of the operand in memory (decides which way the 256 threads sweep the tile, so that global loads coalesce)
template <bool KC>
__device__ __forceinline__ void tg_coords(int t, int r, int& i, int& k) {
  if (KC) { k = t & 31; i = (t >> 5) + 8 * r; }
  else { i = t & 63; k = (t >> 6) + 4 * r; }
}

template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void k_tgemm(int M, int N, int K, const float* __restrict__ A, long long sai, long long sak, const float* __restrict__ B,
                                               long long sbk, long long sbj, const float* __restrict__ bias, float* __restrict__ C, int ldc, int accumulate) {
  __shared__ float As[TG_BK][TG_LD], Bs[TG_BK][TG_LD];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int wr = w >> 1, wc = w & 1, half = l >> 5, l31 = l & 31;
  float ra[8], rb[8];
  // TG_CH accumulator chains: MFMA j of every K tile adds into chain j % TG_CH, and the chains are added pairwise at the end.  Each output element's sum is then
  // TG_CH interleaved chains of K / TG_CH terms instead of one of K terms -- the rounding error of a long batch-row reduction (dW over thousands of rows) grows
  // with the chain's length -- in an order that the shape alone fixes.
  f32x16 acc[TG_CH];
#pragma unroll
  for (int c = 0; c < TG_CH; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#define TG_LOAD(k0)                                                                                         \
  _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                           \
    int i, k;                                                                                               \
    tg_coords<AKC>(t, r, i, k);                                                                             \
    const long long gi = i0 + i, gk = (k0) + k;                                                             \
    ra[r] = (gi < M && gk < K) ? A[gi * sai + gk * sak] : 0.f;                                              \
    tg_coords<BKC>(t, r, i, k);                                                                             \
    const long long gj = j0 + i, gk2 = (k0) + k;                                                            \
    rb[r] = (gj < N && gk2 < K) ? B[gk2 * sbk + gj * sbj] : 0.f;                                            \
  }
  TG_LOAD(0)
  for (int k0 = 0; k0 < K; k0 += TG_BK) {
    __syncthreads();                                   // the previous tile has been read
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      int i, k;
      tg_coords<AKC>(t, r, i, k);
      As[k][i] = ra[r];
      tg_coords<BKC>(t, r, i, k);
      Bs[k][i] = rb[r];
    }
    __syncthreads();
    if (k0 + TG_BK < K) { TG_LOAD(k0 + TG_BK) }        // the next tile's loads fly while this one is multiplied
#pragma unroll
    for (int kk = 0; kk < TG_BK; kk += 2)
      acc[(kk >> 1) % TG_CH] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + half][wr * 32 + l31], Bs[kk + half][wc * 32 + l31], acc[(kk >> 1) % TG_CH], 0, 0, 0);
  }
#undef TG_LOAD
#pragma unroll
  for (int w2 = 1; w2 < TG_CH; w2 *= 2)
#pragma unroll
    for (int c = 0; c + w2 < TG_CH; c += 2 * w2)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] += acc[c + w2][r];
  const int col = j0 + wc * 32 + l31;
  if (col < N) {
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = i0 + wr * 32 + acc_row(r, half);
      if (row < M) {
        float* p = C + (long long)row * ldc + col;
        float v = acc[0][r] + bv;
        if (accumulate) v = *p + v;
        *p = v;
      }
    }
  }
}

int launch_tgemm(int form, int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, bool accumulate,
                 hipStream_t st) {
  if (M < 1 || N < 1 || K < 1 || !A || !B || !C) ETD_FAIL(ETD_EINVAL, "tgemm: bad shape M=%d N=%d K=%d", M, N, K);
  const int a_row = form == ETD_TG_TN ? M : K, b_row = form == ETD_TG_NT ? K : N;
  if (lda < a_row || ldb < b_row || ldc < N) ETD_FAIL(ETD_EINVAL, "tgemm: a row stride is shorter than its row (lda=%d ldb=%d ldc=%d)", lda, ldb, ldc);
  const dim3 grid((N + 63) / 64, (M + 63) / 64), block(256);
  if (grid.y > 65535u) ETD_FAIL(ETD_EINVAL, "tgemm: M=%d is above 65535 row tiles", M);
  const int acc = accumulate ? 1 : 0;
  switch (form) {
    case ETD_TG_NT: hipLaunchKernelGGL((k_tgemm<true, true>), grid, block, 0, st, M, N, K, A, (long long)lda, 1LL, B, 1LL, (long long)ldb, bias, C, ldc, acc); break;
    case ETD_TG_NN: hipLaunchKernelGGL((k_tgemm<true, false>), grid, block, 0, st, M, N, K, A, (long long)lda, 1LL, B, (long long)ldb, 1LL, bias, C, ldc, acc); break;
    case ETD_TG_TN: hipLaunchKernelGGL((k_tgemm<false, false>), grid, block, 0, st, M, N, K, A, 1LL, (long long)lda, B, (long long)ldb, 1LL, bias, C, ldc, acc); break;
    default: ETD_FAIL(ETD_EINVAL, "tgemm: unknown form %d", form);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ================================================================================================ row and elementwise kernels
// LayerNorm statistics of each row + up to two normalised outputs (the two LayerNorms of a GPT-NeoX layer read the same input).  One wave per row.
__global__ __launch_bounds__(64) void k_tln_fwd(const float* __restrict__ x, int M, int H, float eps, float* __restrict__ mean, float* __restrict__ rstd,
                                                const float* __restrict__ g1, const float* __restrict__ b1, float* __restrict__ y1,
                                                const float* __restrict__ g2, const float* __restrict__ b2, float* __restrict__ y2) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* xr = x + (long long)r * H;
  float s = 0.f;
  for (int c = lane; c < H; c += 64) s += xr[c];
  const float mu = wave_sum(s) / (float)H;
  float q = 0.f;
  for (int c = lane; c < H; c += 64) { const float d = xr[c] - mu; q = fmaf(d, d, q); }
  const float rs = 1.f / sqrtf(wave_sum(q) / (float)H + eps);
  if (lane == 0 && mean) { mean[r] = mu; rstd[r] = rs; }
  for (int c = lane; c < H; c += 64) {
    const float xh = (xr[c] - mu) * rs;
    if (y1) y1[(long long)r * H + c] = xh * g1[c] + b1[c];
    if (y2) y2[(long long)r * H + c] = xh * g2[c] + b2[c];
  }
}
// dx += rstd * (dy g - mean(dy g) - xhat mean(dy g xhat)); one wave per row
__global__ __launch_bounds__(64) void k_tln_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ g, int H, float* __restrict__ dx) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float* xr = x + (long long)r * H;
  const float* dr = dy + (long long)r * H;
  const float mu = mean[r], rs = rstd[r];
  float a = 0.f, b = 0.f;
  for (int c = lane; c < H; c += 64) {
    const float dg = dr[c] * g[c];
    a += dg;
    b = fmaf(dg, (xr[c] - mu) * rs, b);
  }
  a = wave_sum(a) / (float)H;
  b = wave_sum(b) / (float)H;
  for (int c = lane; c < H; c += 64) {
    const float xh = (xr[c] - mu) * rs;
    dx[(long long)r * H + c] += rs * (dr[c] * g[c] - a - xh * b);
  }
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__global__ void k_tgelu(const float* __restrict__ x, float* __restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = gelu_f(x[i]);
}
// dy *= gelu'(x) = Phi(x) + x phi(x)
__global__ void k_tgelu_bwd(const float* __restrict__ x, float* __restrict__ dy, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
  dy[i] *= cdf + v * pdf;
}

// Column reductions over the batch rows: 32 columns x 8 row slices per workgroup; slice s adds rows s, s + 8, .. in ascending order and the 8 partial sums are
// added in slice order.  MODE 0: g0[c] += sum_r dy[r][c] (a bias gradient).  MODE 1: also g1[c] += sum_r dy[r][c] xhat[r][c] (LayerNorm: g0 = bias, g1 = gain).
template <int MODE>
__global__ __launch_bounds__(256) void k_tcolred(const float* __restrict__ dy, int ld, int M, int N, const float* __restrict__ x, const float* __restrict__ mean,
                                                 const float* __restrict__ rstd, float* __restrict__ g0, float* __restrict__ g1) {
  __shared__ float p0[8][32], p1[8][32];
  const int t = threadIdx.x, c = blockIdx.x * 32 + (t & 31), s = t >> 5;
  float a0 = 0.f, a1 = 0.f;
  if (c < N)
    for (int r = s; r < M; r += 8) {
      const float v = dy[(long long)r * ld + c];
      a0 += v;
      if (MODE == 1) a1 = fmaf(v, (x[(long long)r * N + c] - mean[r]) * rstd[r], a1);
    }
  p0[s][t & 31] = a0; p1[s][t & 31] = a1;
  __syncthreads();
  if (s == 0 && c < N) {
    float t0 = p0[0][t], t1 = p1[0][t];
    for (int k = 1; k < 8; ++k) { t0 += p0[k][t]; t1 += p1[k][t]; }
    g0[c] += t0;
    if (MODE == 1) g1[c] += t1;
  }
}

// ================================================================================================ optimizer
// fp64 partial sums of squares: block b owns elements [b * chunk, (b + 1) * chunk), thread t every 256th of them; the 256 thread sums are added in thread order
__global__ __launch_bounds__(256) void k_tsumsq(const float* __restrict__ g, long long n, long long chunk, double* __restrict__ partial) {
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

int grad_norm(const float* g, long long n, double* partial_dev, hipStream_t st, double* out) {
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

#pragma clang fp contract(off)
// clip_grad_norm_'s g *= coef, then torch.optim.AdamW's single-tensor step, one element per thread.  1 - beta1 and 1 - beta2 arrive as the host's double differences
// rounded once, as torch passes them: formed here from the rounded betas, 1.f - 0.98f is 9.5e-7 (relative) short of 0.02 and every update 7e-7 too long -- a bias
// that showed as a loss below the fp64 trajectory's at every step.
__global__ void k_tadamw(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n, float coef, float decay,
                         float one_minus_beta1, float beta2, float one_minus_beta2, float step_size, float bc2_sqrt, float eps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = mul_scalar(g[i], coef);
  float pi = mul_scalar(p[i], decay);                                  // p.mul_(1 - lr * weight_decay)
  const float mi = m[i] + mul_scalar(gi - m[i], one_minus_beta1);       // exp_avg.lerp_(grad, 1 - beta1)
  const float vi = mul_scalar(v[i], beta2) + mul_scalar(one_minus_beta2, gi) * gi;   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi = pi - step_size * (mi / denom);                        // p.addcdiv_(exp_avg, denom, value = -step_size)
  p[i] = pi; g[i] = gi; m[i] = mi; v[i] = vi;
}
#pragma clang fp contract(on)

// ================================================================================================ launchers: the grid and block of each kernel above, for the engines and their stage taps
void launch_tln_fwd(const float* x, int M, int H, float eps, float* mean, float* rstd, const float* g1, const float* b1, float* y1, const float* g2,
                    const float* b2, float* y2, hipStream_t st) {
  hipLaunchKernelGGL(k_tln_fwd, dim3(M), dim3(64), 0, st, x, M, H, eps, mean, rstd, g1, b1, y1, g2, b2, y2);
}
void launch_tln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* g, int M, int H, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(k_tln_bwd, dim3(M), dim3(64), 0, st, dy, x, mean, rstd, g, H, dx);
}
void launch_tgelu(const float* x, float* y, long long n, hipStream_t st) { hipLaunchKernelGGL(k_tgelu, ew_grid(n), dim3(256), 0, st, x, y, n); }
void launch_tgelu_bwd(const float* x, float* dy, long long n, hipStream_t st) { hipLaunchKernelGGL(k_tgelu_bwd, ew_grid(n), dim3(256), 0, st, x, dy, n); }
void launch_tcolred(int mode, const float* dy, int ld, int M, int N, const float* x, const float* mean, const float* rstd, float* g0, float* g1,
                    hipStream_t st) {
  const dim3 grid((N + 31) / 32), block(256);
  if (mode == 1) hipLaunchKernelGGL(k_tcolred<1>, grid, block, 0, st, dy, ld, M, N, x, mean, rstd, g0, g1);
  else hipLaunchKernelGGL(k_tcolred<0>, grid, block, 0, st, dy, ld, M, N, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, g0, (float*)nullptr);
}

// the arguments of k_tadamw for optimizer step `step` (1-based): the step's scalars and the hyper-parameters, each a double rounded once
int adamw_check(const char* who, double lr, double beta1, double beta2, double eps, double weight_decay) {
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
    ETD_FAIL(ETD_EINVAL, "%s: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)", who);
  return ETD_OK;
}
AdamwArgs adamw_args(double max_norm, double norm, double lr, double beta1, double beta2, double eps, double weight_decay, long long step) {
  const StepScalars s = step_scalars(max_norm, norm, lr, beta1, beta2, step);
  return {s.coef, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), s.step_size, s.bc2_sqrt, (float)eps};
}
void launch_tadamw(float* p, float* g, float* m, float* v, long long n, const AdamwArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_tadamw, ew_grid(n), dim3(256), 0, st, p, g, m, v, n, a.coef, a.decay, a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.step_size, a.bc2_sqrt, a.eps);
}
