// Training of the source separator on the GPU (DESIGN.md 4n is the contract, tests/separator_train_np.py restates it): the U-Nets of csrc/separator.hip in
// training mode -- every norm on the batch's statistics --, Spleeter's L1 loss on the softmax estimates, the gradient of every kernel, bias, gamma and beta of every
// instrument, and torch.optim.Adam's single-tensor step.  One call is one batch: mix [B][T][F][C], target [I][B][T][F][C]; unit u = b * I + instrument.
//
//   k_sep_conv_mfma / _valu separator.hip's gather convolution, launched through sep_launch with the PLAIN epilogue (bias or none, two output tensors): every forward
//                           convolution and every input gradient -- conv dX = the four parity launches of the transposed geometry on channel-swapped kernels,
//                           transposed-conv dX = a stride-2 convolution of dy to [dskip | dup], head dX = the dilated correlation with the flipped kernel
//   k_st_dw                 weight gradients as a GEMM on v_mfma_f32_32x32x2_f32 with the forward's tile step (separator.h): M = taps x gathered channels, N = dense
//                           channels, K = (unit, position) in slices of ST_DW_SLICE rows; k_st_dw_reduce adds the slices' partials in slice order (fp64, rounded
//                           once) into the gradient
//   k_st_col / k_st_colfin  ordered column reductions: per-channel mean, centred variance, the norm's two backward sums, bias gradients.  fp32 partials of
//                           ST_COL_ROWS rows per workgroup, joined in chunk order in fp64
//   k_st_ew                 normalise + ELU (encoder), ELU + normalise (decoder) and their backward passes, xhat recomputed from the saved pre-norm tensor
//   k_st_loss               softmax over the instruments, |s_i mix - target_i| partials and dlogits in one pass
//   k_tsumsq / k_st_adam    the trainers' gradient norm (train_kernels.h) and torch.optim.Adam's step
//   k_st_dropout            decoder dropout (levels 1 .. 3, only when p > 0): y <- keep ? y s : 0 in place with a Philox4x32-10 mask that is a function of the element
//                           index, the level, the seed and the call counter; the backward pass runs the same kernel on dy, so no mask is stored
//
// fp32 throughout, no atomics: every sum runs in an order the shapes fix, so a call gives the same bits every time.
#include "separator_train.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "etude_hip_debug.h"
#include "train_store.h"

namespace {

__device__ __forceinline__ float st_elu(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float st_elu_grad(float x) { return x > 0.f ? 1.f : expf(x); }

// ================================================================================================ convolutions (the kernels: separator.hip, through sep_launch)
// dst [inst][a][b][r][c] = src [inst][kt(a)][kf(b)][c][r]: the taps of one output parity with the two channel axes swapped
__global__ void k_st_pack(const float* __restrict__ src, float* __restrict__ dst, int pt, int pf, int nt, int nf, int R, int Cc, long long src_is, long long total) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long long per = (long long)nt * nf * R * Cc;
  const int inst = (int)(e / per);
  long long q = e - (long long)inst * per;
  const int c = (int)(q % Cc); q /= Cc;
  const int r = (int)(q % R); q /= R;
  const int b = (int)(q % nf), a = (int)(q / nf);
  const int kt = sep_dec_tap(pt, a), kf = sep_dec_tap(pf, b);
  dst[e] = src[inst * src_is + ((long long)(kt * 5 + kf) * Cc + c) * R + r];
}

// ================================================================================================ weight gradients
// grid (M tiles, N tiles, instruments x slices).  Thread t loads column t & 63 of both tiles (m of A, n of B) at rows k = (t >> 6) + 4 r of the step; the sum over a
// slice runs in the order of separator.h's tile step, as the forward's does.
__global__ __launch_bounds__(SEP_THREADS) void k_st_dw(const StDw a) {
  __shared__ float As[SEP_BK][SEP_LD], Bs[SEP_BK][SEP_LD];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int m0 = blockIdx.x * SEP_BM, n0 = blockIdx.y * SEP_BN;
  const int inst = blockIdx.z / a.slices, sl = blockIdx.z - inst * a.slices;
  const int wr = w >> 1, wc = w & 1, half = l >> 5, l31 = l & 31;
  const int Mtot = a.nt * a.nf * a.Cg, N = a.N0 + a.N1, P = a.Hj * a.Wj;
  const long long Ktot = (long long)a.B * P;
  const long long kbeg = (long long)sl * ST_DW_SLICE, kend = kbeg + ST_DW_SLICE < Ktot ? kbeg + ST_DW_SLICE : Ktot;
  const int m = m0 + (t & 63), n = n0 + (t & 63);
  const bool mok = m < Mtot, nok = n < N;
  int offt = 0, offf = 0, cg = 0;
  if (mok) {
    const int tap = m / a.Cg, ta = tap / a.nf, tb = tap - ta * a.nf;
    cg = m - tap * a.Cg; offt = a.o0t + a.d * ta; offf = a.o0f + a.d * tb;
  }
  float ra[8], rb[8];
  f32x16 tot[4];
  sep_tile_zero(tot);
#define ST_DW_LOAD(k0)                                                                                       \
  {                                                                                                          \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                          \
      const long long k = (k0) + (t >> 6) + 4 * r;                                                           \
      float va = 0.f, vb = 0.f;                                                                              \
      if (k < kend) {                                                                                        \
        const int b = (int)(k / P), pos = (int)(k - (long long)b * P);                                       \
        const int jt = pos / a.Wj, jf = pos - jt * a.Wj;                                                     \
        const long long u = (long long)b * a.I + inst;                                                       \
        if (mok) {                                                                                           \
          const int it = a.S * jt + offt, jx = a.S * jf + offf;                                              \
          if (it >= 0 && it < a.Hg && jx >= 0 && jx < a.Wg) va = a.g[(u / a.g_div) * a.g_us + (long long)(it * a.Wg + jx) * a.Cg + cg]; \
        }                                                                                                    \
        if (nok) vb = n < a.N0 ? a.y0[u * a.y0_us + (long long)pos * a.N0 + n] : a.y1[u * a.y1_us + (long long)pos * a.N1 + (n - a.N0)]; \
      }                                                                                                      \
      ra[r] = va; rb[r] = vb;                                                                                \
    }                                                                                                        \
  }
  ST_DW_LOAD(kbeg)
  int step = 0;
  for (long long k0 = kbeg; k0 < kend; k0 += SEP_BK, ++step) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      As[(t >> 6) + 4 * r][t & 63] = ra[r];
      Bs[(t >> 6) + 4 * r][t & 63] = rb[r];
    }
    __syncthreads();
    if (k0 + SEP_BK < kend) ST_DW_LOAD(k0 + SEP_BK)
    sep_tile_step(As, Bs, wr * 32 + l31, wc * 32 + l31, half, step, tot);
  }
#undef ST_DW_LOAD
  const int col = n0 + wc * 32 + l31;
  if (col >= N) return;
  float* out = a.part + (long long)blockIdx.z * Mtot * N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wr * 32 + acc_row(r, half);
    if (row < Mtot) out[(long long)row * N + col] = sep_tile_total(tot, r);
  }
}

// grad [inst][MN] += the slices' partials, added in slice order in fp64 and rounded once
__global__ void k_st_dw_reduce(const float* __restrict__ part, int slices, long long MN, long long total, float* __restrict__ grad) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long long inst = e / MN, idx = e - inst * MN;
  double acc = 0.0;
  for (int s = 0; s < slices; ++s) acc += (double)part[(inst * slices + s) * MN + idx];
  grad[e] += (float)acc;
}

// ================================================================================================ column reductions
// grid (chunks, column tiles of CT, instruments); 256 threads = CT columns x 256 / CT row lanes.  A lane sums its rows of the chunk in row order; the lanes' sums
// are added in lane order.  The terms are fp32; the sums run in fp64 and a workgroup's partial is rounded to fp32 once.
__global__ __launch_bounds__(256) void k_st_col(const StCol a) {
  __shared__ double p1[256], p2[256];
  const int t = threadIdx.x, cl = t % a.CT, lane = t / a.CT, lanes = 256 / a.CT;
  const int c = blockIdx.y * a.CT + cl, inst = blockIdx.z;
  const long long R = (long long)a.B * a.P;
  const long long r0 = (long long)blockIdx.x * ST_COL_ROWS, r1 = r0 + ST_COL_ROWS < R ? r0 + ST_COL_ROWS : R;
  double s1 = 0.0, s2 = 0.0;      // fp32 terms, summed in fp64: a lane's chain of up to 256 rows and the 256 / CT lanes cost no rounding of their own
  if (c < a.C) {
    const int ic = inst * a.C + c;
    double mean = 0.0, rstd = 0.0;
    float gamma = 0.f, beta = 0.f;
    if (a.mode >= ST_COL_VAR) mean = a.mean[ic];
    if (a.mode >= ST_COL_BWD_ENC) { rstd = a.rstd[ic]; gamma = a.gamma[ic]; beta = a.beta[ic]; }
    for (long long r = r0 + lane; r < r1; r += lanes) {
      const long long b = r / a.P, pos = r - b * a.P;
      const long long o = (b * a.I + inst) * a.us + pos * a.C + c;
      const float x = a.x[o];
      switch (a.mode) {
        case ST_COL_X: s1 += (double)x; break;
        case ST_COL_ELU: s1 += (double)st_elu(x); break;
        case ST_COL_VAR: { const float dlt = (float)((double)x - mean); s1 += (double)(dlt * dlt); } break;
        case ST_COL_VAR_ELU: { const float dlt = (float)((double)st_elu(x) - mean); s1 += (double)(dlt * dlt); } break;
        case ST_COL_BWD_ENC: {
          const float xh = (float)(((double)x - mean) * rstd), dz = a.x2[o] * st_elu_grad(fmaf(gamma, xh, beta));
          s1 += (double)dz; s2 += (double)(dz * xh);
        } break;
        default: {
          const float xh = (float)(((double)st_elu(x) - mean) * rstd), dz = a.x2[o];
          s1 += (double)dz; s2 += (double)(dz * xh);
        } break;
      }
    }
  }
  p1[t] = s1; p2[t] = s2;
  __syncthreads();
  if (lane == 0 && c < a.C) {
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < lanes; ++j) { t1 += p1[j * a.CT + cl]; t2 += p2[j * a.CT + cl]; }
    const long long o = ((long long)inst * a.chunks + blockIdx.x) * a.C + c;
    a.part[o] = (float)t1;
    a.part[(long long)a.I * a.chunks * a.C + o] = (float)t2;
  }
}

// one thread per (instrument, column): the chunks' partials in chunk order, fp64.  o1 .. o3 by mode:
//   MEAN  o1 = mean            VAR  o1 = biased variance, o2 = 1 / sqrt(var + eps)
//   BWD   o1 = mean dz, o2 = mean dz xhat (zeros when the statistics are frozen), o3 += sum dz (beta's gradient), o4 += sum dz xhat (gamma's)
//   BIAS  o3 += sum
__global__ void k_st_colfin(const float* __restrict__ part, int chunks, int C, int I, long long R, int mode, float eps, int frozen, double* o1, double* o2, float* o3,
                            float* o4) {
  const int ic = blockIdx.x * blockDim.x + threadIdx.x;
  if (ic >= I * C) return;
  const int inst = ic / C, c = ic - inst * C;
  const float* q1 = part + (long long)inst * chunks * C + c;
  const float* q2 = q1 + (long long)I * chunks * C;
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < chunks; ++k) s1 += (double)q1[(long long)k * C];
  if (mode == ST_FIN_BWD)
    for (int k = 0; k < chunks; ++k) s2 += (double)q2[(long long)k * C];
  if (mode == ST_FIN_MEAN) {
    o1[ic] = s1 / (double)R;
  } else if (mode == ST_FIN_VAR) {
    const double var = s1 / (double)R;
    o1[ic] = var;
    o2[ic] = 1.0 / sqrt(var + (double)eps);
  } else if (mode == ST_FIN_BWD) {
    o1[ic] = frozen ? 0.0 : s1 / (double)R;
    o2[ic] = frozen ? 0.0 : s2 / (double)R;
    o3[ic] += (float)s1;
    o4[ic] += (float)s2;
  } else {
    o3[ic] += (float)s1;
  }
}

// frozen statistics: mean = the running mean, rstd = 1 / sqrt(running var + eps)
__global__ void k_st_frozen(const float* __restrict__ rmean, const float* __restrict__ rvar, float eps, int n, double* mean, double* rstd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mean[i] = (double)rmean[i];
  rstd[i] = 1.0 / sqrt((double)rvar[i] + (double)eps);
}

__global__ void k_st_d2f(const double* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)src[i];
}

#pragma clang fp contract(off)
// r <- m r + (1 - m) batch; 1 - m arrives as the host's double difference rounded once
__global__ void k_st_running(float* __restrict__ r, const double* __restrict__ batch, int n, float m, float one_minus_m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float keep = m * r[i], add = one_minus_m * (float)batch[i];
  r[i] = keep + add;
}
#pragma clang fp contract(on)

// ================================================================================================ elementwise
__global__ void k_st_ew(const StEw a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.total) return;
  const int ic = (int)((e / a.unit) % a.I) * a.C + (int)(e % a.C);
  // the statistics are fp64 and the differences against them are formed in fp64: a mean rounded to fp32 would shift every element of a channel the same way, an
  // error that a later sum over the channel (a bias or beta gradient, the next norm's mean) adds up coherently
  const float x = a.x[e], gamma = a.gamma[ic];
  const double mean = a.mean[ic], rstd = a.rstd[ic];
  if (a.mode == ST_EW_ENC) {
    a.out[e] = st_elu(fmaf(gamma, (float)(((double)x - mean) * rstd), a.beta[ic]));
  } else if (a.mode == ST_EW_DEC) {
    a.out[e] = fmaf(gamma, (float)(((double)st_elu(x) - mean) * rstd), a.beta[ic]);
  } else if (a.mode == ST_EW_ENC_BWD) {
    const float xh = (float)(((double)x - mean) * rstd), dz = a.dy[e] * st_elu_grad(fmaf(gamma, xh, a.beta[ic]));
    const float dx = (float)(((double)gamma * rstd) * (((double)dz - a.m1[ic]) - (double)xh * a.m2[ic]));
    a.out[e] = a.add ? dx + a.add[e] : dx;
  } else {
    const float xh = (float)(((double)st_elu(x) - mean) * rstd);
    const float de = (float)(((double)gamma * rstd) * (((double)a.dy[e] - a.m1[ic]) - (double)xh * a.m2[ic]));
    a.out[e] = de * st_elu_grad(x);
  }
}

// ================================================================================================ dropout
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): ten rounds of two 32 x 32 -> 64 multiplies, the key bumped by the Weyl constants
// between rounds.  Integer multiplies, shifts and xors only.
__device__ __forceinline__ void st_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one thread per four consecutive elements 4 g .. 4 g + 3 (one Philox block): out[e] = word(e & 3) < thr ? x[e] * s : 0.  out may be x.  vec: both pointers are
// 16-byte aligned, so a whole group moves as one float4.
__global__ __launch_bounds__(256) void k_st_dropout(const float* x, float* out, long long total, unsigned j, unsigned call, unsigned k0, unsigned k1, unsigned thr,
                                                   float s, int vec) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x, e0 = 4 * g;
  if (e0 >= total) return;
  unsigned w[4];
  st_philox((unsigned)(g & 0xffffffffLL), (unsigned)(g >> 32), j, call, k0, k1, w);
  if (vec && e0 + 3 < total) {
    float4 v = *reinterpret_cast<const float4*>(x + e0);
    v.x = w[0] < thr ? v.x * s : 0.f; v.y = w[1] < thr ? v.y * s : 0.f; v.z = w[2] < thr ? v.z * s : 0.f; v.w = w[3] < thr ? v.w * s : 0.f;
    *reinterpret_cast<float4*>(out + e0) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < total) out[e0 + i] = w[i] < thr ? x[e0 + i] * s : 0.f;
  }
}

// ================================================================================================ loss
// one (b, t, f, c) per thread: softmax over the instruments, sum_i |s_i mix - target_i|, dlogits_i = s_i (g_i - sum_j s_j g_j) with g_i = scale sign(s_i mix -
// target_i) mix (sign(0) = 0).  The workgroup's 256 losses are added by a fixed tree.
__global__ __launch_bounds__(256) void k_st_loss(const float* __restrict__ logits, const float* __restrict__ mix, const float* __restrict__ target, long long plane,
                                                int B, int I, float scale, float* __restrict__ partial, float* __restrict__ dlogits) {
  __shared__ float red[256];
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)B * plane;
  float loss = 0.f;
  if (e < total) {
    const long long b = e / plane, q = e - b * plane;
    const float* lg = logits + b * I * plane + q;
    float s[ETD_SEP_MAX_INSTR], g[ETD_SEP_MAX_INSTR];
    float mx = lg[0];
    for (int i = 1; i < I; ++i) mx = fmaxf(mx, lg[i * plane]);
    float den = 0.f;
    for (int i = 0; i < I; ++i) { s[i] = expf(lg[i * plane] - mx); den += s[i]; }
    const float m = mix[e];
    float dot = 0.f;
    for (int i = 0; i < I; ++i) {
      s[i] = s[i] / den;
      const float r = s[i] * m - target[((long long)i * B + b) * plane + q];
      loss += fabsf(r);
      g[i] = r > 0.f ? scale * m : r < 0.f ? -(scale * m) : 0.f;
      dot += s[i] * g[i];
    }
    if (dlogits)
      for (int i = 0; i < I; ++i) dlogits[(b * I + i) * plane + q] = s[i] * (g[i] - dot);
  }
  red[threadIdx.x] = loss;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// ================================================================================================ optimizer (the norm and the scalars: train_kernels.h)
#pragma clang fp contract(off)
// g *= coef (clipping; 1 without), then torch.optim.Adam's single-tensor step.  1 - beta arrive as the host's double differences rounded once.
__global__ void k_st_adam(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n, float coef, float one_minus_beta1,
                          float beta2, float one_minus_beta2, float step_size, float bc2_sqrt, float eps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = mul_scalar(g[i], coef);
  const float mi = fmaf(one_minus_beta1, gi - m[i], m[i]);                            // exp_avg.lerp_(grad, 1 - beta1): torch's CPU kernel ends in one fma
  const float vi = fmaf(mul_scalar(one_minus_beta2, gi), gi, mul_scalar(v[i], beta2));        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2): likewise
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] + mul_scalar(-step_size, mi) / denom;                                       // p.addcdiv_(exp_avg, denom, value = -step_size): the numerator is scaled first
  g[i] = gi; m[i] = mi; v[i] = vi;
}
#pragma clang fp contract(on)

}  // namespace

// ================================================================================================ the engine
struct StPar { long long off = 0, per = 0; };      // [I][per] at P + off

struct etd_septrain {
  etd_sep_cfg cfg;
  int I = 0, C = 0, max_units = 0;
  SepNet net;
  long long plane = 0, szmax = 0;      // floats of a segment and of the largest tensor of a unit
  StPar conv_w[ETD_SEP_LEVELS + 1], conv_b[ETD_SEP_LEVELS + 1], dec_w[ETD_SEP_LEVELS + 1], dec_b[ETD_SEP_LEVELS + 1], head_w, head_b;
  long long gam0 = 0, bet0 = 0, noff[2 * ETD_SEP_LEVELS + 2], NS = 0;                   // norm n's [I][C_n] block starts at noff[n] of every [NS] array
  TrainStore ps;                       // P = [trainable (n_train) | running mean [NS] | running var [NS]]; G, M1 and M2 hold the trainable part only
  std::vector<float> hP;               // the state until the first device call uploads it
  std::vector<float> h_loss;
  DevPool pool;
  double* S = nullptr;                                                                  // the norms' statistics in fp64: [mean | rstd | m1 | m2 | var], [NS] each
  float *dec_pk[ETD_SEP_LEVELS + 1][4], *conv_pk[ETD_SEP_LEVELS + 1][4];
  bool pack_dirty = true;
  double drop_p = 0.0; unsigned long long drop_seed = 0; long long drop_calls = 0;      // decoder dropout: off at p = 0; drop_calls counts the backward calls with p > 0
  Workspace ws;
  int normC(int n) const { return n <= ETD_SEP_LEVELS ? net.Cenc[n] : net.Cdout[n - ETD_SEP_LEVELS]; }
};

namespace {

inline unsigned st_grid(long long n, int threads = 256) { return (unsigned)((n + threads - 1) / threads); }

struct StPlan {                      // offsets in floats of the workspace of a call with B units per instrument
  long long pre[ETD_SEP_LEVELS + 1], act[ETD_SEP_LEVELS + 1], v[ETD_SEP_LEVELS + 1], y[ETD_SEP_LEVELS + 1], D[ETD_SEP_LEVELS + 1];
  long long logits = 0, E[2] = {0, 0}, part = 0, cpart = 0, lpart = 0, total_bytes = 0;
  long long loss_blocks = 0;
};

long long st_slices(long long rows) { return (rows + ST_DW_SLICE - 1) / ST_DW_SLICE; }

void st_plan(const etd_septrain* h, int B, StPlan* p) {
  const long long U = (long long)B * h->I;
  long long o = 0;
  auto take = [&](long long floats) { const long long at = o; o += (floats + 63) & ~63LL; return at; };
  long long part = 0, cpart = 0;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
    p->pre[l] = take(U * h->net.szE[l]);
    p->act[l] = l < ETD_SEP_LEVELS ? take(U * h->net.szE[l]) : 0;
    p->v[l] = take(U * h->net.szD[l]);
    p->y[l] = take(U * h->net.szD[l]);
    p->D[l] = take(U * h->net.szE[l]);
    const long long Pe = (long long)(h->cfg.T >> l) * (h->cfg.F >> l), Pd = (long long)(h->cfg.T >> (7 - l)) * (h->cfg.F >> (7 - l));
    part = std::max(part, st_slices(B * Pe) * h->conv_w[l].per);
    part = std::max(part, st_slices(B * Pd) * h->dec_w[l].per);
    cpart = std::max(cpart, ((B * Pe + ST_COL_ROWS - 1) / ST_COL_ROWS) * h->net.Cenc[l]);
    cpart = std::max(cpart, ((B * 4 * Pd + ST_COL_ROWS - 1) / ST_COL_ROWS) * h->net.Cdout[l]);
  }
  const long long Ph = (long long)h->cfg.T * h->cfg.F;
  part = std::max(part, st_slices(B * Ph) * h->head_w.per);
  cpart = std::max(cpart, ((B * Ph + ST_COL_ROWS - 1) / ST_COL_ROWS) * h->C);
  p->logits = take(U * h->plane);
  p->E[0] = take(U * h->szmax);
  p->E[1] = take(U * h->szmax);
  p->part = take(part * h->I);
  p->cpart = take(2 * cpart * h->I);
  p->loss_blocks = ((long long)B * h->plane + 255) / 256;
  p->lpart = take(p->loss_blocks);
  p->total_bytes = o * 4;
}

long long st_budget(const etd_septrain* h) { return h->cfg.workspace_bytes > 0 ? h->cfg.workspace_bytes : (16LL << 30); }

// the refusals of a call, before anything is launched
int st_check_batch(const etd_septrain* h, int B, StPlan* p, const char* who) {
  if (B < 1 || B > h->max_units) ETD_FAIL(ETD_EINVAL, "%s: B = %d units outside 1 .. max_units = %d", who, B, h->max_units);
  if ((long long)B * h->cfg.T * h->cfg.F > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "%s: B T F = %lld is above 2^31 - 1", who, (long long)B * h->cfg.T * h->cfg.F);
  st_plan(h, B, p);
  if (p->total_bytes > st_budget(h))
    ETD_FAIL(ETD_EINVAL, "%s: a batch of %d units needs %lld bytes of workspace, the budget is %lld (one call is one batch: there is no sub-batching)", who, B,
             p->total_bytes, st_budget(h));
  return ETD_OK;
}

int st_upload(etd_septrain* h) {
  DevPool& Q = h->pool;
  return Q.upload_once([&]() -> int {
    ETD_TRY(h->ps.upload(Q, h->hP.data(), h->ps.n_train));
    ETD_TRY(Q.alloc(&h->S, (size_t)(5 * h->NS), true));
    ETD_TRY(Q.alloc(&h->ps.partial, (size_t)TN_BLOCKS));
    for (int l = 1; l <= ETD_SEP_LEVELS; ++l)
      for (int par = 0; par < 4; ++par) {
        const long long taps = sep_dec_taps(par >> 1) * sep_dec_taps(par & 1);
        ETD_TRY(Q.alloc(&h->dec_pk[l][par], (size_t)(h->dec_w[l].per / 25 * taps * h->I)));
        if (l > 1) ETD_TRY(Q.alloc(&h->conv_pk[l][par], (size_t)(h->conv_w[l].per / 25 * taps * h->I)));
      }
    h->pack_dirty = true;
    return ETD_OK;
  });
}

// the parity-packed, channel-swapped copies of the kernels the forward's transposed convolutions and the encoder's input gradients read
int st_pack(etd_septrain* h, hipStream_t st) {
  if (!h->pack_dirty) return ETD_OK;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l)
    for (int par = 0; par < 4; ++par) {
      const int pt = par >> 1, pf = par & 1, nt = sep_dec_taps(pt), nf = sep_dec_taps(pf);
      {      // deconv l: [kt][kf][co][ci] -> [a][b][ci][co]
        const int Di = h->net.Cenc[7 - l] + (l > 1 ? h->net.Cdout[l - 1] : 0), Do = h->net.Cdout[l];
        const long long total = (long long)h->I * nt * nf * Di * Do;
        hipLaunchKernelGGL(k_st_pack, dim3(st_grid(total)), dim3(256), 0, st, h->ps.P + h->dec_w[l].off, h->dec_pk[l][par], pt, pf, nt, nf, Di, Do, h->dec_w[l].per, total);
      }
      if (l > 1) {      // conv l: [kt][kf][ci][co] -> [a][b][co][ci]
        const int Ci = h->net.Cenc[l - 1], Co = h->net.Cenc[l];
        const long long total = (long long)h->I * nt * nf * Ci * Co;
        hipLaunchKernelGGL(k_st_pack, dim3(st_grid(total)), dim3(256), 0, st, h->ps.P + h->conv_w[l].off, h->conv_pk[l][par], pt, pf, nt, nf, Co, Ci, h->conv_w[l].per, total);
      }
    }
  HIP_TRY(hipGetLastError());
  h->pack_dirty = false;
  return ETD_OK;
}

// a launch with the PLAIN epilogue: one output tensor with all N columns unless the caller splits them; unit u = b * I + instrument
SepLaunch st_conv_base(const etd_septrain* h) {
  SepLaunch a{};
  a.x0_div = 1; a.I = h->I; a.epi = SEP_EPI_PLAIN;
  return a;
}
int st_launch(SepLaunch& a, float* out, long long out_us, int U, bool force_valu, hipStream_t st) {
  a.N0 = a.N; a.pre = out; a.out_us = out_us;
  return sep_launch(a, U, force_valu, nullptr, st);
}

// ---- forward launches -------------------------------------------------------------------------------------------------------------------------------------------
int st_fwd_encoder(etd_septrain* h, int l, const float* x, float* pre, int U, hipStream_t st) {
  SepLaunch a = st_conv_base(h);
  sep_geom_encoder(h->net, l, &a);
  a.x0 = x;
  if (l == 1) { a.x0_us = h->plane; a.x0_div = h->I; } else { a.x0_us = h->net.szE[l - 1]; }
  a.W = h->ps.P + h->conv_w[l].off; a.w_is = h->conv_w[l].per; a.bias = h->ps.P + h->conv_b[l].off;
  return st_launch(a, pre, h->net.szE[l], U, false, st);
}

int st_fwd_decoder(etd_septrain* h, int j, const float* skip, const float* up, float* v, int U, hipStream_t st) {
  for (int par = 0; par < 4; ++par) {
    SepLaunch a = st_conv_base(h);
    sep_geom_deconv(h->net, j, par >> 1, par & 1, &a);
    a.x0 = skip; a.x0_us = h->net.szE[7 - j];
    a.x1 = j > 1 ? up : nullptr; a.x1_us = j > 1 ? h->net.szD[j - 1] : 0;
    a.W = h->dec_pk[j][par]; a.w_is = (long long)a.nt * a.nf * (a.C0 + a.C1) * a.N; a.bias = h->ps.P + h->dec_b[j].off;
    ETD_TRY(st_launch(a, v, h->net.szD[j], U, false, st));
  }
  return ETD_OK;
}

int st_fwd_head(etd_septrain* h, const float* x, float* logits, int U, hipStream_t st) {
  SepLaunch a = st_conv_base(h);
  sep_geom_head(h->net, &a);
  a.x0 = x; a.x0_us = (long long)h->cfg.T * h->cfg.F;
  a.W = h->ps.P + h->head_w.off; a.w_is = h->head_w.per; a.bias = h->ps.P + h->head_b.off;
  return st_launch(a, logits, h->plane, U, true, st);
}

// ---- input gradients (no bias) -----------------------------------------------------------------------------------------------------------------------------------
// conv l (l >= 2): dpre [T >> l][F >> l][Cenc l] -> dx [T >> (l-1)][F >> (l-1)][Cenc l-1]: the geometry of the transposed convolution at conv l's size (decoder
// 7 - l, whose output channels are Cenc l-1), without a second input
int st_dx_encoder(etd_septrain* h, int l, const float* dpre, float* dx, int U, hipStream_t st) {
  for (int par = 0; par < 4; ++par) {
    SepLaunch a = st_conv_base(h);
    sep_geom_deconv(h->net, 7 - l, par >> 1, par & 1, &a);
    a.C1 = 0;
    a.x0 = dpre; a.x0_us = h->net.szE[l];
    a.W = h->conv_pk[l][par]; a.w_is = (long long)a.nt * a.nf * a.C0 * a.N;
    ETD_TRY(st_launch(a, dx, h->net.szE[l - 1], U, false, st));
  }
  return ETD_OK;
}

// the convolution a transposed convolution's gradients run on: decoder j gathers dv [2H][2W][Cdout j] as conv 7 - j gathers its input, at the doubled size
SepLaunch st_geom_dv(const etd_septrain* h, int j) {
  SepLaunch a = st_conv_base(h);
  sep_geom_encoder(h->net, 7 - j, &a);
  a.C0 = h->net.Cdout[j];
  return a;
}

// decoder j: dv [2H][2W][Cdout j] -> dskip [H][W][Cenc 7-j] and dup [H][W][Cdout j-1] (j > 1)
int st_dx_decoder(etd_septrain* h, int j, const float* dv, float* dskip, float* dup, int U, hipStream_t st) {
  SepLaunch a = st_geom_dv(h, j);
  a.x0 = dv; a.x0_us = h->net.szD[j];
  a.N0 = a.N; a.N = a.N0 + (j > 1 ? h->net.Cdout[j - 1] : 0);
  a.W = h->ps.P + h->dec_w[j].off; a.w_is = h->dec_w[j].per;      // [kt][kf][co][ci] is this GEMM's [K][N]
  a.out1 = dup; a.out1_us = j > 1 ? h->net.szD[j - 1] : 0;
  a.pre = dskip; a.out_us = h->net.szE[7 - j];
  return sep_launch(a, U, false, nullptr, st);
}

// head: dlogits [T][F][C] -> dx [T][F][1]: the head's geometry with offset and dilation negated and the channels swapped
int st_dx_head(etd_septrain* h, const float* dlogits, float* dx, int U, hipStream_t st) {
  SepLaunch a = st_conv_base(h);
  sep_geom_head(h->net, &a);
  a.o0t = -a.o0t; a.o0f = -a.o0f; a.d = -a.d; a.C0 = h->C; a.N = 1;
  a.x0 = dlogits; a.x0_us = h->plane;
  a.W = h->ps.P + h->head_w.off; a.w_is = h->head_w.per;          // [kt][kf][1][co] read as [K = (tap, co)][1]
  return st_launch(a, dx, (long long)h->cfg.T * h->cfg.F, U, true, st);
}

// ---- weight gradients --------------------------------------------------------------------------------------------------------------------------------------------
// g: the gathered tensor, read as the convolution `c` reads its first input; y = [y0 | y1]: the dense one, at c's Hj x Wj positions
int st_dw(etd_septrain* h, const SepLaunch& c, const float* g, long long g_us, int g_div, const float* y0, long long y0_us, int N0, const float* y1, long long y1_us,
          int N1, int B, float* part, float* grad, hipStream_t st) {
  StDw a{};
  a.g = g; a.g_us = g_us; a.g_div = g_div; a.Cg = c.C0; a.Hg = c.Hin; a.Wg = c.Win;
  a.S = c.S; a.o0t = c.o0t; a.o0f = c.o0f; a.d = c.d; a.nt = c.nt; a.nf = c.nf; a.Hj = c.Hj; a.Wj = c.Wj;
  a.y0 = y0; a.y0_us = y0_us; a.N0 = N0; a.y1 = y1; a.y1_us = y1_us; a.N1 = N1;
  const long long rows = (long long)B * a.Hj * a.Wj;
  a.B = B; a.I = h->I; a.slices = (int)st_slices(rows); a.part = part;
  const long long M = (long long)a.nt * a.nf * a.Cg, N = a.N0 + a.N1;
  const dim3 grid((unsigned)((M + SEP_BM - 1) / SEP_BM), (unsigned)((N + SEP_BN - 1) / SEP_BN), (unsigned)(h->I * a.slices));
  if (grid.z > 65535u) ETD_FAIL(ETD_EINVAL, "separator training: a weight gradient needs %u slices x instruments (> 65535)", grid.z);
  hipLaunchKernelGGL(k_st_dw, grid, dim3(SEP_THREADS), 0, st, a);
  const long long total = (long long)h->I * M * N;
  hipLaunchKernelGGL(k_st_dw_reduce, dim3(st_grid(total)), dim3(256), 0, st, part, a.slices, M * N, total, grad);
  return ETD_OK;
}

int st_dw_encoder(etd_septrain* h, int l, const float* x, const float* dpre, int B, float* part, float* grad, hipStream_t st) {
  SepLaunch c{};
  sep_geom_encoder(h->net, l, &c);
  return st_dw(h, c, x, l == 1 ? h->plane : h->net.szE[l - 1], l == 1 ? h->I : 1, dpre, h->net.szE[l], c.N, nullptr, 0, 0, B, part, grad, st);
}

int st_dw_decoder(etd_septrain* h, int j, const float* skip, const float* up, const float* dv, int B, float* part, float* grad, hipStream_t st) {
  return st_dw(h, st_geom_dv(h, j), dv, h->net.szD[j], 1, skip, h->net.szE[7 - j], h->net.Cenc[7 - j], j > 1 ? up : nullptr, j > 1 ? h->net.szD[j - 1] : 0,
               j > 1 ? h->net.Cdout[j - 1] : 0, B, part, grad, st);
}

int st_dw_head(etd_septrain* h, const float* x, const float* dlogits, int B, float* part, float* grad, hipStream_t st) {
  SepLaunch c{};
  sep_geom_head(h->net, &c);
  return st_dw(h, c, x, (long long)h->cfg.T * h->cfg.F, 1, dlogits, h->plane, h->C, nullptr, 0, 0, B, part, grad, st);
}

// ---- reductions and elementwise passes ---------------------------------------------------------------------------------------------------------------------------
double* st_S(etd_septrain* h, int which, int n) { return h->S + (long long)which * h->NS + h->noff[n]; }      // which: 0 mean, 1 rstd, 2 m1, 3 m2, 4 var

// one reduction of x [U][P][C] (mode, second tensor x2) and its join; norm n's statistics and affine are read when the mode needs them
int st_col(etd_septrain* h, int mode, int n, const float* x, const float* x2, long long P, int C, int B, float* cpart, int fin, int frozen, double* o1, double* o2,
           float* o3, float* o4, hipStream_t st) {
  StCol a{};
  a.x = x; a.x2 = x2; a.us = P * C; a.P = (int)P; a.C = C; a.B = B; a.I = h->I; a.mode = mode;
  const long long R = (long long)B * P;
  a.chunks = (int)((R + ST_COL_ROWS - 1) / ST_COL_ROWS);
  int CT = 1;
  while (CT < C && CT < 64) CT <<= 1;
  a.CT = CT;
  if (n > 0) { a.mean = st_S(h, 0, n); a.rstd = st_S(h, 1, n); a.gamma = h->ps.P + h->gam0 + h->noff[n]; a.beta = h->ps.P + h->bet0 + h->noff[n]; }
  a.part = cpart;
  hipLaunchKernelGGL(k_st_col, dim3((unsigned)a.chunks, (unsigned)((C + CT - 1) / CT), (unsigned)h->I), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_st_colfin, dim3(st_grid((long long)h->I * C, 64)), dim3(64), 0, st, cpart, a.chunks, C, h->I, R, fin, h->cfg.bn_eps, frozen, o1, o2, o3, o4);
  return ETD_OK;
}

// the batch statistics of norm n over x [U][P][C] (the decoder's norms: over ELU(x)): the mean, then the centred biased variance
int st_stats(etd_septrain* h, int n, const float* x, long long P, int B, float* cpart, hipStream_t st) {
  const bool dec = n > ETD_SEP_LEVELS;
  const int C = h->normC(n);
  ETD_TRY(st_col(h, dec ? ST_COL_ELU : ST_COL_X, n, x, nullptr, P, C, B, cpart, ST_FIN_MEAN, 0, st_S(h, 0, n), nullptr, nullptr, nullptr, st));
  return st_col(h, dec ? ST_COL_VAR_ELU : ST_COL_VAR, n, x, nullptr, P, C, B, cpart, ST_FIN_VAR, 0, st_S(h, 4, n), st_S(h, 1, n), nullptr, nullptr, st);
}

int st_ew(etd_septrain* h, int mode, int n, const float* x, const float* dy, const float* add, float* out, long long unit, int U, hipStream_t st) {
  StEw a{};
  a.x = x; a.dy = dy; a.add = add; a.out = out; a.unit = unit; a.total = unit * U; a.C = h->normC(n); a.I = h->I; a.mode = mode;
  a.mean = st_S(h, 0, n); a.rstd = st_S(h, 1, n); a.m1 = st_S(h, 2, n); a.m2 = st_S(h, 3, n);
  a.gamma = h->ps.P + h->gam0 + h->noff[n]; a.beta = h->ps.P + h->bet0 + h->noff[n];
  const long long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator training: an elementwise pass needs %lld workgroups (> 2^31 - 1)", blocks);
  hipLaunchKernelGGL(k_st_ew, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return ETD_OK;
}

// the norm's backward for norm n: the two sums (gamma's and beta's gradients are added to G), then dx.  Encoder: x = pre, dy = dact, out = dx + add;
// decoder: x = v, dy = dy, out = dv (may alias dy)
int st_norm_bwd(etd_septrain* h, int n, const float* x, const float* dy, const float* add, float* out, long long P, int B, int frozen, float* cpart, hipStream_t st) {
  const bool dec = n > ETD_SEP_LEVELS;
  const int C = h->normC(n);
  ETD_TRY(st_col(h, dec ? ST_COL_BWD_DEC : ST_COL_BWD_ENC, n, x, dy, P, C, B, cpart, ST_FIN_BWD, frozen, st_S(h, 2, n), st_S(h, 3, n), h->ps.G + h->bet0 + h->noff[n],
                 h->ps.G + h->gam0 + h->noff[n], st));
  return st_ew(h, dec ? ST_EW_DEC_BWD : ST_EW_ENC_BWD, n, x, dy, add, out, P * C, B * h->I, st);
}

int st_bias_grad(etd_septrain* h, const float* dy, long long P, int C, int B, float* cpart, float* grad, hipStream_t st) {
  return st_col(h, ST_COL_X, 0, dy, nullptr, P, C, B, cpart, ST_FIN_BIAS, 0, nullptr, nullptr, grad, nullptr, st);
}

int st_loss(etd_septrain* h, const float* logits, const float* mix, const float* target, int B, double loss_scale, float* lpart, long long blocks, float* dlogits,
            double* loss_out, hipStream_t st) {
  const double count = (double)h->I * B * (double)h->plane;
  hipLaunchKernelGGL(k_st_loss, dim3((unsigned)blocks), dim3(256), 0, st, logits, mix, target, h->plane, B, h->I, (float)(loss_scale / count), lpart, dlogits);
  HIP_TRY(hipGetLastError());
  h->h_loss.resize((size_t)blocks);
  HIP_TRY(hipMemcpyAsync(h->h_loss.data(), lpart, sizeof(float) * blocks, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double tot = 0.0;
  for (long long i = 0; i < blocks; ++i) tot += (double)h->h_loss[(size_t)i];
  *loss_out = tot / count;
  return ETD_OK;
}

// y_j <- keep ? y_j s : 0 (or the same on dy_j) over n elements of decoder level j at call counter `call`; s and the threshold are formed in double
int st_dropout(const etd_septrain* h, int j, long long call, const float* x, float* out, long long n, hipStream_t st) {
  const float s = (float)(1.0 / (1.0 - h->drop_p));
  const double t = floor((1.0 - h->drop_p) * 4294967296.0);
  const unsigned thr = t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
  const long long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator training: dropout needs %lld workgroups (> 2^31 - 1)", blocks);
  const int vec = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  hipLaunchKernelGGL(k_st_dropout, dim3((unsigned)blocks), dim3(256), 0, st, x, out, n, (unsigned)j, (unsigned)(call & 0xffffffffLL),
                     (unsigned)(h->drop_seed & 0xffffffffULL), (unsigned)(h->drop_seed >> 32), thr, s, vec);
  return ETD_OK;
}
#define ST_DROP_LEVELS 3

}  // namespace

extern "C" int etd_septrain_create(const etd_sep_cfg* cfg, int max_units, const char* const* instr_names, const char* const* names, const float* const* host_ptrs,
                                   const int64_t* numels, int n, etd_septrain** out) {
  if (!cfg || !out || !instr_names || !names || !host_ptrs || !numels || n < 0) ETD_FAIL(ETD_EINVAL, "septrain_create: null argument");
  {      // the config, the keys, the sizes and the finiteness of the state: etd_sep_create's own refusals (no GPU is touched)
    etd_sep* probe = nullptr;
    ETD_TRY(etd_sep_create(cfg, instr_names, names, host_ptrs, numels, n, &probe));
    etd_sep_destroy(probe);
  }
  const etd_sep_cfg& c = *cfg;
  if (max_units < 1 || (long long)max_units * c.n_instr > 16384) ETD_FAIL(ETD_EINVAL, "septrain_create: max_units = %d must be in 1 .. 16384 / n_instr", max_units);
  etd_septrain* h = new etd_septrain();
  h->cfg = c; h->I = c.n_instr; h->C = c.n_channels; h->max_units = max_units;
  sep_net_init(&h->net, c);
  h->plane = (long long)c.T * c.F * c.n_channels;
  h->szmax = h->plane;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) h->szmax = std::max(h->szmax, std::max(h->net.szE[l], h->net.szD[l]));
  const long long I = h->I;
  long long o = 0;
  auto place = [&](StPar& p, long long per) { p.off = o; p.per = per; o += per * I; };
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
    place(h->conv_w[l], 25LL * h->net.Cenc[l - 1] * h->net.Cenc[l]);
    place(h->conv_b[l], h->net.Cenc[l]);
    const long long Di = h->net.Cenc[7 - l] + (l > 1 ? h->net.Cdout[l - 1] : 0);
    place(h->dec_w[l], 25LL * h->net.Cdout[l] * Di);
    place(h->dec_b[l], h->net.Cdout[l]);
  }
  place(h->head_w, 16LL * c.n_channels);
  place(h->head_b, c.n_channels);
  long long ns = 0;
  for (int nn = 1; nn <= 2 * ETD_SEP_LEVELS; ++nn) { h->noff[nn] = ns; ns += I * h->normC(nn); }
  h->NS = ns;
  h->gam0 = o; o += ns;
  h->bet0 = o; o += ns;
  const long long n_train = o;
  h->ps.n_train = (size_t)o;
  h->ps.n_total = (size_t)(o + 2 * ns);
  auto put = [&](const std::string& key, long long off, long long numel) { h->ps.add_at(key, (size_t)off, (size_t)numel); };
  for (int i = 0; i < I; ++i) {
    const std::string pre = std::string(instr_names[i]) + ".";
    for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
      const std::string sl = std::to_string(l);
      put(pre + "conv" + sl + ".weight", h->conv_w[l].off + i * h->conv_w[l].per, h->conv_w[l].per);
      put(pre + "conv" + sl + ".bias", h->conv_b[l].off + i * h->conv_b[l].per, h->conv_b[l].per);
      put(pre + "deconv" + sl + ".weight", h->dec_w[l].off + i * h->dec_w[l].per, h->dec_w[l].per);
      put(pre + "deconv" + sl + ".bias", h->dec_b[l].off + i * h->dec_b[l].per, h->dec_b[l].per);
    }
    for (int nn = 1; nn <= 2 * ETD_SEP_LEVELS; ++nn) {
      const long long Cn = h->normC(nn), at = h->noff[nn] + i * Cn;
      const std::string k = pre + "bn" + std::to_string(nn);
      put(k + ".gamma", h->gam0 + at, Cn);
      put(k + ".beta", h->bet0 + at, Cn);
      put(k + ".mean", n_train + at, Cn);
      put(k + ".var", n_train + ns + at, Cn);
    }
    put(pre + "head.weight", h->head_w.off + i * h->head_w.per, h->head_w.per);
    put(pre + "head.bias", h->head_b.off + i * h->head_b.per, h->head_b.per);
  }
  h->hP.assign(h->ps.n_total, 0.f);
  (void)h->ps.fill(WeightTable(names, host_ptrs, numels, n), h->hP.data());      // (every key is present and of this size: etd_sep_create has checked)
  *out = h;
  return ETD_OK;
}

extern "C" void etd_septrain_destroy(etd_septrain* h) {
  if (!h) return;
  h->pool.release_uploaded();
  h->ws.release();
  delete h;
}

extern "C" long long etd_septrain_workspace_bytes(const etd_septrain* h, int B) {
  if (!h || B < 1) { g_etd_err = "septrain_workspace_bytes: null handle or B < 1"; return ETD_EINVAL; }
  StPlan p;
  st_plan(h, B, &p);
  return p.total_bytes;
}

extern "C" double etd_septrain_step_flops(const etd_septrain* h, int B) {
  if (!h) return 0.0;
  double f = 0.0;      // one forward's multiply-adds that are not structural zeros
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
    f += 2.0 * h->net.posE(l) * 25.0 * h->net.Cenc[l - 1] * h->net.Cenc[l];
    f += 2.0 * (h->net.posD(l) / 4) * (double)h->dec_w[l].per;
  }
  f += 2.0 * (double)h->cfg.T * h->cfg.F * 16.0 * h->C;
  return 3.0 * f * h->I * B;      // forward, input gradient, weight gradient
}

extern "C" int etd_septrain_forward_backward(etd_septrain* h, const float* mix, const float* target, int B, double loss_scale, int frozen_stats, int backward,
                                             double* loss_out, void* stream) {
  if (!h || !mix || !target || !loss_out) ETD_FAIL(ETD_EINVAL, "septrain_forward_backward: null argument");
  if (!std::isfinite(loss_scale)) ETD_FAIL(ETD_EINVAL, "septrain_forward_backward: loss_scale is not finite");
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_forward_backward"));
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  ETD_TRY(h->ws.reserve(p.total_bytes, st));
  ETD_TRY(st_pack(h, st));
  float* ws = (float*)h->ws.p;
  float* cpart = ws + p.cpart;
  const int U = B * h->I, L = ETD_SEP_LEVELS;
  const bool drop = backward && h->drop_p > 0.0;      // never in the loss-only (validation) path
  if (frozen_stats) hipLaunchKernelGGL(k_st_frozen, dim3(st_grid(h->NS)), dim3(256), 0, st, h->ps.P + h->ps.n_train, h->ps.P + h->ps.n_train + h->NS, h->cfg.bn_eps, (int)h->NS, h->S, h->S + h->NS);
  // ---- forward
  for (int l = 1; l <= L; ++l) {
    ETD_TRY(st_fwd_encoder(h, l, l == 1 ? mix : ws + p.act[l - 1], ws + p.pre[l], U, st));
    if (!frozen_stats) ETD_TRY(st_stats(h, l, ws + p.pre[l], h->net.posE(l), B, cpart, st));
    if (l < L) ETD_TRY(st_ew(h, ST_EW_ENC, l, ws + p.pre[l], nullptr, nullptr, ws + p.act[l], h->net.szE[l], U, st));
  }
  for (int j = 1; j <= L; ++j) {
    ETD_TRY(st_fwd_decoder(h, j, ws + p.pre[7 - j], j > 1 ? ws + p.y[j - 1] : nullptr, ws + p.v[j], U, st));
    if (!frozen_stats) ETD_TRY(st_stats(h, L + j, ws + p.v[j], h->net.posD(j), B, cpart, st));
    ETD_TRY(st_ew(h, ST_EW_DEC, L + j, ws + p.v[j], nullptr, nullptr, ws + p.y[j], h->net.szD[j], U, st));
    if (drop && j <= ST_DROP_LEVELS) ETD_TRY(st_dropout(h, j, h->drop_calls, ws + p.y[j], ws + p.y[j], U * h->net.szD[j], st));      // after the statistics, before any reader
  }
  ETD_TRY(st_fwd_head(h, ws + p.y[L], ws + p.logits, U, st));
  if (!frozen_stats) {      // the running statistics move once per call
    const float m = (float)ST_BN_MOMENTUM, om = (float)(1.0 - ST_BN_MOMENTUM);
    hipLaunchKernelGGL(k_st_running, dim3(st_grid(h->NS)), dim3(256), 0, st, h->ps.P + h->ps.n_train, h->S, (int)h->NS, m, om);
    hipLaunchKernelGGL(k_st_running, dim3(st_grid(h->NS)), dim3(256), 0, st, h->ps.P + h->ps.n_train + h->NS, h->S + 4 * h->NS, (int)h->NS, m, om);
  }
  HIP_TRY(hipGetLastError());
  float *cur = ws + p.E[0], *other = ws + p.E[1];
  if (!backward) return st_loss(h, ws + p.logits, mix, target, B, loss_scale, ws + p.lpart, p.loss_blocks, nullptr, loss_out, st);
  // ---- backward
  ETD_TRY(st_loss(h, ws + p.logits, mix, target, B, loss_scale, ws + p.lpart, p.loss_blocks, cur, loss_out, st));
  float* part = ws + p.part;
  ETD_TRY(st_bias_grad(h, cur, (long long)h->cfg.T * h->cfg.F, h->C, B, cpart, h->ps.G + h->head_b.off, st));
  ETD_TRY(st_dw_head(h, ws + p.y[L], cur, B, part, h->ps.G + h->head_w.off, st));
  ETD_TRY(st_dx_head(h, cur, other, U, st));
  std::swap(cur, other);
  for (int j = L; j >= 1; --j) {      // cur = dy_j
    if (drop && j <= ST_DROP_LEVELS) ETD_TRY(st_dropout(h, j, h->drop_calls, cur, cur, U * h->net.szD[j], st));      // the forward's mask, regenerated
    ETD_TRY(st_norm_bwd(h, L + j, ws + p.v[j], cur, nullptr, cur, h->net.posD(j), B, frozen_stats, cpart, st));      // cur = dv_j
    ETD_TRY(st_bias_grad(h, cur, h->net.posD(j), h->net.Cdout[j], B, cpart, h->ps.G + h->dec_b[j].off, st));
    ETD_TRY(st_dw_decoder(h, j, ws + p.pre[7 - j], j > 1 ? ws + p.y[j - 1] : nullptr, cur, B, part, h->ps.G + h->dec_w[j].off, st));
    ETD_TRY(st_dx_decoder(h, j, cur, ws + p.D[7 - j], other, U, st));
    std::swap(cur, other);
  }
  for (int l = L; l >= 1; --l) {      // D[l] = the skip's gradient; cur = dact_l for l < 6 (conv_6's normalised output is read by nothing)
    if (l < L) ETD_TRY(st_norm_bwd(h, l, ws + p.pre[l], cur, ws + p.D[l], ws + p.D[l], h->net.posE(l), B, frozen_stats, cpart, st));
    ETD_TRY(st_bias_grad(h, ws + p.D[l], h->net.posE(l), h->net.Cenc[l], B, cpart, h->ps.G + h->conv_b[l].off, st));
    ETD_TRY(st_dw_encoder(h, l, l == 1 ? mix : ws + p.act[l - 1], ws + p.D[l], B, part, h->ps.G + h->conv_w[l].off, st));
    if (l > 1) {
      ETD_TRY(st_dx_encoder(h, l, ws + p.D[l], other, U, st));
      std::swap(cur, other);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  if (drop) h->drop_calls += 1;
  return ETD_OK;
}

extern "C" int etd_septrain_set_dropout(etd_septrain* h, double p, unsigned long long seed) {
  if (!h) ETD_FAIL(ETD_EINVAL, "septrain_set_dropout: null handle");
  if (!(p >= 0.0 && p < 1.0)) ETD_FAIL(ETD_EINVAL, "septrain_set_dropout: p = %g is outside [0, 1)", p);
  h->drop_p = p; h->drop_seed = seed;
  return ETD_OK;
}
extern "C" int etd_septrain_set_dropout_calls(etd_septrain* h, long long calls) {
  if (!h || calls < 0) ETD_FAIL(ETD_EINVAL, "septrain_set_dropout_calls: null handle or a negative count");
  h->drop_calls = calls;
  return ETD_OK;
}
extern "C" long long etd_septrain_get_dropout_calls(const etd_septrain* h) { return h ? h->drop_calls : ETD_EINVAL; }

extern "C" int etd_septrain_zero_grad(etd_septrain* h, void* stream) {
  if (!h) ETD_FAIL(ETD_EINVAL, "septrain_zero_grad: null handle");
  ETD_TRY(st_upload(h));
  return h->ps.zero_grad(h->ps.n_train, (hipStream_t)stream);
}

extern "C" int etd_septrain_grad_norm(etd_septrain* h, double* norm, void* stream) {
  if (!h || !norm) ETD_FAIL(ETD_EINVAL, "septrain_grad_norm: null argument");
  ETD_TRY(st_upload(h));
  return h->ps.grad_norm(h->ps.n_train, (hipStream_t)stream, norm);
}

extern "C" int etd_septrain_step(etd_septrain* h, double max_norm, double lr, double beta1, double beta2, double eps, double* norm_out, void* stream) {
  if (!h) ETD_FAIL(ETD_EINVAL, "septrain_step: null handle");
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    ETD_FAIL(ETD_EINVAL, "septrain_step: lr and eps must be >= 0 and the betas in [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  TrainStore& ps = h->ps;
  double norm = 0.0;                                   // max_norm <= 0: no clipping, and no norm unless the caller asks
  if (max_norm > 0.0 || norm_out) ETD_TRY(ps.grad_norm(ps.n_train, st, &norm));
  if (norm_out) *norm_out = norm;
  ps.step += 1;
  const StepScalars s = step_scalars(max_norm, norm, lr, beta1, beta2, ps.step);
  hipLaunchKernelGGL(k_st_adam, dim3(st_grid((long long)ps.n_train)), dim3(256), 0, st, ps.P, ps.G, ps.M1, ps.M2, (long long)ps.n_train, s.coef, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), s.step_size, s.bc2_sqrt, (float)eps);
  HIP_TRY(hipGetLastError());
  h->pack_dirty = true;
  return ETD_OK;
}

extern "C" int etd_septrain_set_step(etd_septrain* h, long long step) {
  if (!h || step < 0) ETD_FAIL(ETD_EINVAL, "septrain_set_step: null handle or negative step");
  h->ps.step = step;
  return ETD_OK;
}
extern "C" long long etd_septrain_get_step(const etd_septrain* h) { return h ? h->ps.step : ETD_EINVAL; }

// which: 0 state (parameters and running statistics), 1 gradient, 2 exp_avg, 3 exp_avg_sq.  The store's checks, and around them what is the separator's own
static int septrain_io(etd_septrain* h, const char* name, int which, float* out, const float* in, long long numel, hipStream_t st) {
  if (!h || !name || (!out && !in)) ETD_FAIL(ETD_EINVAL, "etd_septrain: null argument");
  if (which < 0 || which > 3) ETD_FAIL(ETD_EINVAL, "etd_septrain: which = %d is not 0 .. 3", which);
  const TrainStore::Tensor* t = nullptr;
  ETD_TRY(h->ps.find("etd_septrain", "tensor", name, numel, &t));
  if (which > 0 && t->off >= h->ps.n_train) ETD_FAIL(ETD_EINVAL, "etd_septrain: '%s' is a running statistic: it has no gradient and no moments", name);
  if (!h->pool.uploaded && out) {      // the state is the host's copy, and the gradients and moments are zeros
    if (which == 0) memcpy(out, &h->hP[t->off], sizeof(float) * t->n);
    else memset(out, 0, sizeof(float) * t->n);
    return ETD_OK;
  }
  ETD_TRY(st_upload(h));
  return h->ps.copy(*t, which, out, in, st);
}

extern "C" int etd_septrain_read(etd_septrain* h, const char* name, int which, float* out_host, long long numel, void* stream) {
  if (!out_host) ETD_FAIL(ETD_EINVAL, "septrain_read: null buffer");
  return septrain_io(h, name, which, out_host, nullptr, numel, (hipStream_t)stream);
}

extern "C" int etd_septrain_write_moment(etd_septrain* h, const char* name, int second, const float* in_host, long long numel, void* stream) {
  if (!in_host || second < 0 || second > 1) ETD_FAIL(ETD_EINVAL, "septrain_write_moment: null buffer or second not 0 / 1");
  return septrain_io(h, name, 2 + second, nullptr, in_host, numel, (hipStream_t)stream);
}

// ================================================================================================ stage taps (include/etude_hip_debug.h)
extern "C" int etd_septrain_debug_dx(etd_septrain* h, int kind, int layer, const float* dy_dev, int B, float* out0_dev, float* out1_dev, void* stream) {
  if (!h || !dy_dev || !out0_dev) ETD_FAIL(ETD_EINVAL, "septrain_debug_dx: null argument");
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_debug_dx"));
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  ETD_TRY(st_pack(h, st));
  const int U = B * h->I;
  if (kind == 0) {
    if (layer < 2 || layer > ETD_SEP_LEVELS) ETD_FAIL(ETD_EINVAL, "septrain_debug_dx: encoder layer = %d outside 2 .. %d", layer, ETD_SEP_LEVELS);
    ETD_TRY(st_dx_encoder(h, layer, dy_dev, out0_dev, U, st));
  } else if (kind == 1) {
    if (layer < 1 || layer > ETD_SEP_LEVELS || (layer > 1 && !out1_dev)) ETD_FAIL(ETD_EINVAL, "septrain_debug_dx: decoder layer = %d outside 1 .. %d, or no out1", layer, ETD_SEP_LEVELS);
    ETD_TRY(st_dx_decoder(h, layer, dy_dev, out0_dev, out1_dev, U, st));
  } else if (kind == 2) {
    ETD_TRY(st_dx_head(h, dy_dev, out0_dev, U, st));
  } else {
    ETD_FAIL(ETD_EINVAL, "septrain_debug_dx: kind = %d is not 0, 1 or 2", kind);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_septrain_debug_dw(etd_septrain* h, int kind, int layer, const float* x0_dev, const float* x1_dev, const float* dy_dev, int B, float* dw_dev,
                                     void* stream) {
  if (!h || !x0_dev || !dy_dev || !dw_dev) ETD_FAIL(ETD_EINVAL, "septrain_debug_dw: null argument");
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_debug_dw"));
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  ETD_TRY(h->ws.reserve(p.total_bytes, st));
  float* part = (float*)h->ws.p + p.part;
  if (kind != 2 && (layer < 1 || layer > ETD_SEP_LEVELS)) ETD_FAIL(ETD_EINVAL, "septrain_debug_dw: layer = %d outside 1 .. %d", layer, ETD_SEP_LEVELS);
  if (kind == 0) {
    ETD_TRY(st_dw_encoder(h, layer, x0_dev, dy_dev, B, part, dw_dev, st));
  } else if (kind == 1) {
    if (layer > 1 && !x1_dev) ETD_FAIL(ETD_EINVAL, "septrain_debug_dw: decoder layer %d needs x1", layer);
    ETD_TRY(st_dw_decoder(h, layer, x0_dev, x1_dev, dy_dev, B, part, dw_dev, st));
  } else if (kind == 2) {
    ETD_TRY(st_dw_head(h, x0_dev, dy_dev, B, part, dw_dev, st));
  } else {
    ETD_FAIL(ETD_EINVAL, "septrain_debug_dw: kind = %d is not 0, 1 or 2", kind);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_septrain_debug_norm(etd_septrain* h, int norm, const float* x_dev, int B, const float* dy_dev, float* y_dev, float* dx_dev, float* stats_dev,
                                       void* stream) {
  if (!h || !x_dev || !y_dev || (dy_dev && !dx_dev)) ETD_FAIL(ETD_EINVAL, "septrain_debug_norm: null argument");
  if (norm < 1 || norm > 2 * ETD_SEP_LEVELS) ETD_FAIL(ETD_EINVAL, "septrain_debug_norm: norm = %d outside 1 .. %d", norm, 2 * ETD_SEP_LEVELS);
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_debug_norm"));
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  ETD_TRY(h->ws.reserve(p.total_bytes, st));
  float* cpart = (float*)h->ws.p + p.cpart;
  const bool dec = norm > ETD_SEP_LEVELS;
  const long long P = dec ? h->net.posD(norm - ETD_SEP_LEVELS) : h->net.posE(norm);
  const int C = h->normC(norm), U = B * h->I;
  ETD_TRY(st_stats(h, norm, x_dev, P, B, cpart, st));
  ETD_TRY(st_ew(h, dec ? ST_EW_DEC : ST_EW_ENC, norm, x_dev, nullptr, nullptr, y_dev, P * C, U, st));
  if (dy_dev) ETD_TRY(st_norm_bwd(h, norm, x_dev, dy_dev, nullptr, dx_dev, P, B, 0, cpart, st));
  if (stats_dev) {      // [mean | var] of the batch, [I][C] each
    hipLaunchKernelGGL(k_st_d2f, dim3(st_grid((long long)h->I * C)), dim3(256), 0, st, st_S(h, 0, norm), stats_dev, h->I * C);
    hipLaunchKernelGGL(k_st_d2f, dim3(st_grid((long long)h->I * C)), dim3(256), 0, st, st_S(h, 4, norm), stats_dev + (long long)h->I * C, h->I * C);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_septrain_debug_loss(etd_septrain* h, const float* logits_dev, const float* mix_dev, const float* target_dev, int B, double loss_scale,
                                       double* loss_out, float* dlogits_dev, void* stream) {
  if (!h || !logits_dev || !mix_dev || !target_dev || !loss_out || !dlogits_dev) ETD_FAIL(ETD_EINVAL, "septrain_debug_loss: null argument");
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_debug_loss"));
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(st_upload(h));
  ETD_TRY(h->ws.reserve(p.total_bytes, st));
  return st_loss(h, logits_dev, mix_dev, target_dev, B, loss_scale, (float*)h->ws.p + p.lpart, p.loss_blocks, dlogits_dev, loss_out, st);
}

extern "C" int etd_septrain_debug_dropout(etd_septrain* h, int j, const float* y_dev, int B, long long numel, long long call, float* out_dev, void* stream) {
  if (!h || !y_dev || !out_dev) ETD_FAIL(ETD_EINVAL, "septrain_debug_dropout: null argument");
  if (j < 1 || j > ST_DROP_LEVELS) ETD_FAIL(ETD_EINVAL, "septrain_debug_dropout: level j = %d outside 1 .. %d", j, ST_DROP_LEVELS);
  if (call < 0) ETD_FAIL(ETD_EINVAL, "septrain_debug_dropout: call = %lld is negative", call);
  StPlan p;
  ETD_TRY(st_check_batch(h, B, &p, "septrain_debug_dropout"));
  const long long full = (long long)B * h->I * h->net.szD[j];
  if (numel < 0 || numel > full) ETD_FAIL(ETD_EINVAL, "septrain_debug_dropout: numel = %lld outside 0 .. %lld", numel, full);
  ETD_TRY(st_dropout(h, j, call, y_dev, out_dev, numel ? numel : full, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
