// Source separator on the GPU: a song's audio [channels][N] -> its stems [instr][channels][N], the input of etd_stemfeat_run (DESIGN.md 4m is the contract,
// tests/separator_np.py restates it).  Modelled on Spleeter 2.x's 5stems model (spleeter/model/functions/unet.py, spleeter/separator.py): STFT with n_fft zeros on
// both ends, one six-level U-Net per instrument on the magnitudes below bin F in segments of T frames, a softmax over the instruments, ratio masks, inverse STFT.
//
//   k_sep_stft       one workgroup per (channel, frame): window -> the real FFT of lds_rfft.h -> X [c][t][k] and |X| in the U-Net's [t][k][c] layout
//   k_sep_conv_mfma  every convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = output positions, N = output channels, K = taps x input channels gathered
//                    from the NHWC activations (no im2col buffer); bias, ELU and the batch-norm affine in the epilogue.  A transposed convolution is four such
//                    launches, one per output parity, each with the 2 or 3 kernel taps per axis that reach it: no lane multiplies by a structural zero.
//   k_sep_conv_valu  the same launch descriptor, one output element per thread: layers with K < 64 (the first convolution of mono or stereo audio), Cout = 1 and the head
//                    Both are the trainer's convolutions too (separator_train.hip, through sep_launch with the PLAIN epilogue): separator.h holds the descriptor,
//                    the tile step and the layers' geometry.
//   k_sep_mask       softmax over the instruments, ratio mask, zero extension and the product with X in one pass
//   (k_mwf_*)        with etd_sep_set_mwf: passes of multichannel Wiener filtering in place on the masked spectra (separator_mwf.hip)
//   k_sep_istft      one workgroup per (stem, channel, frame): inverse split pass -> the same Stockham stages on conjugated data -> windowed frame
//   k_sep_ola        gather overlap-add: every output sample sums its at most four frames in ascending frame order
//
// Arithmetic: fp32 operands and accumulation.  No atomics; every sum runs in an order fixed by the layer's shape, and a unit (song, segment, instrument) never
// reads another unit's data, so a song's stems are bit-identical alone, in any batch and under any workspace budget.
#include "separator.h"
#include "prof.h"

#include <cmath>
#include <string>

#include "etude_hip_debug.h"

namespace {

// ================================================================================================ STFT
struct SepStftArgs {
  const float* wav; long long N, Tf; int C, n_fft, lgM, hop;
  const float* window; const float2* twM; const float2* twS;
  float2* X; int bins;               // X [c][t][bins], bins <= n_fft / 2 + 1
  float* mag; int F;                 // [t][F][C] or null
};

// the Stockham stages of lds_rfft.h on (sr, si); returns with the result in (sr, si) (the pointers are swapped as the passes go)
__device__ __forceinline__ void sep_fft_stages(float*& sr, float*& si, float*& dr, float*& di, const float2* twM, int M, int lgM, int tid) {
  int Ns = 1, lgNs = 0;
  if (lgM & 1) {
    for (int j = tid; j < (M >> 1); j += SEP_THREADS) rfft::radix2(sr, si, dr, di, M, j);
    __syncthreads();
    float* q = sr; sr = dr; dr = q; q = si; si = di; di = q;
    Ns = 2; lgNs = 1;
  }
  for (; Ns < M; Ns <<= 2, lgNs += 2) {
    for (int j = tid; j < (M >> 2); j += SEP_THREADS) rfft::radix4(sr, si, dr, di, rfft::TwGlobal{twM}, M, Ns, M >> (lgNs + 2), j);
    __syncthreads();
    float* q = sr; sr = dr; dr = q; q = si; si = di; di = q;
  }
}

__global__ __launch_bounds__(SEP_THREADS) void k_sep_stft(const SepStftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int M = a.n_fft >> 1, PM = RFFT_PM(M), tid = threadIdx.x;
  float *sr = sm, *si = sm + PM, *dr = sm + 2 * PM, *di = sm + 3 * PM;
  const long long b = blockIdx.x;
  const int c = (int)(b / a.Tf);
  const long long t = b - (long long)c * a.Tf;
  const float* wav = a.wav + (long long)c * a.N;
  for (int i = tid; i < a.n_fft; i += SEP_THREADS) {
    const long long idx = t * a.hop - a.n_fft + i;     // n_fft zeros in front of the signal
    float v = 0.f;
    if (idx >= 0 && idx < a.N) v = wav[idx] * a.window[i];
    ((i & 1) ? si : sr)[RFFT_PAD(i >> 1)] = v;
  }
  __syncthreads();
  sep_fft_stages(sr, si, dr, di, a.twM, M, a.lgM, tid);
  float2* X = a.X + ((long long)c * a.Tf + t) * a.bins;
  for (int k = tid; k < a.bins; k += SEP_THREADS) {
    float xr, xi;
    rfft::split_bin(sr, si, a.twS, M, k, xr, xi);
    X[k] = make_float2(xr, xi);
    if (a.mag && k < a.F) a.mag[(t * a.F + k) * a.C + c] = sqrtf(xr * xr + xi * xi);
  }
}

// ================================================================================================ the convolutions
__device__ __forceinline__ float sep_elu(float x) { return x > 0.f ? x : expm1f(x); }

// element ci of the concatenated channels at input pixel (it, jf) of a unit, 0 outside the image
__device__ __forceinline__ float sep_gather(const SepLaunch& a, const float* x0, const float* x1, int it, int jf, int ci) {
  if (it < 0 || it >= a.Hin || jf < 0 || jf >= a.Win) return 0.f;
  const int p = it * a.Win + jf;
  return ci < a.C0 ? x0[p * a.C0 + ci] : x1[p * a.C1 + (ci - a.C0)];
}

// the epilogue EPI (= a.epi: the launch picks the instantiation) of one output element: v = the sum, at GEMM position (jt, jf), output channel col
template <int EPI> __device__ __forceinline__ void sep_store(const SepLaunch& a, int u, int inst, int jt, int jf, int col, float v) {
  if (EPI == SEP_EPI_PLAIN) {
    if (a.bias) v += a.bias[inst * a.N + col];
    const long long p = (long long)(a.oS * jt + a.opt) * a.Wout + (a.oS * jf + a.opf);
    if (col < a.N0) a.pre[(long long)u * a.out_us + p * a.N0 + col] = v;
    else a.out1[(long long)u * a.out1_us + p * (a.N - a.N0) + (col - a.N0)] = v;
    return;
  }
  const long long o = (long long)u * a.out_us + ((long long)(a.oS * jt + a.opt) * a.Wout + (a.oS * jf + a.opf)) * a.N + col;
  v += a.bias[inst * a.N + col];
  if (EPI == SEP_EPI_HEAD) { a.pre[o] = v; return; }
  const float bn_a = a.bn_a[inst * a.N + col], bn_s = a.bn_s[inst * a.N + col];
  if (EPI == SEP_EPI_CONV) {
    if (a.pre) a.pre[o] = v;
    if (a.act) a.act[o] = sep_elu(fmaf(bn_a, v, bn_s));
  } else {
    a.act[o] = fmaf(bn_a, sep_elu(v), bn_s);
  }
}

// grid (M tiles, N tiles, units).  The K sum of an output element runs in the order of separator.h's tile step.
template <int EPI> __global__ __launch_bounds__(SEP_THREADS) void k_sep_conv_mfma(const SepLaunch a) {
  __shared__ float As[SEP_BK][SEP_LD], Bs[SEP_BK][SEP_LD];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int m0 = blockIdx.x * SEP_BM, n0 = blockIdx.y * SEP_BN, u = blockIdx.z;
  const int wr = w >> 1, wc = w & 1, half = l >> 5, l31 = l & 31;
  const int inst = (a.u0 + u) % a.I;
  const int Cin = a.C0 + a.C1, K = a.nt * a.nf * Cin, Mpos = a.Hj * a.Wj;
  const float* x0 = a.x0 + (long long)((a.x0_u0 + u) / a.x0_div) * a.x0_us;
  const float* x1 = a.C1 ? a.x1 + (long long)u * a.x1_us : nullptr;
  const float* W = a.W + (long long)inst * a.w_is;
  // this thread's 8 rows of the A tile (k = t & 31 is its column): the input pixel of tap (0, 0), or far outside for a row past the last position
  int rt[8], rf[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int pos = m0 + (t >> 5) + 8 * r;
    if (pos < Mpos) {
      const int jt = pos / a.Wj, jf = pos - jt * a.Wj;
      rt[r] = a.S * jt + a.o0t; rf[r] = a.S * jf + a.o0f;
    } else {
      rt[r] = -(1 << 28); rf[r] = 0;
    }
  }
  float ra[8], rb[8];
  f32x16 tot[4];
  sep_tile_zero(tot);
#define SEP_LOAD(k0)                                                                                        \
  {                                                                                                         \
    const int kg = (k0) + (t & 31);                                                                         \
    const int tap = kg / Cin, ci = kg - tap * Cin, ta = tap / a.nf, tb = tap - ta * a.nf;                   \
    _Pragma("unroll") for (int r = 0; r < 8; ++r)                                                           \
      ra[r] = kg < K ? sep_gather(a, x0, x1, rt[r] + a.d * ta, rf[r] + a.d * tb, ci) : 0.f;                 \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                         \
      const int kb = (k0) + (t >> 6) + 4 * r, nb = n0 + (t & 63);                                           \
      rb[r] = (kb < K && nb < a.N) ? W[(long long)kb * a.N + nb] : 0.f;                                     \
    }                                                                                                       \
  }
  SEP_LOAD(0)
  int step = 0;
  for (int k0 = 0; k0 < K; k0 += SEP_BK, ++step) {
    __syncthreads();                                   // the previous tile has been read
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      As[t & 31][(t >> 5) + 8 * r] = ra[r];
      Bs[(t >> 6) + 4 * r][t & 63] = rb[r];
    }
    __syncthreads();
    if (k0 + SEP_BK < K) SEP_LOAD(k0 + SEP_BK)         // the next tile's loads fly while this one is multiplied
    sep_tile_step(As, Bs, wr * 32 + l31, wc * 32 + l31, half, step, tot);
  }
#undef SEP_LOAD
  const int col = n0 + wc * 32 + l31;
  if (col >= a.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int pos = m0 + wr * 32 + acc_row(r, half);
    if (pos >= Mpos) continue;
    const int jt = pos / a.Wj, jf = pos - jt * a.Wj;
    sep_store<EPI>(a, u, inst, jt, jf, col, sep_tile_total(tot, r));
  }
}

// one output element per thread, channel fastest: per tap one fmaf chain over the input channels, the taps' sums added in tap order
template <int EPI> __global__ __launch_bounds__(SEP_THREADS) void k_sep_conv_valu(const SepLaunch a, long long total) {
  const long long e = (long long)blockIdx.x * SEP_THREADS + threadIdx.x;
  if (e >= total) return;
  const int col = (int)(e % a.N);
  const long long q = e / a.N;
  const int Mpos = a.Hj * a.Wj;
  const int pos = (int)(q % Mpos), u = (int)(q / Mpos);
  const int jt = pos / a.Wj, jf = pos - jt * a.Wj;
  const int inst = (a.u0 + u) % a.I, Cin = a.C0 + a.C1;
  const float* x0 = a.x0 + (long long)((a.x0_u0 + u) / a.x0_div) * a.x0_us;
  const float* x1 = a.C1 ? a.x1 + (long long)u * a.x1_us : nullptr;
  const float* W = a.W + (long long)inst * a.w_is + col;
  float sum = 0.f;
  for (int ta = 0; ta < a.nt; ++ta) {
    const int it = a.S * jt + a.o0t + a.d * ta;
    if (it < 0 || it >= a.Hin) continue;               // (a tap outside the image adds exact zeros)
    for (int tb = 0; tb < a.nf; ++tb) {
      const int jx = a.S * jf + a.o0f + a.d * tb;
      if (jx < 0 || jx >= a.Win) continue;
      const int p = it * a.Win + jx;
      const float* wk = W + (long long)(ta * a.nf + tb) * Cin * a.N;
      float acc = 0.f;
      for (int ci = 0; ci < a.C0; ++ci) acc = fmaf(x0[p * a.C0 + ci], wk[(long long)ci * a.N], acc);
      for (int ci = 0; ci < a.C1; ++ci) acc = fmaf(x1[p * a.C1 + ci], wk[(long long)(a.C0 + ci) * a.N], acc);
      sum += acc;
    }
  }
  sep_store<EPI>(a, u, inst, jt, jf, col, sum);
}

// ================================================================================================ masks
struct SepMaskArgs {
  const float* logits;               // [seg][I][T][F][C]
  const float* mag;                  // [seg * T][F][C]
  const float2* X;                   // [C][Tf][F]
  float2* Y;                         // [I][C][Tf][F]
  long long Tf; int T, F, C, I, p; float eps;
};

__global__ __launch_bounds__(SEP_THREADS) void k_sep_mask(const SepMaskArgs a) {
  const long long e = (long long)blockIdx.x * SEP_THREADS + threadIdx.x;
  if (e >= a.Tf * a.F) return;
  const long long t = e / a.F;
  const int k = (int)(e - t * a.F);
  const long long seg = t / a.T;
  const int tl = (int)(t - seg * a.T);
  const long long plane = (long long)a.T * a.F * a.C;
  const float eps_i = a.eps / (float)a.I;
  for (int c = 0; c < a.C; ++c) {
    const long long in_unit = ((long long)tl * a.F + k) * a.C + c;
    const float* lg = a.logits + seg * a.I * plane + in_unit;
    float v[ETD_SEP_MAX_INSTR];
    float mx = lg[0];
    for (int i = 1; i < a.I; ++i) mx = fmaxf(mx, lg[i * plane]);
    float den = 0.f;
    for (int i = 0; i < a.I; ++i) { v[i] = expf(lg[i * plane] - mx); den += v[i]; }
    const float m = a.mag[(t * a.F + k) * a.C + c];
    float tot = 0.f;
    for (int i = 0; i < a.I; ++i) {
      const float est = (v[i] / den) * m;
      float pw = est;
      for (int j = 1; j < a.p; ++j) pw *= est;
      v[i] = pw; tot += pw;
    }
    tot += a.eps;
    const float2 x = a.X[((long long)c * a.Tf + t) * a.F + k];
    for (int i = 0; i < a.I; ++i) {
      const float mk = (v[i] + eps_i) / tot;
      a.Y[(((long long)i * a.C + c) * a.Tf + t) * a.F + k] = make_float2(mk * x.x, mk * x.y);
    }
  }
}

// ================================================================================================ inverse STFT
struct SepIstftArgs {
  const float2* Y;                   // [rows][Tf][F], rows = stems x channels
  long long Tf; int F, n_fft, lgM;
  const float* window; const float2* twM; const float2* twS;
  float* frames;                     // [rows][Tf][n_fft]
};

__global__ __launch_bounds__(SEP_THREADS) void k_sep_istft(const SepIstftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int M = a.n_fft >> 1, PM = RFFT_PM(M), tid = threadIdx.x;
  float *sr = sm, *si = sm + PM, *dr = sm + 2 * PM, *di = sm + 3 * PM;
  const long long b = blockIdx.x;                      // row * Tf + t
  const float2* Y = a.Y + b * a.F;
  const float2 zero = make_float2(0.f, 0.f);
  for (int k = tid; k < M; k += SEP_THREADS) {
    const int kb = M - k;                              // (k = 0: the Nyquist bin)
    float2 ya = k < a.F ? Y[k] : zero, yb = kb < a.F ? Y[kb] : zero;
    if (k == 0) { ya.y = 0.f; yb.y = 0.f; }            // an inverse real FFT reads no imaginary part of the DC and Nyquist bins
    float zr, zi;
    rfft::isplit_conj(ya, yb, a.twS[k], zr, zi);
    sr[RFFT_PAD(k)] = zr; si[RFFT_PAD(k)] = zi;
  }
  __syncthreads();
  sep_fft_stages(sr, si, dr, di, a.twM, M, a.lgM, tid);
  const float inv = 1.f / (float)M;                    // (a power of two: exact)
  float* out = a.frames + b * a.n_fft;
  for (int i = tid; i < a.n_fft; i += SEP_THREADS) {
    const int j = RFFT_PAD(i >> 1);
    const float v = (i & 1) ? -si[j] : sr[j];
    out[i] = (v * inv) * a.window[i];
  }
}

// out [rows][N]: sample n lies at padded position n + n_fft of frames t with t hop <= n + n_fft < t hop + n_fft
__global__ __launch_bounds__(SEP_THREADS) void k_sep_ola(const float* __restrict__ frames, long long Tf, int n_fft, int hop, long long N, long long rows, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * SEP_THREADS + threadIdx.x;
  if (e >= rows * N) return;
  const long long row = e / N, n = e - row * N;
  const long long p = n + n_fft;
  long long t1 = p / hop;
  if (t1 > Tf - 1) t1 = Tf - 1;
  long long t0 = (p - n_fft + hop) / hop;              // ceil((p - n_fft + 1) / hop) for p >= n_fft
  if (t0 < 0) t0 = 0;
  const float* f = frames + row * Tf * n_fft;
  float acc = 0.f;
  for (long long t = t0; t <= t1; ++t) acc += f[t * n_fft + (p - t * hop)];
  out[e] = acc * (2.f / 3.f);
}

}  // namespace

template <int EPI> static int sep_launch_kernel(const SepLaunch& a, int n_units, bool valu, const char* name, hipStream_t st) {
  const long long Mpos = (long long)a.Hj * a.Wj;
  if (valu) {
    const long long total = (long long)n_units * Mpos * a.N, blocks = (total + SEP_THREADS - 1) / SEP_THREADS;
    if (blocks > 0x7fffffffLL)
      ETD_FAIL(ETD_EINVAL, "separator: %s needs %lld workgroups (> 2^31 - 1); lower the workspace budget", name ? name : "a training convolution", blocks);
    hipLaunchKernelGGL(k_sep_conv_valu<EPI>, dim3((unsigned)blocks), dim3(SEP_THREADS), 0, st, a, total);
  } else {
    const dim3 grid((unsigned)((Mpos + SEP_BM - 1) / SEP_BM), (unsigned)((a.N + SEP_BN - 1) / SEP_BN), (unsigned)n_units);
    hipLaunchKernelGGL(k_sep_conv_mfma<EPI>, grid, dim3(SEP_THREADS), 0, st, a);
  }
  return ETD_OK;
}

static int sep_launch_epi(const SepLaunch& a, int n_units, bool valu, const char* name, hipStream_t st) {
  switch (a.epi) {
    case SEP_EPI_CONV: return sep_launch_kernel<SEP_EPI_CONV>(a, n_units, valu, name, st);
    case SEP_EPI_DECONV: return sep_launch_kernel<SEP_EPI_DECONV>(a, n_units, valu, name, st);
    case SEP_EPI_HEAD: return sep_launch_kernel<SEP_EPI_HEAD>(a, n_units, valu, name, st);
    case SEP_EPI_PLAIN: return sep_launch_kernel<SEP_EPI_PLAIN>(a, n_units, valu, name, st);
  }
  ETD_FAIL(ETD_EINVAL, "separator: epilogue %d is not one of the four", a.epi);
}

int sep_launch(const SepLaunch& a, int n_units, bool force_valu, const char* name, hipStream_t st) {
  const int K = a.nt * a.nf * (a.C0 + a.C1);
  const bool valu = K < SEP_MFMA_MIN_K || a.N == 1 || a.epi == SEP_EPI_HEAD || force_valu;
  if (!name) return sep_launch_epi(a, n_units, valu, name, st);
  ProfScope ps(name, st, 2.0 * (double)n_units * (double)a.Hj * a.Wj * K * a.N, 0);
  return sep_launch_epi(a, n_units, valu, name, st);
}

struct etd_sep {
  etd_sep_cfg cfg;
  int M = 0, lgM = 0, L = ETD_SEP_LEVELS;
  SepNet net;
  // a unit's activations, in floats: conv_l before the norm (the skips and the decoder's first input) and the two buffers every other tensor alternates between
  long long pre_off[ETD_SEP_LEVELS + 1], a_off[2], unit_floats = 0;
  double seg_flops = 0;
  // host tables (create needs no GPU); uploaded by the first run
  std::vector<float> window;
  std::vector<float2> twM, twS;
  std::vector<float> w_conv[ETD_SEP_LEVELS], b_conv[ETD_SEP_LEVELS], w_dec[ETD_SEP_LEVELS][4], b_dec[ETD_SEP_LEVELS], bn_a[2 * ETD_SEP_LEVELS], bn_s[2 * ETD_SEP_LEVELS];
  std::vector<float> w_head, b_head;
  DevPool pool;
  float* d_window = nullptr; float2 *d_twM = nullptr, *d_twS = nullptr;
  float *d_w_conv[ETD_SEP_LEVELS], *d_b_conv[ETD_SEP_LEVELS], *d_w_dec[ETD_SEP_LEVELS][4], *d_b_dec[ETD_SEP_LEVELS], *d_bn_a[2 * ETD_SEP_LEVELS], *d_bn_s[2 * ETD_SEP_LEVELS];
  float *d_w_head = nullptr, *d_b_head = nullptr;
  Workspace ws;
  int mwf = 0;                       // Wiener iterations between the mask pass and the inverse STFT (etd_sep_set_mwf; 0 = none)
};

namespace {

int sep_upload(etd_sep* h) {
  DevPool& P = h->pool;
  return P.upload_once([&]() -> int {
    ETD_TRY(P.upload(&h->d_window, h->window.data(), h->window.size()));
    ETD_TRY(P.upload(&h->d_twM, h->twM.data(), h->twM.size()));
    ETD_TRY(P.upload(&h->d_twS, h->twS.data(), h->twS.size()));
    for (int l = 0; l < ETD_SEP_LEVELS; ++l) {
      ETD_TRY(P.upload(&h->d_w_conv[l], h->w_conv[l].data(), h->w_conv[l].size()));
      ETD_TRY(P.upload(&h->d_b_conv[l], h->b_conv[l].data(), h->b_conv[l].size()));
      for (int p = 0; p < 4; ++p) ETD_TRY(P.upload(&h->d_w_dec[l][p], h->w_dec[l][p].data(), h->w_dec[l][p].size()));
      ETD_TRY(P.upload(&h->d_b_dec[l], h->b_dec[l].data(), h->b_dec[l].size()));
    }
    for (int n = 0; n < 2 * ETD_SEP_LEVELS; ++n) {
      ETD_TRY(P.upload(&h->d_bn_a[n], h->bn_a[n].data(), h->bn_a[n].size()));
      ETD_TRY(P.upload(&h->d_bn_s[n], h->bn_s[n].data(), h->bn_s[n].size()));
    }
    ETD_TRY(P.upload(&h->d_w_head, h->w_head.data(), h->w_head.size()));
    return P.upload(&h->d_b_head, h->b_head.data(), h->b_head.size());
  });
}

// the test hooks run every unit of a launch with one instrument's weights
void sep_fix_instrument(SepLaunch& a, int fixed) {
  if (fixed < 0) return;
  a.W += (long long)fixed * a.w_is; a.bias += (long long)fixed * a.N;
  if (a.bn_a) { a.bn_a += (long long)fixed * a.N; a.bn_s += (long long)fixed * a.N; }
  a.u0 = 0; a.I = 1;
}

// encoder layer l = 1 .. 6 over n units: x0 (stride x0_us; shared by the I instruments of a segment when x0_div = I) -> pre / act (stride out_us)
int sep_encoder(etd_sep* h, int l, const float* x0, long long x0_us, int x0_u0, int x0_div, float* pre, float* act, long long out_us, int u0, int n, hipStream_t st,
                int fixed = -1) {
  SepLaunch a{};
  sep_geom_encoder(h->net, l, &a);
  a.x0 = x0; a.x0_us = x0_us; a.x0_u0 = x0_u0; a.x0_div = x0_div;
  a.W = h->d_w_conv[l - 1]; a.w_is = 25LL * a.C0 * a.N; a.bias = h->d_b_conv[l - 1]; a.bn_a = h->d_bn_a[l - 1]; a.bn_s = h->d_bn_s[l - 1];
  a.pre = pre; a.act = act; a.out_us = out_us; a.epi = SEP_EPI_CONV;
  a.u0 = u0; a.I = h->cfg.n_instr;
  sep_fix_instrument(a, fixed);
  return sep_launch(a, n, false, "k_sep_conv", st);
}

// decoder layer j = 1 .. 6: [skip | up] -> act, four launches by output parity
int sep_decoder(etd_sep* h, int j, const float* skip, long long skip_us, const float* up, long long up_us, float* act, long long out_us, int u0, int n, hipStream_t st,
                int fixed = -1) {
  for (int par = 0; par < 4; ++par) {
    const int pt = par >> 1, pf = par & 1;
    SepLaunch a{};
    sep_geom_deconv(h->net, j, pt, pf, &a);
    a.x0 = skip; a.x0_us = skip_us; a.x0_div = 1; a.x1 = up; a.x1_us = up_us;
    a.W = h->d_w_dec[j - 1][par]; a.w_is = (long long)a.nt * a.nf * (a.C0 + a.C1) * a.N;
    a.bias = h->d_b_dec[j - 1]; a.bn_a = h->d_bn_a[ETD_SEP_LEVELS + j - 1]; a.bn_s = h->d_bn_s[ETD_SEP_LEVELS + j - 1];
    a.act = act; a.out_us = out_us; a.epi = SEP_EPI_DECONV;
    a.u0 = u0; a.I = h->cfg.n_instr;
    sep_fix_instrument(a, fixed);
    ETD_TRY(sep_launch(a, n, false, "k_sep_deconv", st));
  }
  return ETD_OK;
}

int sep_head(etd_sep* h, const float* x, long long x_us, float* logits, long long out_us, int u0, int n, hipStream_t st, int fixed = -1) {
  SepLaunch a{};
  sep_geom_head(h->net, &a);
  a.x0 = x; a.x0_us = x_us; a.x0_div = 1;
  a.W = h->d_w_head; a.w_is = 16LL * a.N; a.bias = h->d_b_head;
  a.pre = logits; a.out_us = out_us; a.epi = SEP_EPI_HEAD;
  a.u0 = u0; a.I = h->cfg.n_instr;
  sep_fix_instrument(a, fixed);
  return sep_launch(a, n, false, "k_sep_head", st);
}

// the U-Nets of units u0 .. u0 + n - 1 (unit = segment * I + instrument): mag [segments][T][F][C] -> logits + u0 * T F C, activations in `work`
int sep_unet(etd_sep* h, const float* mag, float* logits, float* work, int u0, int n, hipStream_t st) {
  const long long us = h->unit_floats, plane = (long long)h->cfg.T * h->cfg.F * h->cfg.n_channels;
  float* A[2] = {work + h->a_off[0], work + h->a_off[1]};
  ETD_TRY(sep_encoder(h, 1, mag, plane, u0, h->cfg.n_instr, work + h->pre_off[1], A[0], us, u0, n, st));
  for (int l = 2; l <= ETD_SEP_LEVELS; ++l)
    ETD_TRY(sep_encoder(h, l, A[l & 1], us, 0, 1, work + h->pre_off[l], l < ETD_SEP_LEVELS ? A[(l - 1) & 1] : nullptr, us, u0, n, st));
  for (int j = 1; j <= ETD_SEP_LEVELS; ++j)
    ETD_TRY(sep_decoder(h, j, work + h->pre_off[7 - j], us, j > 1 ? A[j & 1] : nullptr, us, A[(j - 1) & 1], us, u0, n, st));
  return sep_head(h, A[1], us, logits + (long long)u0 * plane, plane, u0, n, st);
}

int sep_stft(etd_sep* h, const float* wav, long long N, long long Tf, float2* X, int bins, float* mag, hipStream_t st) {
  if ((long long)h->cfg.n_channels * Tf > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator: more than 2^31 - 1 frames in one song");
  SepStftArgs a;
  a.wav = wav; a.N = N; a.Tf = Tf; a.C = h->cfg.n_channels; a.n_fft = h->cfg.n_fft; a.lgM = h->lgM; a.hop = h->cfg.hop;
  a.window = h->d_window; a.twM = h->d_twM; a.twS = h->d_twS; a.X = X; a.bins = bins; a.mag = mag; a.F = h->cfg.F;
  const double fr = (double)a.C * Tf;
  ProfScope ps("k_sep_stft", st, fr * (5.0 * h->M * h->lgM + 12.0 * h->M), fr * ((double)h->cfg.hop * 4 + bins * 8.0));
  hipLaunchKernelGGL(k_sep_stft, dim3((unsigned)(a.C * Tf)), dim3(SEP_THREADS), (size_t)SEP_FFT_LDS_FLOATS(h->M) * sizeof(float), st, a);
  return ETD_OK;
}

int sep_mask(etd_sep* h, const float* logits, const float* mag, const float2* X, long long Tf, float2* Y, hipStream_t st) {
  SepMaskArgs a;
  a.logits = logits; a.mag = mag; a.X = X; a.Y = Y; a.Tf = Tf; a.T = h->cfg.T; a.F = h->cfg.F; a.C = h->cfg.n_channels; a.I = h->cfg.n_instr;
  a.p = h->cfg.separation_exponent; a.eps = h->cfg.mask_eps;
  const long long blocks = (Tf * a.F + SEP_THREADS - 1) / SEP_THREADS;
  if (blocks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator: more than 2^31 - 1 workgroups in the mask pass");
  ProfScope ps("k_sep_mask", st, 0, (double)Tf * a.F * a.C * (a.I * 12.0 + 12.0));
  hipLaunchKernelGGL(k_sep_mask, dim3((unsigned)blocks), dim3(SEP_THREADS), 0, st, a);
  return ETD_OK;
}

// rows = stems x channels of one song: Y [rows][Tf][F] -> out [rows][N] through frames [rows][Tf][n_fft]
int sep_istft(etd_sep* h, const float2* Y, long long Tf, long long N, long long rows, float* frames, float* out, hipStream_t st) {
  if (rows * Tf > 0x7fffffffLL || (rows * N + SEP_THREADS - 1) / SEP_THREADS > 0x7fffffffLL)
    ETD_FAIL(ETD_EINVAL, "separator: more than 2^31 - 1 workgroups in the inverse STFT");
  SepIstftArgs a;
  a.Y = Y; a.Tf = Tf; a.F = h->cfg.F; a.n_fft = h->cfg.n_fft; a.lgM = h->lgM; a.window = h->d_window; a.twM = h->d_twM; a.twS = h->d_twS; a.frames = frames;
  const double fr = (double)rows * Tf;
  {
    ProfScope ps("k_sep_istft", st, fr * (5.0 * h->M * h->lgM + 12.0 * h->M), fr * (a.F * 8.0 + a.n_fft * 4.0));
    hipLaunchKernelGGL(k_sep_istft, dim3((unsigned)(rows * Tf)), dim3(SEP_THREADS), (size_t)SEP_FFT_LDS_FLOATS(h->M) * sizeof(float), st, a);
  }
  {
    ProfScope ps("k_sep_ola", st, 0, (double)rows * N * 20.0);
    hipLaunchKernelGGL(k_sep_ola, dim3((unsigned)((rows * N + SEP_THREADS - 1) / SEP_THREADS)), dim3(SEP_THREADS), 0, st, frames, Tf, a.n_fft, h->cfg.hop, N, rows, out);
  }
  return ETD_OK;
}

struct SepPlan {
  std::vector<long long> Tf, seg0;   // per song of the group: frames, first segment of the group
  long long segs = 0;                // segments of the group
  long long nb = 0;                  // units per sub-batch
  long long work_budget = 0;
  long long off_X = 0, off_mag = 0, off_logits = 0, off_Y = 0, off_work = 0, total = 0;      // bytes
  std::vector<long long> x_off, y_off;                                                      // per song, in float2
};

long long sep_budget(const etd_sep* h) { return h->cfg.workspace_bytes > 0 ? h->cfg.workspace_bytes : (4LL << 30); }

// bytes a song holds from its STFT to its inverse STFT: X and |X| below bin F, the mask logits of its segments, the masked spectra
long long sep_song_bytes(const etd_sep* h, long long N) {
  const etd_sep_cfg& c = h->cfg;
  const long long Tf = 1 + (N + c.n_fft) / c.hop, segs = (Tf + c.T - 1) / c.T;
  return (long long)c.n_channels * Tf * c.F * 8 * (1 + c.n_instr) + segs * c.T * c.F * c.n_channels * 4 * (1 + c.n_instr);
}

// stems of a song whose frames `budget` bytes hold at once (at least one)
long long sep_stems_per_pass(const etd_sep* h, long long Tf, long long budget) {
  const long long per = (long long)h->cfg.n_channels * Tf * h->cfg.n_fft * 4;
  long long ni = budget / per;
  if (ni < 1) ni = 1;
  if (ni > h->cfg.n_instr) ni = h->cfg.n_instr;
  return ni;
}

// A call runs as groups of consecutive songs, one after the other in the same workspace.  A group takes songs while what they hold (sep_song_bytes) stays within
// half the budget -- one song is the floor --, and the rest of the budget (one unit / one stem at the least) goes to the U-Net activations and the inverse STFT's
// frames.  Nothing a song computes depends on its group.
int sep_groups(const etd_sep* h, int n_songs, const int64_t* N_host, std::vector<int>* first) {
  if (!h || !N_host || n_songs < 1) ETD_FAIL(ETD_EINVAL, "separator: null argument or n_songs < 1");
  first->clear();
  long long held = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long N = N_host[s];
    if (N < 1) ETD_FAIL(ETD_EINVAL, "separator: song %d has N = %lld (need >= 1)", s, N);
    if (N > (1LL << 32)) ETD_FAIL(ETD_EINVAL, "separator: song %d has N = %lld (> 2^32)", s, N);
    const long long b = sep_song_bytes(h, N);
    if (s == 0 || held + b > sep_budget(h) / 2) { first->push_back(s); held = 0; }
    held += b;
  }
  first->push_back(n_songs);
  return ETD_OK;
}

// the plan of one group (N_host: its first song)
int sep_plan(const etd_sep* h, int n_songs, const int64_t* N_host, SepPlan* p) {
  const etd_sep_cfg& c = h->cfg;
  p->Tf.resize(n_songs); p->seg0.resize(n_songs); p->x_off.resize(n_songs); p->y_off.resize(n_songs);
  long long segs = 0, xf = 0, yf = 0, held = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long Tf = 1 + (N_host[s] + c.n_fft) / c.hop;
    p->Tf[s] = Tf; p->seg0[s] = segs; p->x_off[s] = xf; p->y_off[s] = yf;
    segs += (Tf + c.T - 1) / c.T;
    xf += (long long)c.n_channels * Tf * c.F;
    yf += (long long)c.n_instr * c.n_channels * Tf * c.F;
    held += sep_song_bytes(h, N_host[s]);
  }
  if (segs * c.n_instr > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator: more than 2^31 - 1 (segment, instrument) units in one group of songs");
  p->segs = segs;
  p->work_budget = sep_budget(h) > held ? sep_budget(h) - held : 0;
  long long work = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long fr = sep_stems_per_pass(h, p->Tf[s], p->work_budget) * c.n_channels * p->Tf[s] * c.n_fft * 4;
    work = fr > work ? fr : work;
  }
  long long nb = p->work_budget / (h->unit_floats * 4);
  if (nb < 1) nb = 1;
  if (nb > segs * c.n_instr) nb = segs * c.n_instr;
  if (nb > 16384) nb = 16384;                          // (gridDim.z)
  p->nb = nb;
  const long long uw = nb * h->unit_floats * 4;
  work = uw > work ? uw : work;
  if (h->mwf > 0)                                      // the Wiener stage borrows the work region: its tables do not depend on the budget, so they raise the floor
    for (int s = 0; s < n_songs; ++s) {
      const long long mw = sep_mwf_scratch_bytes(c.n_instr, c.n_channels, c.F, p->Tf[s]);
      work = mw > work ? mw : work;
    }
  const long long plane = (long long)c.T * c.F * c.n_channels * 4;
  WsCursor ws;
  p->off_X = ws.take(xf * 8);
  p->off_mag = ws.take(segs * plane);
  p->off_logits = ws.take(segs * c.n_instr * plane);
  p->off_Y = ws.take(yf * 8);
  p->off_work = ws.take(work);
  p->total = ws.off;
  return ETD_OK;
}

// every group's plan and the largest workspace among them
int sep_plan_call(const etd_sep* h, int n_songs, const int64_t* N_host, std::vector<int>* first, std::vector<SepPlan>* plans, long long* bytes) {
  ETD_TRY(sep_groups(h, n_songs, N_host, first));
  plans->resize(first->size() - 1);
  *bytes = 0;
  for (size_t g = 0; g + 1 < first->size(); ++g) {
    ETD_TRY(sep_plan(h, (*first)[g + 1] - (*first)[g], N_host + (*first)[g], &(*plans)[g]));
    if ((*plans)[g].total > *bytes) *bytes = (*plans)[g].total;
  }
  return ETD_OK;
}

}  // namespace

extern "C" int etd_sep_create(const etd_sep_cfg* cfg, const char* const* instr_names, const char* const* names, const float* const* host_ptrs, const int64_t* numels,
                              int n, etd_sep** out) {
  if (!cfg || !out || !instr_names || !names || !host_ptrs || !numels || n < 0) ETD_FAIL(ETD_EINVAL, "sep_create: null argument");
  ETD_CHECK_CFG(cfg, etd_sep_cfg, "sep_create");
  const etd_sep_cfg& c = *cfg;
  if (c.n_instr < 1 || c.n_instr > ETD_SEP_MAX_INSTR) ETD_FAIL(ETD_EINVAL, "sep_create: n_instr = %d must be in 1 .. %d", c.n_instr, ETD_SEP_MAX_INSTR);
  if (c.n_channels < 1 || c.n_channels > ETD_SEP_MAX_CHANNELS) ETD_FAIL(ETD_EINVAL, "sep_create: n_channels = %d must be in 1 .. %d", c.n_channels, ETD_SEP_MAX_CHANNELS);
  if (c.n_fft < 1024 || c.n_fft > 4096 || (c.n_fft & (c.n_fft - 1))) ETD_FAIL(ETD_EINVAL, "sep_create: n_fft = %d must be a power of two in 1024 .. 4096", c.n_fft);
  if (c.hop * 4 != c.n_fft) ETD_FAIL(ETD_EINVAL, "sep_create: hop = %d must be n_fft / 4 = %d", c.hop, c.n_fft / 4);
  const int mult = 1 << ETD_SEP_LEVELS;
  if (c.T < mult || c.T % mult || c.F < mult || c.F % mult) ETD_FAIL(ETD_EINVAL, "sep_create: T = %d and F = %d must be positive multiples of %d", c.T, c.F, mult);
  if (c.F > c.n_fft / 2) ETD_FAIL(ETD_EINVAL, "sep_create: F = %d must be <= n_fft / 2 = %d", c.F, c.n_fft / 2);
  // (with n_channels <= 8 a segment's [T][F][C] planes then stay within 2^30 elements: the kernels index a unit's tensors with an int)
  if (c.T > (1 << 16) || c.F > 2048) ETD_FAIL(ETD_EINVAL, "sep_create: T = %d must be <= 65536 and F = %d <= 2048", c.T, c.F);
  for (int l = 0; l < ETD_SEP_LEVELS; ++l)
    if (c.filters[l] < 1 || c.filters[l] > 4096) ETD_FAIL(ETD_EINVAL, "sep_create: filters[%d] = %d must be in 1 .. 4096", l, c.filters[l]);
  if (c.separation_exponent < 1 || c.separation_exponent > 8) ETD_FAIL(ETD_EINVAL, "sep_create: separation_exponent = %d must be in 1 .. 8", c.separation_exponent);
  if (!(c.mask_eps > 0.f) || !std::isfinite(c.mask_eps) || !(c.bn_eps > 0.f) || !std::isfinite(c.bn_eps))
    ETD_FAIL(ETD_EINVAL, "sep_create: mask_eps and bn_eps must be positive and finite");
  if (c.workspace_bytes < 0) ETD_FAIL(ETD_EINVAL, "sep_create: workspace_bytes = %lld is negative", c.workspace_bytes);
  for (int i = 0; i < c.n_instr; ++i)
    if (!instr_names[i] || !instr_names[i][0]) ETD_FAIL(ETD_EINVAL, "sep_create: instrument %d has no name", i);

  etd_sep* h = new etd_sep();
  auto fail = [&](int rc) { delete h; return rc; };
  h->cfg = c;
  h->M = c.n_fft / 2;
  while ((1 << h->lgM) < h->M) ++h->lgM;
  sep_net_init(&h->net, c);
  // the unit's layout; every tensor of a unit must be indexable by an int
  long long o = 0, amax = 0;
  const long long lim = 1LL << 30;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
    const long long sz = h->net.szE[l];
    if (sz > lim) { g_etd_err = "sep_create: an activation of one segment has more than 2^30 elements"; return fail(ETD_EINVAL); }
    h->pre_off[l] = o; o += (sz + 63) & ~63LL;
    if (l < ETD_SEP_LEVELS && sz > amax) amax = sz;
    const long long up = h->net.szD[l];
    if (up > lim) { g_etd_err = "sep_create: an activation of one segment has more than 2^30 elements"; return fail(ETD_EINVAL); }
    if (up > amax) amax = up;
  }
  amax = (amax + 63) & ~63LL;
  h->a_off[0] = o; o += amax;
  h->a_off[1] = o; o += amax;
  h->unit_floats = o;

  h->window.resize(c.n_fft);
  for (int i = 0; i < c.n_fft; ++i) h->window[i] = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * i / c.n_fft));      // periodic Hann
  rfft_twiddles(h->M, h->twM, h->twS);

  const WeightTable wt(names, host_ptrs, numels, n);
  const int I = c.n_instr;
  auto need = [&](const std::string& key, int64_t numel) -> const float* {
    const float* p = wt.get(key, numel);
    if (p && !finite_all(p, (size_t)numel)) { g_etd_err = "weight '" + key + "' holds a non-finite value"; return nullptr; }
    return p;
  };
  double flops = 0;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
    const int Ci = h->net.Cenc[l - 1], Co = h->net.Cenc[l];
    h->w_conv[l - 1].resize((size_t)I * 25 * Ci * Co); h->b_conv[l - 1].resize((size_t)I * Co);
    flops += 2.0 * (c.T >> l) * (c.F >> l) * 25.0 * Ci * Co;
    // decoder j = l
    const int j = l, D0 = h->net.Cenc[7 - j], D1 = j > 1 ? h->net.Cdout[j - 1] : 0, Di = D0 + D1, Do = h->net.Cdout[j];
    for (int par = 0; par < 4; ++par) h->w_dec[j - 1][par].resize((size_t)I * sep_dec_taps(par >> 1) * sep_dec_taps(par & 1) * Di * Do);
    h->b_dec[j - 1].resize((size_t)I * Do);
    flops += 2.0 * (c.T >> (7 - j)) * (c.F >> (7 - j)) * 25.0 * Di * Do;
    h->bn_a[l - 1].resize((size_t)I * Co); h->bn_s[l - 1].resize((size_t)I * Co);
    h->bn_a[ETD_SEP_LEVELS + j - 1].resize((size_t)I * Do); h->bn_s[ETD_SEP_LEVELS + j - 1].resize((size_t)I * Do);
  }
  h->w_head.resize((size_t)I * 16 * c.n_channels); h->b_head.resize((size_t)I * c.n_channels);
  flops += 2.0 * c.T * c.F * 16.0 * c.n_channels;
  h->seg_flops = flops * I;
  for (int i = 0; i < I; ++i) {
    const std::string pre = std::string(instr_names[i]) + ".";
    for (int l = 1; l <= ETD_SEP_LEVELS; ++l) {
      const int Ci = h->net.Cenc[l - 1], Co = h->net.Cenc[l];
      const float* w = need(pre + "conv" + std::to_string(l) + ".weight", 25LL * Ci * Co);
      if (!w) return fail(ETD_EINVAL);
      memcpy(&h->w_conv[l - 1][(size_t)i * 25 * Ci * Co], w, (size_t)25 * Ci * Co * 4);      // [kt][kf][ci][co] is the GEMM's [K][N]
      const float* b = need(pre + "conv" + std::to_string(l) + ".bias", Co);
      if (!b) return fail(ETD_EINVAL);
      memcpy(&h->b_conv[l - 1][(size_t)i * Co], b, (size_t)Co * 4);
      const int j = l, D0 = h->net.Cenc[7 - j], D1 = j > 1 ? h->net.Cdout[j - 1] : 0, Di = D0 + D1, Do = h->net.Cdout[j];
      const float* wd = need(pre + "deconv" + std::to_string(j) + ".weight", 25LL * Do * Di);
      if (!wd) return fail(ETD_EINVAL);
      for (int par = 0; par < 4; ++par) {               // [kt][kf][co][ci] -> per parity [a][b][ci][co]
        const int pt = par >> 1, pf = par & 1, nt = sep_dec_taps(pt), nf = sep_dec_taps(pf);
        float* dst = &h->w_dec[j - 1][par][(size_t)i * nt * nf * Di * Do];
        for (int a = 0; a < nt; ++a)
          for (int b2 = 0; b2 < nf; ++b2) {
            const float* src = wd + ((size_t)sep_dec_tap(pt, a) * 5 + sep_dec_tap(pf, b2)) * Do * Di;
            for (int ci = 0; ci < Di; ++ci)
              for (int co = 0; co < Do; ++co) dst[(((size_t)a * nf + b2) * Di + ci) * Do + co] = src[(size_t)co * Di + ci];
          }
      }
      const float* bd = need(pre + "deconv" + std::to_string(j) + ".bias", Do);
      if (!bd) return fail(ETD_EINVAL);
      memcpy(&h->b_dec[j - 1][(size_t)i * Do], bd, (size_t)Do * 4);
    }
    for (int nn = 1; nn <= 2 * ETD_SEP_LEVELS; ++nn) {   // a = gamma / sqrt(var + eps), s = beta - mean a: fp64, rounded once
      const int Cn = nn <= ETD_SEP_LEVELS ? h->net.Cenc[nn] : h->net.Cdout[nn - ETD_SEP_LEVELS];
      const std::string k = pre + "bn" + std::to_string(nn);
      const float *g = need(k + ".gamma", Cn), *be = g ? need(k + ".beta", Cn) : nullptr, *mu = be ? need(k + ".mean", Cn) : nullptr, *va = mu ? need(k + ".var", Cn) : nullptr;
      if (!va) return fail(ETD_EINVAL);
      for (int ch = 0; ch < Cn; ++ch) {
        if (!((double)va[ch] + (double)c.bn_eps > 0.0)) { g_etd_err = "weight '" + k + ".var' + bn_eps is not positive"; return fail(ETD_EINVAL); }
        const double a = (double)g[ch] / sqrt((double)va[ch] + (double)c.bn_eps);
        h->bn_a[nn - 1][(size_t)i * Cn + ch] = (float)a;
        h->bn_s[nn - 1][(size_t)i * Cn + ch] = (float)((double)be[ch] - (double)mu[ch] * a);
      }
    }
    const float* wh = need(pre + "head.weight", 16LL * c.n_channels);
    if (!wh) return fail(ETD_EINVAL);
    memcpy(&h->w_head[(size_t)i * 16 * c.n_channels], wh, (size_t)16 * c.n_channels * 4);
    const float* bh = need(pre + "head.bias", c.n_channels);
    if (!bh) return fail(ETD_EINVAL);
    memcpy(&h->b_head[(size_t)i * c.n_channels], bh, (size_t)c.n_channels * 4);
  }
  *out = h;
  return ETD_OK;
}

extern "C" void etd_sep_destroy(etd_sep* h) {
  if (!h) return;
  h->pool.release_uploaded();
  h->ws.release();
  delete h;
}

extern "C" long long etd_sep_num_frames(const etd_sep* h, long long N) {
  if (!h || N < 1) { g_etd_err = "sep_num_frames: null handle or N < 1"; return ETD_EINVAL; }
  return 1 + (N + h->cfg.n_fft) / h->cfg.hop;
}

extern "C" long long etd_sep_unit_bytes(const etd_sep* h) {
  if (!h) { g_etd_err = "sep_unit_bytes: null handle"; return ETD_EINVAL; }
  return h->unit_floats * 4;
}

extern "C" double etd_sep_segment_flops(const etd_sep* h) { return h ? h->seg_flops : 0.0; }

extern "C" long long etd_sep_workspace_bytes(const etd_sep* h, int n_songs, const int64_t* N_host) {
  std::vector<int> first; std::vector<SepPlan> plans; long long bytes = 0;
  const int rc = sep_plan_call(h, n_songs, N_host, &first, &plans, &bytes);
  return rc != ETD_OK ? rc : bytes;
}

extern "C" int etd_sep_run(etd_sep* h, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, float* const* out_ptrs, void* stream) {
  if (!h || !wav_ptrs || !out_ptrs) ETD_FAIL(ETD_EINVAL, "sep_run: null argument");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int> first; std::vector<SepPlan> plans; long long bytes = 0;
  ETD_TRY(sep_plan_call(h, n_songs, N_host, &first, &plans, &bytes));
  for (int s = 0; s < n_songs; ++s)
    if (!wav_ptrs[s] || !out_ptrs[s]) ETD_FAIL(ETD_EINVAL, "sep_run: song %d has a null pointer", s);
  ETD_TRY(sep_upload(h));
  ETD_TRY(h->ws.reserve(bytes, st));
  const etd_sep_cfg& c = h->cfg;
  const long long plane = (long long)c.T * c.F * c.n_channels;
  for (size_t g = 0; g < plans.size(); ++g) {            // (the groups follow each other on the stream, in the same workspace)
    const SepPlan& p = plans[g];
    const int s0 = first[g], ng = first[g + 1] - s0;
    float2* X = (float2*)(h->ws.p + p.off_X);
    float* mag = (float*)(h->ws.p + p.off_mag);
    float* logits = (float*)(h->ws.p + p.off_logits);
    float2* Y = (float2*)(h->ws.p + p.off_Y);
    float* work = (float*)(h->ws.p + p.off_work);
    HIP_TRY(hipMemsetAsync(mag, 0, (size_t)(p.segs * plane * 4), st));          // the frames past a song's last are zeros
    for (int s = 0; s < ng; ++s)
      ETD_TRY(sep_stft(h, wav_ptrs[s0 + s], N_host[s0 + s], p.Tf[s], X + p.x_off[s], c.F, mag + p.seg0[s] * plane, st));
    const long long units = p.segs * c.n_instr;
    for (long long u0 = 0; u0 < units; u0 += p.nb)
      ETD_TRY(sep_unet(h, mag, logits, work, (int)u0, (int)(units - u0 < p.nb ? units - u0 : p.nb), st));
    for (int s = 0; s < ng; ++s) {
      const long long N = N_host[s0 + s];
      ETD_TRY(sep_mask(h, logits + p.seg0[s] * c.n_instr * plane, mag + p.seg0[s] * plane, X + p.x_off[s], p.Tf[s], Y + p.y_off[s], st));
      if (h->mwf > 0) ETD_TRY(sep_mwf_run(X + p.x_off[s], Y + p.y_off[s], p.Tf[s], c.n_instr, c.n_channels, c.F, h->mwf, work, st));
      const long long ni = sep_stems_per_pass(h, p.Tf[s], p.work_budget);
      for (long long i0 = 0; i0 < c.n_instr; i0 += ni) {
        const long long n = c.n_instr - i0 < ni ? c.n_instr - i0 : ni;
        ETD_TRY(sep_istft(h, Y + p.y_off[s] + i0 * c.n_channels * p.Tf[s] * c.F, p.Tf[s], N, n * c.n_channels, work, out_ptrs[s0 + s] + i0 * c.n_channels * N, st));
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_magnitudes(etd_sep* h, const float* wav_dev, long long N, float* mag_dev, void* stream) {
  if (!h || !wav_dev || !mag_dev || N < 1) ETD_FAIL(ETD_EINVAL, "sep_magnitudes: null argument or N < 1");
  if (N > (1LL << 32)) ETD_FAIL(ETD_EINVAL, "sep_magnitudes: N = %lld (> 2^32)", N);
  hipStream_t st = (hipStream_t)stream;
  const etd_sep_cfg& c = h->cfg;
  const long long Tf = 1 + (N + c.n_fft) / c.hop, segs = (Tf + c.T - 1) / c.T;
  ETD_TRY(sep_upload(h));
  ETD_TRY(h->ws.reserve(ws_align((long long)c.n_channels * Tf * c.F * 8), st));
  HIP_TRY(hipMemsetAsync(mag_dev, 0, (size_t)(segs * c.T * c.F * c.n_channels * 4), st));      // the frames past the song's last are zeros
  ETD_TRY(sep_stft(h, wav_dev, N, Tf, (float2*)h->ws.p, c.F, mag_dev, st));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_set_mwf(etd_sep* h, int iterations) {
  if (!h) ETD_FAIL(ETD_EINVAL, "sep_set_mwf: null handle");
  if (iterations < 0 || iterations > SEP_MWF_MAX_ITER) ETD_FAIL(ETD_EINVAL, "sep_set_mwf: iterations = %d must be in 0 .. %d", iterations, SEP_MWF_MAX_ITER);
  if (iterations > 0 && h->cfg.n_channels > SEP_MWF_MAX_CHANNELS)
    ETD_FAIL(ETD_EINVAL, "sep_set_mwf: Wiener filtering takes 1 or %d channels, the engine has %d", SEP_MWF_MAX_CHANNELS, h->cfg.n_channels);
  h->mwf = iterations;
  return ETD_OK;
}

extern "C" int etd_sep_get_mwf(const etd_sep* h) {
  if (!h) ETD_FAIL(ETD_EINVAL, "sep_get_mwf: null handle");
  return h->mwf;
}

// ================================================================================================ test hooks
extern "C" int etd_sep_debug_stft(etd_sep* h, const float* wav_dev, long long N, float* X_dev, void* stream) {
  if (!h || !wav_dev || !X_dev || N < 1) ETD_FAIL(ETD_EINVAL, "sep_debug_stft: null argument or N < 1");
  ETD_TRY(sep_upload(h));
  ETD_TRY(sep_stft(h, wav_dev, N, 1 + (N + h->cfg.n_fft) / h->cfg.hop, (float2*)X_dev, h->M + 1, nullptr, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_debug_layer(etd_sep* h, int instr, int kind, int layer, const float* x0_dev, const float* x1_dev, int n_units, float* pre_dev, float* act_dev,
                                   void* stream) {
  if (!h || !x0_dev || n_units < 1 || n_units > 16384) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: null argument or n_units outside 1 .. 16384");
  if (instr < 0 || instr >= h->cfg.n_instr) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: instr = %d outside 0 .. %d", instr, h->cfg.n_instr - 1);
  if (kind != 2 && (layer < 1 || layer > ETD_SEP_LEVELS)) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: layer = %d outside 1 .. %d", layer, ETD_SEP_LEVELS);
  hipStream_t st = (hipStream_t)stream;
  const etd_sep_cfg& c = h->cfg;
  ETD_TRY(sep_upload(h));
  const int n = n_units;
  if (kind == 0) {
    const int l = layer;
    const long long in_us = (long long)(c.T >> (l - 1)) * (c.F >> (l - 1)) * h->net.Cenc[l - 1], out_us = (long long)(c.T >> l) * (c.F >> l) * h->net.Cenc[l];
    if (!pre_dev && !act_dev) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: no output");
    ETD_TRY(sep_encoder(h, l, x0_dev, in_us, 0, 1, pre_dev, act_dev, out_us, 0, n, st, instr));
  } else if (kind == 1) {
    const int j = layer;
    const long long pix = (long long)(c.T >> (7 - j)) * (c.F >> (7 - j));
    if (!act_dev || (j > 1 && !x1_dev)) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: a decoder layer needs act_dev, and x1_dev for j > 1");
    ETD_TRY(sep_decoder(h, j, x0_dev, pix * h->net.Cenc[7 - j], j > 1 ? x1_dev : nullptr, j > 1 ? pix * h->net.Cdout[j - 1] : 0, act_dev, 4 * pix * h->net.Cdout[j], 0, n, st, instr));
  } else if (kind == 2) {
    const long long pix = (long long)c.T * c.F;
    if (!pre_dev) ETD_FAIL(ETD_EINVAL, "sep_debug_layer: the head needs pre_dev");
    ETD_TRY(sep_head(h, x0_dev, pix, pre_dev, pix * c.n_channels, 0, n, st, instr));
  } else {
    ETD_FAIL(ETD_EINVAL, "sep_debug_layer: kind = %d is not 0, 1 or 2", kind);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_debug_mask(etd_sep* h, const float* logits_dev, const float* mag_dev, const float* X_dev, long long Tf, float* Y_dev, void* stream) {
  if (!h || !logits_dev || !mag_dev || !X_dev || !Y_dev || Tf < 1) ETD_FAIL(ETD_EINVAL, "sep_debug_mask: null argument or Tf < 1");
  ETD_TRY(sep_mask(h, logits_dev, mag_dev, (const float2*)X_dev, Tf, (float2*)Y_dev, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_debug_istft(etd_sep* h, const float* Y_dev, long long N, float* out_dev, void* stream) {
  if (!h || !Y_dev || !out_dev || N < 1) ETD_FAIL(ETD_EINVAL, "sep_debug_istft: null argument or N < 1");
  hipStream_t st = (hipStream_t)stream;
  const etd_sep_cfg& c = h->cfg;
  const long long Tf = 1 + (N + c.n_fft) / c.hop, rows = (long long)c.n_instr * c.n_channels;
  ETD_TRY(sep_upload(h));
  ETD_TRY(h->ws.reserve(ws_align(rows * Tf * c.n_fft * 4), st));
  ETD_TRY(sep_istft(h, (const float2*)Y_dev, Tf, N, rows, (float*)h->ws.p, out_dev, st));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sep_debug_mwf(etd_sep* h, const float* X_dev, float* Y_dev, long long Tf, int iterations, void* stream) {
  if (!h || !X_dev || !Y_dev || Tf < 1) ETD_FAIL(ETD_EINVAL, "sep_debug_mwf: null argument or Tf < 1");
  if (iterations < 0 || iterations > SEP_MWF_MAX_ITER) ETD_FAIL(ETD_EINVAL, "sep_debug_mwf: iterations = %d must be in 0 .. %d", iterations, SEP_MWF_MAX_ITER);
  const etd_sep_cfg& c = h->cfg;
  if (c.n_channels > SEP_MWF_MAX_CHANNELS) ETD_FAIL(ETD_EINVAL, "sep_debug_mwf: Wiener filtering takes 1 or %d channels, the engine has %d", SEP_MWF_MAX_CHANNELS, c.n_channels);
  if (iterations == 0) return ETD_OK;
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(h->ws.reserve(ws_align(sep_mwf_scratch_bytes(c.n_instr, c.n_channels, c.F, Tf)), st));
  ETD_TRY(sep_mwf_run((const float2*)X_dev, (float2*)Y_dev, Tf, c.n_instr, c.n_channels, c.F, iterations, h->ws.p, st));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
