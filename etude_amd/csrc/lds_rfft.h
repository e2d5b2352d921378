// The real FFT in LDS that the stem features (csrc/stemfeat.hip, n_fft = 64 .. 4096) and the tuning estimation (csrc/tuning.hip, n_fft = 16 384) share.
//
// The plan: a real frame of n_fft samples is the complex sequence z[i] = x[2i] + i x[2i + 1] of M = n_fft / 2 points.  One Stockham (self-sorting, out of place between
// two LDS buffer pairs) FFT of M points -- a radix-2 stage first when log2 M is odd (its twiddles are all 1), then radix-4 stages, a barrier after each -- gives Z, and a
// split pass X[k] = E[k] + W^k O[k] gives the n_fft / 2 + 1 bins.  n_fft = 4096: 6 passes and barriers where the radix-2 complex FFT of the full frame takes 12.
// Twiddles come from two tables built in fp64 on the host (rfft_twiddles): every power is looked up, none is formed by a multiplication on the device.
//
// A buffer pair is two float arrays of RFFT_PM(M) words, real and imaginary parts apart, complex point i at RFFT_PAD(i).  This header holds the arithmetic, one
// butterfly or bin per call: the padding rule, the complex product, a butterfly of the radix-2 and of a radix-4 stage, a bin of the split pass.  A kernel owns the
// loops over them, the barriers and the pass order (a runtime loop over the stages for the stem features, seven passes with constant sizes for the tuning), so the
// compiler sees each kernel's loops as it did when the arithmetic was written out in them, and passes what differs: M (the functions are force-inlined, so
// constants fold) and where exp(-2 pi i n / M) is read from (TwLds / TwGlobal).  The source-level order of the floating-point operations is the contract: every
// result bit follows from it.
#pragma once
#include <cmath>
#include <vector>

#include "common.h"

// LDS index of complex point i: one float of padding after every 32, so that the power-of-two strides of the Stockham stages spread over the banks
#define RFFT_PAD(i) ((i) + ((i) >> 5))
// floats of one padded array of M points (kernels and launches size their LDS by this)
#define RFFT_PM(M) (RFFT_PAD(M) + 1)

// twM[n] = exp(-2 pi i n / M), n < M (the stages), and twS[k] = exp(-2 pi i k / (2 M)), k <= M (the split pass), rounded from fp64
inline void rfft_twiddles(int M, std::vector<float2>& twM, std::vector<float2>& twS) {
  const double pi = 3.14159265358979323846;
  const int n_fft = 2 * M;
  twM.resize(M);
  for (int n = 0; n < M; ++n) twM[n] = make_float2((float)cos(-2.0 * pi * n / M), (float)sin(-2.0 * pi * n / M));
  twS.resize(M + 1);
  for (int k = 0; k <= M; ++k) twS[k] = make_float2((float)cos(-2.0 * pi * k / n_fft), (float)sin(-2.0 * pi * k / n_fft));
}

#ifdef __HIPCC__
namespace rfft {

// exp(-2 pi i n / M) of the stages: the host table where it lies in global memory, or a copy in LDS at RFFT_PAD(n) in float2 units
struct TwGlobal { const float2* __restrict__ p; __device__ __forceinline__ float2 operator()(int n) const { return p[n]; } };
struct TwLds { const float2* p; __device__ __forceinline__ float2 operator()(int n) const { return p[RFFT_PAD(n)]; } };

// (xr + i xi)(wr + i wi) as four multiplies, a subtraction and an addition of their own (the roundings of the plain expression under -ffp-contract=off).  Left to the
// SLP vectoriser the products are paired crosswise into v_pk_mul_f32 ... op_sel:[0,1], the packed form kept out of this library (tests/test_isa_guard.py).
__device__ __forceinline__ void cmul(float xr, float xi, float wr, float wi, float& yr, float& yi) {
  float a, b, c, d;
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(a) : "v"(xr), "v"(wr));
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(b) : "v"(xi), "v"(wi));
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(c) : "v"(xr), "v"(wi));
  asm volatile("v_mul_f32 %0, %1, %2" : "=v"(d) : "v"(xi), "v"(wr));
  yr = a - b;
  yi = c + d;
}

// butterfly j < M / 2 of the opening radix-2 stage (Ns = 1, twiddles all 1): (sr, si) -> (dr, di)
__device__ __forceinline__ void radix2(const float* sr, const float* si, float* dr, float* di, int M, int j) {
  const int i0 = RFFT_PAD(j), i1 = RFFT_PAD(j + (M >> 1));
  const float ar = sr[i0], ai = si[i0], br = sr[i1], bi = si[i1];
  const int o0 = RFFT_PAD(2 * j), o1 = RFFT_PAD(2 * j + 1);
  dr[o0] = ar + br; di[o0] = ai + bi;
  dr[o1] = ar - br; di[o1] = ai - bi;
}

// butterfly j < M / 4 of one radix-4 stage, Ns points per transform so far: (sr, si) -> (dr, di).  st = M / (4 Ns) is the twiddle stride:
// w^r = exp(-2 pi i k r / (4 Ns)) = tw(k r st)
template <class Tw>
__device__ __forceinline__ void radix4(const float* sr, const float* si, float* dr, float* di, const Tw tw, int M, int Ns, int st, int j) {
  const int Q = M >> 2;
  const int k = j & (Ns - 1), j0 = ((j - k) << 2) + k;
  const int i0 = RFFT_PAD(j), i1 = RFFT_PAD(j + Q), i2 = RFFT_PAD(j + 2 * Q), i3 = RFFT_PAD(j + 3 * Q);
  const float2 w1 = tw(k * st), w2 = tw(2 * k * st), w3 = tw(3 * k * st);
  const float v0r = sr[i0], v0i = si[i0];
  float v1r, v1i, v2r, v2i, v3r, v3i;
  cmul(sr[i1], si[i1], w1.x, w1.y, v1r, v1i);
  cmul(sr[i2], si[i2], w2.x, w2.y, v2r, v2i);
  cmul(sr[i3], si[i3], w3.x, w3.y, v3r, v3i);
  const float a0r = v0r + v2r, a0i = v0i + v2i, a1r = v0r - v2r, a1i = v0i - v2i;
  const float a2r = v1r + v3r, a2i = v1i + v3i;
  const float a3r = v1i - v3i, a3i = -(v1r - v3r);          // -i (v1 - v3)
  const int o0 = RFFT_PAD(j0), o1 = RFFT_PAD(j0 + Ns), o2 = RFFT_PAD(j0 + 2 * Ns), o3 = RFFT_PAD(j0 + 3 * Ns);
  dr[o0] = a0r + a2r; di[o0] = a0i + a2i;
  dr[o1] = a1r + a3r; di[o1] = a1i + a3i;
  dr[o2] = a0r - a2r; di[o2] = a0i - a2i;
  dr[o3] = a1r - a3r; di[o3] = a1i - a3i;
}

// the split pass for bin k <= M: X[k] = E + W^k O, E = (Z[k] + conj Z[M - k]) / 2, O = -i (Z[k] - conj Z[M - k]) / 2, W^k = twS[k] = exp(-2 pi i k / n_fft);
// returns |X[k]|^2, its two squares multiplies of their own
__device__ __forceinline__ float split_power(const float* zr, const float* zi, const float2* twS, int M, int k) {
  const int ia = RFFT_PAD(k & (M - 1)), ib = RFFT_PAD((M - k) & (M - 1));
  const float ar = zr[ia], ai = zi[ia], br = zr[ib], bi = -zi[ib];
  const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
  const float orr = 0.5f * (ai - bi), oi = -0.5f * (ar - br);
  const float2 w = twS[k];
  float pr, pi;
  cmul(orr, oi, w.x, w.y, pr, pi);
  const float xr = er + pr, xi = ei + pi;
  float p0, p1;
  asm volatile("v_mul_f32 %0, %1, %1" : "=v"(p0) : "v"(xr));
  asm volatile("v_mul_f32 %0, %1, %1" : "=v"(p1) : "v"(xi));
  return p0 + p1;
}

// ---- what the separator (csrc/separator.hip) adds: the complex bin of the split pass, and the inverse transform as an inverse split pass in front of the same stages.

// the split pass for bin k <= M as a complex number: split_power's arithmetic up to X[k], returned instead of squared
__device__ __forceinline__ void split_bin(const float* zr, const float* zi, const float2* twS, int M, int k, float& xr, float& xi) {
  const int ia = RFFT_PAD(k & (M - 1)), ib = RFFT_PAD((M - k) & (M - 1));
  const float ar = zr[ia], ai = zi[ia], br = zr[ib], bi = -zi[ib];
  const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
  const float orr = 0.5f * (ai - bi), oi = -0.5f * (ar - br);
  const float2 w = twS[k];
  float pr, pi;
  cmul(orr, oi, w.x, w.y, pr, pi);
  xr = er + pr;
  xi = ei + pi;
}

// the inverse split pass for point k < M: from the bins a = X[k] and b = X[M - k] (k = 0: b = X[M]) to conj Z[k], Z = E + i O, E = (a + conj b) / 2,
// O = conj(W^k) (a - conj b) / 2, w = twS[k].  The forward stages on conj Z give R with z[n] = conj(R[n]) / M: x[2n] = R.re / M, x[2n + 1] = -R.im / M.
__device__ __forceinline__ void isplit_conj(float2 a, float2 b, float2 w, float& zr, float& zi) {
  const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);
  const float dr = 0.5f * (a.x - b.x), di = 0.5f * (a.y + b.y);
  float pr, pi;
  cmul(dr, di, w.x, -w.y, pr, pi);
  zr = er - pi;
  zi = -(ei + pr);
}

}  // namespace rfft
#endif
