// Multichannel Wiener filtering of the separator's stems (DESIGN.md 4r is the contract, tests/separator_mwf_np.py restates it; modelled on norbert.wiener /
// expectation_maximization, parity unpinned).  One song at a time, in place on its masked spectra Y [I][C][Tf][F] between k_sep_mask and k_sep_istft, with the
// mixture X [C][Tf][F]; C = 1 or 2.  Per iteration, on y / s and x / s in fp64 (s = max(1, max|X| / 10), eps = 2^-23, reg = sqrt(eps)):
//   v_j[t][k] = (1 / C) sum_c |y_jc|^2        R_j[k] = sum_t y_j y_j^H / (eps + sum_t v_j)        Cxx = sum_j v_j R_j + reg I        y_j <- v_j R_j Cxx^-1 x
//
//   k_mwf_scale   max |X|^2 per workgroup (a max has no order), folded to s and 1 / s by k_mwf_scale_fold; once per song
//   k_mwf_stats   one thread per (source, bin) and chunk of 64 frames: reads Y once, frame after frame, and writes the chunk's sums of y y^H and v
//   k_mwf_reduce  one thread per (source, bin): adds the chunks in ascending order and forms R
//   k_mwf_apply   one workgroup per 64 bins x 32 frames, R of its bins in LDS; a thread reads x and the I sources' y of a (t, k), recomputes v (never stored), forms
//                 Cxx, its closed-form inverse and the gains in registers and writes Y in place, rounded to fp32 once
// Every global access is a float2 (or a double) at consecutive k across a wave: Y and X are k-fastest.  No atomics, vector stores only; a sum's order is fixed by
// the song's frame count alone, and a song reads nothing but its own X and Y: bit-identical alone, in any batch, under any workspace budget, from run to run.
#include "separator.h"
#include "prof.h"

namespace {

constexpr int MWF_SCALE_BLOCKS = 1024;     // most workgroups of k_mwf_scale (= partial maxima)
constexpr int MWF_TT = 32;                 // frames per workgroup of k_mwf_apply (8 per wave)
constexpr double MWF_EPS = 1.1920928955078125e-07;          // 2^-23
constexpr double MWF_REG = 3.4526698300124393e-04;          // sqrt(2^-23)

// slots of a (source, bin): C = 1: |y|^2, then sum v; C = 2: |y_0|^2, |y_1|^2, Re and Im of y_0 conj(y_1), then sum v.  R keeps the first C * C.
__host__ __device__ constexpr int mwf_nr(int C) { return C * C; }

__device__ __forceinline__ double mwf_wave_max(double m) {
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  return m;
}

// pmax[block] = max |X|^2 over the elements the workgroup strides through
__global__ __launch_bounds__(SEP_THREADS) void k_mwf_scale(const float2* __restrict__ X, long long n, double* __restrict__ pmax) {
  __shared__ double sm[SEP_THREADS / 64];
  double m = 0.0;
  for (long long e = (long long)blockIdx.x * SEP_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * SEP_THREADS) {
    const float2 x = X[e];
    m = fmax(m, (double)x.x * (double)x.x + (double)x.y * (double)x.y);
  }
  m = mwf_wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) pmax[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

// sc[0] = s = max(1, max|X| / 10), sc[1] = 1 / s; one workgroup
__global__ __launch_bounds__(SEP_THREADS) void k_mwf_scale_fold(const double* __restrict__ pmax, int n, double* __restrict__ sc) {
  __shared__ double sm[SEP_THREADS / 64];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += SEP_THREADS) m = fmax(m, pmax[i]);
  m = mwf_wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = fmax(1.0, sqrt(fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]))) / 10.0);
    sc[0] = s; sc[1] = 1.0 / s;
  }
}

// grid (chunks, ceil(I F / 256)): part [chunk][slot][j F + k] = the chunk's sums, its frames added in ascending order
template <int C> __global__ __launch_bounds__(SEP_THREADS) void k_mwf_stats(const float2* __restrict__ Y, long long Tf, int F, int IF, const double* __restrict__ sc,
                                                                            double* __restrict__ part) {
  const int e = blockIdx.y * SEP_THREADS + threadIdx.x;
  if (e >= IF) return;
  const int j = e / F, k = e - j * F;
  const long long t0 = (long long)blockIdx.x * SEP_MWF_CHUNK;
  const int n = (int)(Tf - t0 < SEP_MWF_CHUNK ? Tf - t0 : SEP_MWF_CHUNK);
  const long long plane = Tf * F;
  const double is = sc[1];
  const float2* y = Y + ((long long)j * C) * plane + t0 * F + k;
  double r00 = 0.0, r11 = 0.0, re = 0.0, im = 0.0, sv = 0.0;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const float2 a = y[(long long)i * F];
    const double ax = a.x * is, ay = a.y * is, pa = ax * ax + ay * ay;
    r00 += pa;
    if (C == 2) {
      const float2 b = y[plane + (long long)i * F];
      const double bx = b.x * is, by = b.y * is, pb = bx * bx + by * by;
      r11 += pb;
      re += ax * bx + ay * by;                           // y_0 conj(y_1)
      im += ay * bx - ax * by;
      sv += 0.5 * (pa + pb);
    } else {
      sv += pa;
    }
  }
  double* p = part + (long long)blockIdx.x * (mwf_nr(C) + 1) * IF + e;
  p[0] = r00;
  if (C == 2) { p[IF] = r11; p[2LL * IF] = re; p[3LL * IF] = im; }
  p[(long long)mwf_nr(C) * IF] = sv;
}

// R [slot][j F + k] = (the chunks' sums, added in ascending order) / (eps + sum v)
template <int C> __global__ __launch_bounds__(64) void k_mwf_reduce(const double* __restrict__ part, int chunks, int IF, double* __restrict__ R) {
  constexpr int NR = mwf_nr(C), NP = NR + 1;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= IF) return;
  double s[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) s[p] = 0.0;
#pragma unroll 4
  for (int c = 0; c < chunks; ++c) {
    const double* q = part + (long long)c * NP * IF + e;
#pragma unroll
    for (int p = 0; p < NP; ++p) s[p] += q[(long long)p * IF];
  }
  const double den = MWF_EPS + s[NR];
#pragma unroll
  for (int p = 0; p < NR; ++p) R[(long long)p * IF + e] = s[p] / den;
}

// grid (ceil(Tf / 32), F / 64), dynamic LDS I * C * C * 64 doubles: the R of the workgroup's 64 bins, [j][slot][bin]
template <int C, int I> __global__ __launch_bounds__(SEP_THREADS) void k_mwf_apply(const float2* __restrict__ X, float2* Y, const double* __restrict__ R,
                                                                                  const double* __restrict__ sc, long long Tf, int F) {
  extern __shared__ __attribute__((aligned(16))) double lr[];
  constexpr int NR = mwf_nr(C);
  const int tid = threadIdx.x, kk = tid & 63, w = tid >> 6, k0 = blockIdx.y * 64, IF = I * F;
  for (int idx = tid; idx < I * NR * 64; idx += SEP_THREADS) {
    const int jp = idx >> 6, j = jp / NR, p = jp - j * NR;
    lr[idx] = R[(long long)p * IF + j * F + k0 + (idx & 63)];
  }
  __syncthreads();
  const double s = sc[0], is = sc[1];
  const long long plane = Tf * F, tb = (long long)blockIdx.x * MWF_TT;
  for (int i = w; i < MWF_TT; i += SEP_THREADS / 64) {
    const long long t = tb + i;
    if (t >= Tf) break;
    const long long o = t * F + k0 + kk;
    float2 ya[I], yb[C == 2 ? I : 1];
#pragma unroll
    for (int j = 0; j < I; ++j) {
      ya[j] = Y[(long long)j * C * plane + o];
      if (C == 2) yb[j] = Y[((long long)j * C + 1) * plane + o];
    }
    const float2 xa = X[o];
    double v[I];
    if (C == 1) {
      double cxx = 0.0;
#pragma unroll
      for (int j = 0; j < I; ++j) {
        const double ax = ya[j].x * is, ay = ya[j].y * is;
        v[j] = ax * ax + ay * ay;
        cxx += v[j] * lr[j * 64 + kk];
      }
      cxx += MWF_REG;
      const double zx = (xa.x * is) / cxx, zy = (xa.y * is) / cxx;
#pragma unroll
      for (int j = 0; j < I; ++j) {
        const double g = (v[j] * lr[j * 64 + kk]) * s;
        Y[(long long)j * plane + o] = make_float2((float)(g * zx), (float)(g * zy));
      }
    } else {
      const float2 xb = X[plane + o];
      double c00 = 0.0, c11 = 0.0, cre = 0.0, cim = 0.0;
#pragma unroll
      for (int j = 0; j < I; ++j) {
        const double ax = ya[j].x * is, ay = ya[j].y * is, bx = yb[j].x * is, by = yb[j].y * is;
        v[j] = 0.5 * ((ax * ax + ay * ay) + (bx * bx + by * by));
        const double* r = lr + j * NR * 64 + kk;
        c00 += v[j] * r[0]; c11 += v[j] * r[64]; cre += v[j] * r[128]; cim += v[j] * r[192];
      }
      c00 += MWF_REG; c11 += MWF_REG;
      // Cxx = [c00, c01; conj(c01), c11] is Hermitian: its inverse is [c11, -c01; -conj(c01), c00] / (c00 c11 - |c01|^2); z = Cxx^-1 x
      const double det = c00 * c11 - (cre * cre + cim * cim);
      const double x0r = xa.x * is, x0i = xa.y * is, x1r = xb.x * is, x1i = xb.y * is;
      const double z0r = (c11 * x0r - (cre * x1r - cim * x1i)) / det, z0i = (c11 * x0i - (cre * x1i + cim * x1r)) / det;
      const double z1r = (c00 * x1r - (cre * x0r + cim * x0i)) / det, z1i = (c00 * x1i - (cre * x0i - cim * x0r)) / det;
#pragma unroll
      for (int j = 0; j < I; ++j) {
        const double* r = lr + j * NR * 64 + kk;
        const double r00 = r[0], r11 = r[64], rr = r[128], ri = r[192], g = v[j] * s;
        // R_j z: row 0 = r00 z0 + r01 z1, row 1 = conj(r01) z0 + r11 z1
        const double o0r = r00 * z0r + (rr * z1r - ri * z1i), o0i = r00 * z0i + (rr * z1i + ri * z1r);
        const double o1r = (rr * z0r + ri * z0i) + r11 * z1r, o1i = (rr * z0i - ri * z0r) + r11 * z1i;
        Y[(long long)j * C * plane + o] = make_float2((float)(g * o0r), (float)(g * o0i));
        Y[((long long)j * C + 1) * plane + o] = make_float2((float)(g * o1r), (float)(g * o1i));
      }
    }
  }
}

struct MwfScratch {                        // in doubles from the scratch's start
  long long chunks, pmax, sc, R, part, total;
  MwfScratch(int I, int C, int F, long long Tf) {
    chunks = (Tf + SEP_MWF_CHUNK - 1) / SEP_MWF_CHUNK;
    const long long IF = (long long)I * F;
    pmax = 0; sc = pmax + MWF_SCALE_BLOCKS; R = sc + 32; part = R + mwf_nr(C) * IF; total = part + chunks * (mwf_nr(C) + 1) * IF;
  }
};

// the instantiation of k_mwf_apply for `n` sources
template <int C, int I = 1> int mwf_apply(int n, dim3 grid, hipStream_t st, const float2* X, float2* Y, const double* R, const double* sc, long long Tf, int F) {
  if (n == I) {
    hipLaunchKernelGGL((k_mwf_apply<C, I>), grid, dim3(SEP_THREADS), (size_t)I * mwf_nr(C) * 64 * sizeof(double), st, X, Y, R, sc, Tf, F);
    return ETD_OK;
  }
  if constexpr (I < ETD_SEP_MAX_INSTR) return mwf_apply<C, I + 1>(n, grid, st, X, Y, R, sc, Tf, F);
  ETD_FAIL(ETD_EINVAL, "separator: Wiener filtering of %d sources (1 .. %d)", n, ETD_SEP_MAX_INSTR);
}

template <int C> int mwf_run(const float2* X, float2* Y, long long Tf, int I, int F, int iterations, double* d, hipStream_t st) {
  const MwfScratch m(I, C, F, Tf);
  const int IF = I * F;
  const long long nx = (long long)C * Tf * F;
  const double ybytes = (double)I * C * Tf * F * 8.0;
  if (m.chunks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "separator: more than 2^31 - 1 workgroups in the Wiener filter");
  long long sb = (nx + SEP_THREADS - 1) / SEP_THREADS;
  if (sb > MWF_SCALE_BLOCKS) sb = MWF_SCALE_BLOCKS;
  {
    ProfScope ps("k_mwf_scale", st, 0, (double)nx * 8.0);
    hipLaunchKernelGGL(k_mwf_scale, dim3((unsigned)sb), dim3(SEP_THREADS), 0, st, X, nx, d + m.pmax);
    hipLaunchKernelGGL(k_mwf_scale_fold, dim3(1), dim3(SEP_THREADS), 0, st, d + m.pmax, (int)sb, d + m.sc);
  }
  for (int it = 0; it < iterations; ++it) {
    {
      ProfScope ps("k_mwf_stats", st, 0, ybytes);
      hipLaunchKernelGGL(k_mwf_stats<C>, dim3((unsigned)m.chunks, (unsigned)((IF + SEP_THREADS - 1) / SEP_THREADS)), dim3(SEP_THREADS), 0, st, Y, Tf, F, IF, d + m.sc,
                         d + m.part);
    }
    {
      ProfScope ps("k_mwf_reduce", st, 0, (double)m.chunks * (mwf_nr(C) + 1) * IF * 8.0);
      hipLaunchKernelGGL(k_mwf_reduce<C>, dim3((unsigned)((IF + 63) / 64)), dim3(64), 0, st, d + m.part, (int)m.chunks, IF, d + m.R);
    }
    {
      ProfScope ps("k_mwf_apply", st, 0, 2.0 * ybytes + (double)nx * 8.0);
      ETD_TRY(mwf_apply<C>(I, dim3((unsigned)((Tf + MWF_TT - 1) / MWF_TT), (unsigned)(F / 64)), st, X, Y, d + m.R, d + m.sc, Tf, F));
    }
  }
  return ETD_OK;
}

}  // namespace

long long sep_mwf_scratch_bytes(int I, int C, int F, long long Tf) { return MwfScratch(I, C, F, Tf).total * 8; }

int sep_mwf_run(const float2* X, float2* Y, long long Tf, int I, int C, int F, int iterations, void* scratch, hipStream_t st) {
  if (!X || !Y || !scratch || Tf < 1) ETD_FAIL(ETD_EINVAL, "separator: Wiener filter: null argument or Tf < 1");
  if (iterations < 1 || iterations > SEP_MWF_MAX_ITER) ETD_FAIL(ETD_EINVAL, "separator: mwf iterations = %d must be in 1 .. %d", iterations, SEP_MWF_MAX_ITER);
  if (I < 1 || I > ETD_SEP_MAX_INSTR || F < 64 || F % 64) ETD_FAIL(ETD_EINVAL, "separator: Wiener filter: %d sources, F = %d", I, F);
  if (C == 1) return mwf_run<1>(X, Y, Tf, I, F, iterations, (double*)scratch, st);
  if (C == 2) return mwf_run<2>(X, Y, Tf, I, F, iterations, (double*)scratch, st);
  ETD_FAIL(ETD_EINVAL, "separator: Wiener filtering takes 1 or 2 channels, not %d", C);
}
