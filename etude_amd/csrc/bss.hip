// BSS Eval v4 on the GPU: references and estimates [J][C][N] fp32 -> the eight energies per (source, window) that SDR / ISR / SIR / SAR and the plain SDR are formed
// from.  DESIGN.md 4p is the contract (this project's own, modelled on museval's bss_eval with time-invariant filters; parity unpinned); tests/bss_np.py restates it.
//
// Everything is fp64.  One tile routine on v_mfma_f64_16x16x4_f64 serves three kernels:
//   k_bss_corr     the lagged correlations as a GEMM: rows (signal, lag) gathered Hankel-wise from one LDS image of a sample chunk, columns the lag-0 references,
//                  K the samples of a slice; per-slice partials, joined in slice order by k_bss_corr_join
//   k_bss_syrk     the trailing update of the blocked right-looking Cholesky (panel 16: k_bss_potrf16, k_bss_trsm, k_bss_syrk per panel)
//   k_bss_project  a window's projections as a GEMM: rows the output samples gathered Toeplitz-wise from an LDS image of the window's references, K = (signal, tap),
//                  columns the S columns of A and the S of the block-diagonal B
// Lane maps of the instruction (lane l, r = l & 15, h = l >> 4): A[row r][k h], B[k h][col r], C/D register i = [row h + 4 i][col r] -- NOT the other shapes' C/D map.
// No atomics; every sum runs in an order the shapes fix; tracks run one after another in one workspace, so a track's bits depend on its samples alone.
#include "bss.h"
#include "host_util.h"
#include "etude_hip.h"
#include "etude_hip_debug.h"

#include <vector>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma_f64(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// window w of a track: samples a .. b - 1; the last window runs to N, a track below one window is one window
__host__ __device__ __forceinline__ void bss_window(int w, int nwin, int window, int hop, long long N, long long* a, long long* b) {
  *a = (long long)w * hop;
  *b = (w == nwin - 1) ? N : *a + window;
}

// ---------------------------------------------------------------------------------------------------------------- step 1: correlations
// grid (slices, 2 S signals z, ceil(L / 256)); 256 threads.  part [slice][z][L][S] = sum over the slice's n of z[n + lag] x_col[n].
__global__ __launch_bounds__(256) void k_bss_corr(const BssTrack t, double* part) {
  __shared__ float Aimg[BSS_CHUNK + BSS_LAGS_PER_WG];
  __shared__ float Bimg[BSS_CHUNK * 16];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, kk = lane >> 4;
  const int slice = (int)blockIdx.x, zi = (int)blockIdx.y, lg0 = (int)blockIdx.z * BSS_LAGS_PER_WG;
  const float* z = (zi < t.S ? t.ref + (long long)zi * t.N : t.est + (long long)(zi - t.S) * t.N);
  const int l0 = lg0 + 64 * wave;
  const bool active = l0 < t.L;
  const long long s_begin = (long long)slice * BSS_SLICE;
  d4 hi[4], lo[4];                                             // the running sums as unevaluated pairs hi + lo
#pragma unroll
  for (int i = 0; i < 4; ++i) { hi[i] = (d4){0.0, 0.0, 0.0, 0.0}; lo[i] = hi[i]; }
  for (int ch = 0; ch < BSS_SLICE / BSS_CHUNK; ++ch) {
    const long long nb = s_begin + (long long)ch * BSS_CHUNK;
    if (nb >= t.N) break;                                     // (uniform)
    __syncthreads();
    for (int i = tid; i < BSS_CHUNK + BSS_LAGS_PER_WG; i += 256) {
      const long long g = nb + lg0 + i;
      Aimg[i] = g < t.N ? z[g] : 0.f;
    }
    for (int i = tid; i < BSS_CHUNK * 16; i += 256) {
      const int col = i / BSS_CHUNK, c = i % BSS_CHUNK;
      const long long g = nb + c;
      Bimg[c * 16 + col] = (col < t.S && g < t.N) ? t.ref[(long long)col * t.N + g] : 0.f;
    }
    __syncthreads();
    if (!active) continue;
    for (int u = 0; u < BSS_CHUNK / 64; ++u) {                // 16 steps of 4 samples; a step is ONE MFMA from zero (products exact, three roundings), added by TwoSum
      const int s0 = 16 * u;
      double av[28], bv[16];
#pragma unroll
      for (int q = 0; q < 28; ++q) av[q] = (double)Aimg[4 * (s0 + q) + kk + 64 * wave + r];      // <= 766
#pragma unroll
      for (int q = 0; q < 16; ++q) bv[q] = (double)Bimg[(4 * (s0 + q) + kk) * 16 + r];
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int lb = 0; lb < 4; ++lb) {
          const d4 p = mfma_f64(av[s + 4 * lb], bv[s], (d4){0.0, 0.0, 0.0, 0.0});
          const d4 sum = hi[lb] + p, bb = sum - hi[lb];
          lo[lb] += (hi[lb] - (sum - bb)) + (p - bb);
          hi[lb] = sum;
        }
    }
  }
  if (!active) return;
#pragma unroll
  for (int lb = 0; lb < 4; ++lb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lag = l0 + 16 * lb + kk + 4 * i;
      if (lag < t.L && r < t.S) part[(((long long)slice * (2 * t.S) + zi) * t.L + lag) * t.S + r] = hi[lb][i] + lo[lb][i];
    }
}

// the partials in slice order -> r [S][S][L] (r[p][q][l]: q shifted) and d [S][S][L] (d[p][e][l]: the estimate shifted)
__global__ void k_bss_corr_join(const double* part, int n_slices, int S, int L, double* r, double* d) {
  const long long per = (long long)2 * S * L * S;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per) return;
  double acc = 0.0, low = 0.0;                                 // TwoSum over the slices, in slice order
  for (int s = 0; s < n_slices; ++s) {
    const double v = part[s * per + i], sum = acc + v, bb = sum - acc;
    low += (acc - (sum - bb)) + (v - bb);
    acc = sum;
  }
  acc += low;
  const int p = (int)(i % S), lag = (int)((i / S) % L), zi = (int)(i / ((long long)S * L));
  if (zi < S) r[((long long)p * S + zi) * L + lag] = acc;
  else d[((long long)p * S + (zi - S)) * L + lag] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- step 2: matrices
// G [(p, k)][(q, m)] over the P signals from sel0 (n = P L): r_pq[k - m] or r_qp[m - k], eps on the diagonal
__global__ void k_bss_gram(const double* r, int S, int L, int sel0, int P, double* G) {
  const long long n = (long long)P * L;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n) return;
  const int row = (int)(i / n), col = (int)(i % n);
  const int p = sel0 + row / L, k = row % L, q = sel0 + col / L, m = col % L;
  double v = k >= m ? r[((long long)p * S + q) * L + (k - m)] : r[((long long)q * S + p) * L + (m - k)];
  if (row == col) v += 0x1p-52;
  G[i] = v;
}
// right-hand sides [n][16]: column e < ne is d[p][e0 + e][k]; the rest is zero
__global__ void k_bss_rhs(const double* d, int S, int L, int sel0, int P, int e0, int ne, double* Dm) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= P * L * 16) return;
  const int row = i >> 4, e = i & 15;
  const int p = sel0 + row / L, k = row % L;
  Dm[i] = e < ne ? d[((long long)p * S + (e0 + e)) * L + k] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky, panel 16, in place in the lower triangle
__global__ __launch_bounds__(256) void k_bss_potrf16(double* G, int ld, int k0, int* status) {
  __shared__ double a[16][17];
  const int tid = (int)threadIdx.x, r = tid >> 4, c2 = tid & 15;
  a[r][c2] = G[(long long)(k0 + r) * ld + k0 + c2];
  __syncthreads();
  for (int c = 0; c < 16; ++c) {
    double piv = a[c][c];
    if (!(piv > 0.0) || !isfinite(piv)) {
      piv = __builtin_nan("");
      if (tid == 0) *status = 1;
    }
    __syncthreads();
    const double dd = sqrt(piv);
    if (c2 == c && r >= c) a[r][c] = (r == c) ? dd : a[r][c] / dd;
    __syncthreads();
    if (c2 > c && r >= c2) a[r][c2] -= a[r][c] * a[c2][c];
    __syncthreads();
  }
  if (c2 <= r) G[(long long)(k0 + r) * ld + k0 + c2] = a[r][c2];
}

// the panel below the diagonal block: L_ik = A_ik L_kk^-T, one thread per row
__global__ __launch_bounds__(256) void k_bss_trsm(double* G, int ld, int n, int k0) {
  __shared__ double Lk[16][17];
  const int tid = (int)threadIdx.x;
  Lk[tid >> 4][tid & 15] = G[(long long)(k0 + (tid >> 4)) * ld + k0 + (tid & 15)];
  __syncthreads();
  const int i = k0 + 16 + (int)blockIdx.x * 256 + tid;
  if (i >= n) return;
  double* row = G + (long long)i * ld + k0;
  double x[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    double v = row[c];
#pragma unroll
    for (int u = 0; u < c; ++u) v -= x[u] * Lk[c][u];
    x[c] = v / Lk[c][c];
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) row[c] = x[c];
}

// the trailing update C_ij -= P_i P_j^T on the tiles of the lower triangle: one wave per tile, four MFMAs.  grid (ceil(mb / 4), mb)
__global__ __launch_bounds__(256) void k_bss_syrk(double* G, int ld, int k0, int mb) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, kk = lane >> 4;
  const int ti = (int)blockIdx.y, tj = (int)blockIdx.x * 4 + wave;
  if (tj > ti || tj >= mb) return;
  const long long i0 = k0 + 16 + 16 * ti, j0 = k0 + 16 + 16 * tj;
  d4 c;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = G[(i0 + kk + 4 * i) * ld + j0 + r];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double a = -G[(i0 + r) * ld + k0 + 4 * s + kk];
    const double b = G[(j0 + r) * ld + k0 + 4 * s + kk];
    c = mfma_f64(a, b, c);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) G[(i0 + kk + 4 * i) * ld + j0 + r] = c[i];
}

// forward and backward substitution of 16 right-hand sides Dm [n][16] in place: ONE workgroup, block by block in a fixed order
__global__ __launch_bounds__(1024) void k_bss_subst(const double* G, int ld, int n, double* Dm) {
  __shared__ double Lk[16][17], X[16][17];
  const int tid = (int)threadIdx.x, e = tid & 15, rr = tid >> 4;
  const int nb = n / 16;
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = 16 * kb;
    if (tid < 256) { Lk[rr][e] = G[(long long)(k0 + rr) * ld + k0 + e]; X[rr][e] = Dm[(k0 + rr) * 16 + e]; }
    __syncthreads();
    if (tid < 16)
      for (int t = 0; t < 16; ++t) {
        double v = X[t][e];
        for (int u = 0; u < t; ++u) v -= Lk[t][u] * X[u][e];
        X[t][e] = v / Lk[t][t];
      }
    __syncthreads();
    if (tid < 256) Dm[(k0 + rr) * 16 + e] = X[rr][e];
    for (int i = k0 + 16 + rr; i < n; i += 64) {
      const double* row = G + (long long)i * ld + k0;
      double v = Dm[i * 16 + e];
#pragma unroll
      for (int t = 0; t < 16; ++t) v -= row[t] * X[t][e];
      Dm[i * 16 + e] = v;
    }
    __syncthreads();
  }
  for (int kb = nb - 1; kb >= 0; --kb) {
    const int k0 = 16 * kb;
    if (tid < 256) { Lk[rr][e] = G[(long long)(k0 + rr) * ld + k0 + e]; X[rr][e] = Dm[(k0 + rr) * 16 + e]; }
    __syncthreads();
    if (tid < 16)
      for (int t = 15; t >= 0; --t) {
        double v = X[t][e];
        for (int u = 15; u > t; --u) v -= Lk[u][t] * X[u][e];
        X[t][e] = v / Lk[t][t];
      }
    __syncthreads();
    if (tid < 256) Dm[(k0 + rr) * 16 + e] = X[rr][e];
    for (int i = rr; i < k0; i += 64) {
      double v = Dm[i * 16 + e];
#pragma unroll
      for (int t = 15; t >= 0; --t) v -= G[(long long)(k0 + t) * ld + i] * X[t][e];
      Dm[i * 16 + e] = v;
    }
    __syncthreads();
  }
}

// where the residual of a solve reads the system it was assembled from: G as P x P blocks of order L and the right-hand sides [P L][16]
struct BssFromCorr {
  const double *r, *d;
  int S, L, sel0, P, e0, ne;
  __device__ __forceinline__ int blocks() const { return P; }
  __device__ __forceinline__ int order() const { return L; }
  __device__ __forceinline__ double g(int p, int k, int q, int m) const {
    const double v = k >= m ? r[((long long)(sel0 + p) * S + sel0 + q) * L + (k - m)] : r[((long long)(sel0 + q) * S + sel0 + p) * L + (m - k)];
    return (p == q && k == m) ? v + 0x1p-52 : v;
  }
  __device__ __forceinline__ double rhs(int p, int k, int e) const { return e < ne ? d[((long long)(sel0 + p) * S + (e0 + e)) * L + k] : 0.0; }
};
struct BssFromMatrix {            // a caller's G [n][n] and right-hand sides [n][m], padded to np with the identity
  const double *G, *B;
  int n, m, np;
  __device__ __forceinline__ int blocks() const { return 1; }
  __device__ __forceinline__ int order() const { return np; }
  __device__ __forceinline__ double g(int, int k, int, int c) const { return (k < n && c < n) ? G[(long long)k * n + c] : (k == c ? 1.0 : 0.0); }
  __device__ __forceinline__ double rhs(int, int k, int e) const { return (k < n && e < m) ? B[(long long)k * m + e] : 0.0; }
};
// R [n][16] = D - G X with every product split exactly (fma) and every sum a TwoSum: one thread per entry, columns in order.  One step of iterative refinement
// then solves G dX = R with the factor at hand (k_bss_subst) and adds dX (k_bss_add).
template <class Src>
__global__ void k_bss_residual(const Src src, const double* X, double* R) {
  const int P = src.blocks(), Lo = src.order();
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= P * Lo * 16) return;
  const int row = i >> 4, e = i & 15, p = row / Lo, k = row % Lo;
  double hi = src.rhs(p, k, e), lo = 0.0;
  for (int q = 0; q < P; ++q)
    for (int m = 0; m < Lo; ++m) {
      const double g = src.g(p, k, q, m), x = X[(q * Lo + m) * 16 + e];
      const double pr = -(g * x), pe = -__builtin_fma(g, x, pr);      // g x = -(pr + pe) exactly
      const double sum = hi + pr, bb = sum - hi;
      lo += ((hi - (sum - bb)) + (pr - bb)) + pe;
      hi = sum;
    }
  R[i] = hi + lo;
}
__global__ void k_bss_add(double* X, const double* dX, int n16) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n16) X[i] += dX[i];
}

// a caller's matrix [n][n] into the padded square [np][np] (identity on the padding) and its right-hand sides [n][m] into [np][16]
__global__ void k_bss_pad_matrix(const double* A, int n, int np, double* G) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)np * np) return;
  const int row = (int)(i / np), col = (int)(i % np);
  G[i] = (row < n && col < n) ? A[(long long)row * n + col] : (row == col ? 1.0 : 0.0);
}
__global__ void k_bss_pad_rhs(const double* B, int n, int m, int np, double* Dm) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= np * 16) return;
  const int row = i >> 4, e = i & 15;
  Dm[i] = (row < n && e < m) ? B[(long long)row * m + e] : 0.0;
}
// [n][16] -> the first m columns [n][m]
__global__ void k_bss_take_cols(const double* Dm, int n, int m, double* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * m) return;
  out[i] = Dm[(i / m) * 16 + i % m];
}
// ... and back: a caller's filters [n][m] into [n][16]
__global__ void k_bss_put_cols(const double* in, int n, int m, double* Dm) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * 16) return;
  Dm[i] = (i & 15) < m ? in[(long long)(i >> 4) * m + (i & 15)] : 0.0;
}

// F [S L][NC]: columns 0 .. S - 1 the all-source filters A, columns S + (j, c) the block-diagonal B_j (rows of source j only), zeros elsewhere
__global__ void k_bss_pack(const double* DmA, const double* DmB, int J, int C, int L, int NC, double* F) {
  const int S = J * C, n = S * L;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * NC) return;
  const int row = i / NC, col = i % NC;
  double v = 0.0;
  if (col < S) v = DmA[row * 16 + col];
  else if (col < 2 * S) {
    const int j = (col - S) / C, c = (col - S) % C, p = row / L, k = row % L;
    if (p / C == j) v = DmB[((long long)j * C * L + (p % C) * L + k) * 16 + c];
  }
  F[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- step 3: silent windows
__global__ __launch_bounds__(256) void k_bss_silent(const BssTrack t, int* silent) {
  const int w = (int)blockIdx.x, tid = (int)threadIdx.x;
  long long a, b;
  bss_window(w, t.nwin, t.window, t.hop, t.N, &a, &b);
  int flag = 0;
  for (int src = 0; src < 2 * t.J; ++src) {
    const float* x = (src < t.J ? t.ref + (long long)src * t.C * t.N : t.est + (long long)(src - t.J) * t.C * t.N);
    int nz = 0;
    for (int c = 0; c < t.C; ++c)
      for (long long n = a + tid; n < b; n += 256) nz |= x[c * t.N + n] != 0.f;
    if (!__syncthreads_or(nz)) flag = 1;
  }
  if (tid == 0) silent[w] = flag;
}

// ---------------------------------------------------------------------------------------------------------------- step 4: projections
// grid (ceil(Wout / 256), windows of this batch); 256 threads; dynamic LDS S (256 + L) floats.  P [window][wout_max][NC]: columns as F's.
__global__ __launch_bounds__(256) void k_bss_project(const BssTrack t, const double* F, int NC, int w_first, int wout_max, double* P) {
  extern __shared__ float Ximg[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, kk = lane >> 4;
  const int w = w_first + (int)blockIdx.y, L = t.L, IM = BSS_ROWS_PER_WG + L;
  long long a, b;
  bss_window(w, t.nwin, t.window, t.hop, t.N, &a, &b);
  const long long Ww = b - a, Wout = Ww + L - 1;
  const long long n_base = (long long)blockIdx.x * BSS_ROWS_PER_WG;
  if (n_base >= Wout) return;                                  // (uniform)
  for (int i = tid; i < t.S * IM; i += 256) {
    const int p = i / IM;
    const long long m = n_base - L + (i % IM);                 // window-local sample; zero outside the window
    Ximg[i] = (m >= 0 && m < Ww) ? t.ref[(long long)p * t.N + a + m] : 0.f;
  }
  __syncthreads();
  const int nct = NC / 16;
  d4 tot[4][2], in[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) { tot[i][0] = (d4){0.0, 0.0, 0.0, 0.0}; tot[i][1] = tot[i][0]; }
  for (int p = 0; p < t.S; ++p) {
    const float* img = Ximg + p * IM;
#pragma unroll
    for (int i = 0; i < 4; ++i) { in[i][0] = (d4){0.0, 0.0, 0.0, 0.0}; in[i][1] = in[i][0]; }
    for (int s0 = 0; s0 < L / 4; s0 += 4) {                    // 16 taps: tile tq at step ds reads x[n0 + 16 tq + r - 4 (s0 + ds) - kk] = xv[4 tq - ds + 3]
      double xv[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) xv[q] = (double)img[64 * wave + L + r - kk - 4 * s0 + 4 * (q - 3)];
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        const double* frow = F + ((long long)p * L + 4 * (s0 + ds) + kk) * NC + r;
        const double f0 = frow[0];
        const double f1 = nct > 1 ? frow[16] : 0.0;
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
          in[tq][0] = mfma_f64(xv[4 * tq - ds + 3], f0, in[tq][0]);
          if (nct > 1) in[tq][1] = mfma_f64(xv[4 * tq - ds + 3], f1, in[tq][1]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { tot[i][0] += in[i][0]; tot[i][1] += in[i][1]; }
  }
  double* out = P + (long long)blockIdx.y * wout_max * NC;
#pragma unroll
  for (int tq = 0; tq < 4; ++tq)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long n = n_base + 64 * wave + 16 * tq + kk + 4 * i;
      if (n < Wout) {
        if (r < 2 * t.S) out[n * NC + r] = tot[tq][0][i];
        if (nct > 1 && 16 + r < 2 * t.S) out[n * NC + 16 + r] = tot[tq][1][i];
      }
    }
}

// P -> ps [J][C][Wout], pa [J][C][Wout] of one window (the tap's output)
__global__ void k_bss_unpack_proj(const double* P, int S, int NC, long long Wout, double* ps, double* pa) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * Wout) return;
  const int sig = (int)(i / Wout);
  const long long n = i % Wout;
  pa[i] = P[n * NC + sig];
  ps[i] = P[n * NC + S + sig];
}

// ---------------------------------------------------------------------------------------------------------------- step 5: energies
// grid (J, windows of this batch); 256 threads: thread t adds samples t, t + 256, ... channel by channel, then a fixed tree.  E [J][nwin][8]
__global__ __launch_bounds__(256) void k_bss_energy(const BssTrack t, const double* P, int NC, int w_first, int wout_max, const int* silent, const int* status, double* E) {
  __shared__ double red[8][256];
  const int tid = (int)threadIdx.x, j = (int)blockIdx.x, w = w_first + (int)blockIdx.y;
  long long a, b;
  bss_window(w, t.nwin, t.window, t.hop, t.N, &a, &b);
  const long long Ww = b - a, Wout = Ww + t.L - 1;
  const double* Pw = P + (long long)blockIdx.y * wout_max * NC;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < t.C; ++c) {
    const int sig = j * t.C + c;
    const float* x = t.ref + (long long)sig * t.N + a;
    const float* y = t.est + (long long)sig * t.N + a;
    for (long long n = tid; n < Wout; n += 256) {
      const double s = n < Ww ? (double)x[n] : 0.0, ye = n < Ww ? (double)y[n] : 0.0;
      const double pa = Pw[n * NC + sig], ps = Pw[n * NC + t.S + sig];
      const double e_spat = ps - s, e_interf = pa - ps, e_artif = ye - pa;
      const double v1 = (e_spat + e_interf) + e_artif, v3 = s + e_spat, v5 = v3 + e_interf, v7 = s - ye;
      acc[0] += s * s; acc[1] += v1 * v1; acc[2] += e_spat * e_spat; acc[3] += v3 * v3;
      acc[4] += e_interf * e_interf; acc[5] += v5 * v5; acc[6] += e_artif * e_artif;
      if (n < Ww) acc[7] += v7 * v7;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[i][tid] = acc[i];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h)
#pragma unroll
      for (int i = 0; i < 8; ++i) red[i][tid] += red[i][tid + h];
    __syncthreads();
  }
  if (tid < 8) E[((long long)j * t.nwin + w) * 8 + tid] = (silent[w] || *status) ? __builtin_nan("") : red[tid][0];
}

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

// ================================================================================================================ the handle
struct BssLayout {            // offsets into the workspace; bytes at the end
  long long part, r, d, G, Gj, DmA, DmB, DmR, F, P, bytes_fixed, per_window, bytes_min;
  int n_slices, NC, wout_max;
};

struct etd_bss {
  etd_bss_cfg cfg;
  long long budget;
  void* ws = nullptr;
  long long ws_bytes = 0;
  bool timing = false;
  double stage_ms[5] = {0, 0, 0, 0, 0};
  std::vector<std::pair<hipEvent_t, int>> marks;
};

namespace {

int bss_check_shape(const etd_bss* h, int J, int C, long long N, int track) {
  const int L = h->cfg.filters_len;
  if (J < 1 || J > BSS_MAX_SOURCES) ETD_FAIL(ETD_EINVAL, "bss: track %d has %d sources (need 1 .. %d)", track, J, BSS_MAX_SOURCES);
  if (C < 1 || C > BSS_MAX_CHANNELS) ETD_FAIL(ETD_EINVAL, "bss: track %d has %d channels (need 1 or 2)", track, C);
  if (N < L) ETD_FAIL(ETD_EINVAL, "bss: track %d has N = %lld samples, below filters_len = %d", track, N, L);
  if (N > (1LL << 31) - 1 - BSS_SLICE) ETD_FAIL(ETD_EINVAL, "bss: track %d has N = %lld samples (above 2^31 - 1 - %d)", track, N, BSS_SLICE);
  if ((long long)J * C * L > BSS_MAX_ORDER) ETD_FAIL(ETD_EINVAL, "bss: track %d: S L = %lld is above %d", track, (long long)J * C * L, BSS_MAX_ORDER);
  return ETD_OK;
}

int bss_num_windows(const etd_bss* h, long long N) {
  return N < h->cfg.window ? 1 : (int)((N - h->cfg.window + h->cfg.hop) / h->cfg.hop);
}

BssLayout bss_layout(const etd_bss* h, int J, int C, long long N) {
  BssLayout y;
  const long long S = (long long)J * C, L = h->cfg.filters_len, n = S * L, nj = C * L;
  const int nwin = bss_num_windows(h, N);
  long long a, b;
  bss_window(nwin - 1, nwin, h->cfg.window, h->cfg.hop, N, &a, &b);
  long long longest = b - a;
  if (nwin > 1 && h->cfg.window > longest) longest = h->cfg.window;
  y.wout_max = (int)(longest + L - 1);
  y.n_slices = (int)((N + BSS_SLICE - 1) / BSS_SLICE);
  y.NC = 2 * S <= 16 ? 16 : 32;
  WsCursor c;
  y.part = c.take(8LL * y.n_slices * 2 * S * L * S);
  y.r = c.take(8 * S * S * L);
  y.d = c.take(8 * S * S * L);
  y.G = c.take(8 * n * n);
  y.Gj = c.take(8 * nj * nj);
  y.DmA = c.take(8 * n * 16);
  y.DmB = c.take(8 * J * nj * 16);
  y.DmR = c.take(8 * n * 16);
  y.F = c.take(8 * n * y.NC);
  y.P = c.off;
  y.bytes_fixed = c.off;
  y.per_window = ws_align(8LL * y.wout_max * y.NC);
  y.bytes_min = y.bytes_fixed + y.per_window;
  return y;
}

int bss_grow(etd_bss* h, long long bytes, hipStream_t st) {
  if (bytes <= h->ws_bytes) return ETD_OK;
  HIP_TRY(hipStreamSynchronize(st));
  if (h->ws) { (void)hipDeviceSynchronize(); (void)hipFree(h->ws); h->ws = nullptr; h->ws_bytes = 0; }
  HIP_TRY(hipMalloc(&h->ws, (size_t)bytes + 256));
  h->ws_bytes = bytes;
  return ETD_OK;
}

void bss_mark(etd_bss* h, int stage, hipStream_t st) {
  if (!h->timing) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, st);
  h->marks.push_back({e, stage});
}
void bss_collect(etd_bss* h) {
  if (!h->timing || h->marks.empty()) return;
  (void)hipEventSynchronize(h->marks.back().first);
  for (size_t i = 1; i < h->marks.size(); ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->marks[i - 1].first, h->marks[i].first);
    if (h->marks[i].second >= 0) h->stage_ms[h->marks[i].second] += ms;
  }
  for (auto& m : h->marks) (void)hipEventDestroy(m.first);
  h->marks.clear();
}

BssTrack bss_track(const etd_bss* h, const float* ref, const float* est, int J, int C, long long N) {
  BssTrack t;
  t.ref = ref; t.est = est; t.J = J; t.C = C; t.S = J * C; t.L = h->cfg.filters_len; t.N = N;
  t.window = h->cfg.window; t.hop = h->cfg.hop; t.nwin = bss_num_windows(h, N);
  return t;
}

// stage 1 -> r, d in the workspace
void bss_corr(etd_bss* h, const BssTrack& t, const BssLayout& y, hipStream_t st) {
  char* ws = (char*)h->ws;
  bss_mark(h, -1, st);
  hipLaunchKernelGGL(k_bss_corr, dim3((unsigned)y.n_slices, (unsigned)(2 * t.S), blocks(t.L, BSS_LAGS_PER_WG)), dim3(256), 0, st, t, (double*)(ws + y.part));
  hipLaunchKernelGGL(k_bss_corr_join, dim3(blocks(2LL * t.S * t.L * t.S, 256)), dim3(256), 0, st, (const double*)(ws + y.part), y.n_slices, t.S, t.L,
                     (double*)(ws + y.r), (double*)(ws + y.d));
  bss_mark(h, 0, st);
}

// Cholesky of G [n][n] (n a multiple of 16) in place, then the substitutions of Dm [n][16]
template <class Src>
void bss_chol_solve(etd_bss* h, double* G, int n, double* Dm, double* DmR, const Src& src, int* status, hipStream_t st) {
  for (int k0 = 0; k0 < n; k0 += BSS_NB) {
    hipLaunchKernelGGL(k_bss_potrf16, dim3(1), dim3(256), 0, st, G, n, k0, status);
    const int m = n - k0 - BSS_NB;
    if (m > 0) {
      hipLaunchKernelGGL(k_bss_trsm, dim3(blocks(m, 256)), dim3(256), 0, st, G, n, n, k0);
      hipLaunchKernelGGL(k_bss_syrk, dim3(blocks(m / 16, 4), (unsigned)(m / 16)), dim3(256), 0, st, G, n, k0, m / 16);
    }
  }
  bss_mark(h, 1, st);
  hipLaunchKernelGGL(k_bss_subst, dim3(1), dim3(1024), 0, st, (const double*)G, n, n, Dm);
  // one step of iterative refinement on the compensated residual
  hipLaunchKernelGGL(k_bss_residual<Src>, dim3(blocks(n * 16, 256)), dim3(256), 0, st, src, (const double*)Dm, DmR);
  hipLaunchKernelGGL(k_bss_subst, dim3(1), dim3(1024), 0, st, (const double*)G, n, n, DmR);
  hipLaunchKernelGGL(k_bss_add, dim3(blocks(n * 16, 256)), dim3(256), 0, st, Dm, (const double*)DmR, n * 16);
  bss_mark(h, 2, st);
}

// stage 2: r, d -> DmA, DmB, F
void bss_filters(etd_bss* h, const BssTrack& t, const BssLayout& y, int* status, hipStream_t st) {
  char* ws = (char*)h->ws;
  const double *r = (const double*)(ws + y.r), *d = (const double*)(ws + y.d);
  double *G = (double*)(ws + y.G), *Gj = (double*)(ws + y.Gj), *DmA = (double*)(ws + y.DmA), *DmB = (double*)(ws + y.DmB);
  const int n = t.S * t.L, nj = t.C * t.L;
  bss_mark(h, -1, st);
  hipLaunchKernelGGL(k_bss_gram, dim3(blocks((long long)n * n, 256)), dim3(256), 0, st, r, t.S, t.L, 0, t.S, G);
  hipLaunchKernelGGL(k_bss_rhs, dim3(blocks(n * 16, 256)), dim3(256), 0, st, d, t.S, t.L, 0, t.S, 0, t.S, DmA);
  bss_mark(h, -1, st);
  bss_chol_solve(h, G, n, DmA, (double*)(ws + y.DmR), BssFromCorr{r, d, t.S, t.L, 0, t.S, 0, t.S}, status, st);
  for (int j = 0; j < t.J; ++j) {
    double* Dj = DmB + (long long)j * nj * 16;
    hipLaunchKernelGGL(k_bss_gram, dim3(blocks((long long)nj * nj, 256)), dim3(256), 0, st, r, t.S, t.L, j * t.C, t.C, Gj);
    hipLaunchKernelGGL(k_bss_rhs, dim3(blocks(nj * 16, 256)), dim3(256), 0, st, d, t.S, t.L, j * t.C, t.C, j * t.C, t.C, Dj);
    bss_mark(h, -1, st);
    bss_chol_solve(h, Gj, nj, Dj, (double*)(ws + y.DmR), BssFromCorr{r, d, t.S, t.L, j * t.C, t.C, j * t.C, t.C}, status, st);
  }
  hipLaunchKernelGGL(k_bss_pack, dim3(blocks((long long)n * y.NC, 256)), dim3(256), 0, st, (const double*)DmA, (const double*)DmB, t.J, t.C, t.L, y.NC, (double*)(ws + y.F));
}

void bss_project(etd_bss* h, const BssTrack& t, const BssLayout& y, int w_first, int nw, hipStream_t st) {
  char* ws = (char*)h->ws;
  hipLaunchKernelGGL(k_bss_project, dim3(blocks(y.wout_max, BSS_ROWS_PER_WG), (unsigned)nw), dim3(256), (size_t)t.S * (BSS_ROWS_PER_WG + t.L) * sizeof(float), st, t,
                     (const double*)(ws + y.F), y.NC, w_first, y.wout_max, (double*)(ws + y.P));
}

// stages 3 .. 5: windows in batches of what the workspace holds behind the fixed part
void bss_windows(etd_bss* h, const BssTrack& t, const BssLayout& y, double* E, int* silent, const int* status, hipStream_t st) {
  char* ws = (char*)h->ws;
  hipLaunchKernelGGL(k_bss_silent, dim3((unsigned)t.nwin), dim3(256), 0, st, t, silent);
  long long cap = (h->ws_bytes - y.bytes_fixed) / y.per_window;
  if (cap > 4096) cap = 4096;
  for (int w0 = 0; w0 < t.nwin; w0 += (int)cap) {
    const int nw = t.nwin - w0 < cap ? t.nwin - w0 : (int)cap;
    bss_mark(h, -1, st);
    bss_project(h, t, y, w0, nw, st);
    bss_mark(h, 3, st);
    hipLaunchKernelGGL(k_bss_energy, dim3((unsigned)t.J, (unsigned)nw), dim3(256), 0, st, t, (const double*)(ws + y.P), y.NC, w0, y.wout_max, (const int*)silent, status, E);
    bss_mark(h, 4, st);
  }
}

int bss_prepare(etd_bss* h, const char* who, int J, int C, long long N, BssLayout* y, hipStream_t st) {
  ETD_TRY(bss_check_shape(h, J, C, N, 0));
  *y = bss_layout(h, J, C, N);
  if (y->bytes_min > h->budget) ETD_FAIL(ETD_EINVAL, "%s: the track needs %lld bytes of workspace, the budget is %lld", who, y->bytes_min, h->budget);
  return bss_grow(h, y->bytes_min, st);
}

}  // namespace

extern "C" int etd_bss_create(const etd_bss_cfg* cfg, etd_bss** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "bss_create: null argument");
  ETD_CHECK_CFG(cfg, etd_bss_cfg, "bss_create");
  if (cfg->filters_len < 16 || cfg->filters_len > BSS_MAX_L || cfg->filters_len % 16)
    ETD_FAIL(ETD_EINVAL, "bss_create: filters_len = %d (need a multiple of 16 in 16 .. %d)", cfg->filters_len, BSS_MAX_L);
  if (cfg->window < cfg->filters_len) ETD_FAIL(ETD_EINVAL, "bss_create: window = %d is below filters_len = %d", cfg->window, cfg->filters_len);
  if (cfg->hop < 1 || cfg->hop > cfg->window) ETD_FAIL(ETD_EINVAL, "bss_create: hop = %d (need 1 .. window = %d)", cfg->hop, cfg->window);
  if (cfg->workspace_bytes < 0) ETD_FAIL(ETD_EINVAL, "bss_create: workspace_bytes = %lld", cfg->workspace_bytes);
  etd_bss* h = new etd_bss();
  h->cfg = *cfg;
  h->budget = cfg->workspace_bytes ? cfg->workspace_bytes : (4LL << 30);
  *out = h;
  return ETD_OK;
}

extern "C" void etd_bss_destroy(etd_bss* h) {
  if (!h) return;
  if (h->ws) { (void)hipDeviceSynchronize(); (void)hipFree(h->ws); }
  delete h;
}

extern "C" long long etd_bss_num_windows(const etd_bss* h, long long N) {
  if (!h || N < 1) { g_etd_err = "bss_num_windows: null handle or N < 1"; return ETD_EINVAL; }
  return bss_num_windows(h, N);
}

extern "C" long long etd_bss_workspace_bytes(const etd_bss* h, int J, int C, long long N) {
  if (!h) { g_etd_err = "bss_workspace_bytes: null handle"; return ETD_EINVAL; }
  const int rc = bss_check_shape(h, J, C, N, 0);
  if (rc != ETD_OK) return rc;
  return bss_layout(h, J, C, N).bytes_min;
}

extern "C" int etd_bss_run(etd_bss* h, int n_tracks, const float* const* ref_ptrs, const float* const* est_ptrs, const int32_t* J_host, const int32_t* C_host,
                           const int64_t* N_host, double* const* E_ptrs, int32_t* const* silent_ptrs, int32_t* status_dev, void* stream) {
  if (!h || !ref_ptrs || !est_ptrs || !J_host || !C_host || !N_host || !E_ptrs || !silent_ptrs || !status_dev) ETD_FAIL(ETD_EINVAL, "bss_run: null argument");
  if (n_tracks < 1) ETD_FAIL(ETD_EINVAL, "bss_run: %d tracks", n_tracks);
  long long need = 0, want = 0;
  std::vector<BssLayout> lay((size_t)n_tracks);
  for (int b = 0; b < n_tracks; ++b) {
    if (!ref_ptrs[b] || !est_ptrs[b] || !E_ptrs[b] || !silent_ptrs[b]) ETD_FAIL(ETD_EINVAL, "bss_run: track %d: null pointer", b);
    ETD_TRY(bss_check_shape(h, J_host[b], C_host[b], N_host[b], b));
    lay[b] = bss_layout(h, J_host[b], C_host[b], N_host[b]);
    if (lay[b].bytes_min > h->budget)
      ETD_FAIL(ETD_EINVAL, "bss_run: track %d needs %lld bytes of workspace, the budget is %lld", b, lay[b].bytes_min, h->budget);
    if (lay[b].bytes_min > need) need = lay[b].bytes_min;
    long long all = lay[b].bytes_fixed + lay[b].per_window * bss_num_windows(h, N_host[b]);
    if (all > h->budget) all = h->budget;
    if (all > want) want = all;
  }
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(bss_grow(h, want > need ? want : need, st));
  for (int k = 0; k < 5; ++k) h->stage_ms[k] = 0.0;
  for (int b = 0; b < n_tracks; ++b) {
    const BssTrack t = bss_track(h, ref_ptrs[b], est_ptrs[b], J_host[b], C_host[b], N_host[b]);
    HIP_TRY(hipMemsetAsync(status_dev + b, 0, sizeof(int32_t), st));
    bss_corr(h, t, lay[b], st);
    bss_filters(h, t, lay[b], status_dev + b, st);
    bss_windows(h, t, lay[b], E_ptrs[b], silent_ptrs[b], status_dev + b, st);
    HIP_TRY(hipGetLastError());
  }
  bss_collect(h);
  return ETD_OK;
}

// ================================================================================================================ debug taps (include/etude_hip_debug.h)
extern "C" int etd_bss_debug_timing(etd_bss* h, int on, double* stage_ms5) {
  if (!h) ETD_FAIL(ETD_EINVAL, "bss_debug_timing: null handle");
  h->timing = on != 0;
  if (stage_ms5)
    for (int k = 0; k < 5; ++k) stage_ms5[k] = h->stage_ms[k];
  return ETD_OK;
}

extern "C" int etd_bss_debug_corr(etd_bss* h, const float* ref_dev, const float* est_dev, int J, int C, long long N, double* r_dev, double* d_dev, void* stream) {
  if (!h || !ref_dev || !est_dev || !r_dev || !d_dev) ETD_FAIL(ETD_EINVAL, "bss_debug_corr: null argument");
  hipStream_t st = (hipStream_t)stream;
  BssLayout y;
  ETD_TRY(bss_prepare(h, "bss_debug_corr", J, C, N, &y, st));
  const BssTrack t = bss_track(h, ref_dev, est_dev, J, C, N);
  bss_corr(h, t, y, st);
  const size_t nb = 8ull * t.S * t.S * t.L;
  HIP_TRY(hipMemcpyAsync(r_dev, (char*)h->ws + y.r, nb, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_dev, (char*)h->ws + y.d, nb, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_bss_debug_solve(etd_bss* h, const double* G_dev, const double* rhs_dev, int n, int m, double* x_dev, int32_t* status_dev, void* stream) {
  if (!h || !G_dev || !rhs_dev || !x_dev || !status_dev) ETD_FAIL(ETD_EINVAL, "bss_debug_solve: null argument");
  if (n < 1 || n > BSS_MAX_ORDER || m < 1 || m > 16) ETD_FAIL(ETD_EINVAL, "bss_debug_solve: n = %d, m = %d (need 1 .. %d and 1 .. 16)", n, m, BSS_MAX_ORDER);
  hipStream_t st = (hipStream_t)stream;
  const int np = (n + 15) / 16 * 16;
  WsCursor c;
  const long long oG = c.take(8LL * np * np), oD = c.take(8LL * np * 16), oR = c.take(8LL * np * 16);
  if (c.off > h->budget) ETD_FAIL(ETD_EINVAL, "bss_debug_solve: needs %lld bytes of workspace, the budget is %lld", c.off, h->budget);
  ETD_TRY(bss_grow(h, c.off, st));
  double *G = (double*)((char*)h->ws + oG), *Dm = (double*)((char*)h->ws + oD);
  HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_bss_pad_matrix, dim3(blocks((long long)np * np, 256)), dim3(256), 0, st, G_dev, n, np, G);
  hipLaunchKernelGGL(k_bss_pad_rhs, dim3(blocks(np * 16, 256)), dim3(256), 0, st, rhs_dev, n, m, np, Dm);
  bss_chol_solve(h, G, np, Dm, (double*)((char*)h->ws + oR), BssFromMatrix{G_dev, rhs_dev, n, m, np}, status_dev, st);
  hipLaunchKernelGGL(k_bss_take_cols, dim3(blocks((long long)n * m, 256)), dim3(256), 0, st, (const double*)Dm, n, m, x_dev);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_bss_debug_filters(etd_bss* h, const float* ref_dev, const float* est_dev, int J, int C, long long N, double* A_dev, double* B_dev,
                                     int32_t* status_dev, void* stream) {
  if (!h || !ref_dev || !est_dev || !A_dev || !B_dev || !status_dev) ETD_FAIL(ETD_EINVAL, "bss_debug_filters: null argument");
  hipStream_t st = (hipStream_t)stream;
  BssLayout y;
  ETD_TRY(bss_prepare(h, "bss_debug_filters", J, C, N, &y, st));
  const BssTrack t = bss_track(h, ref_dev, est_dev, J, C, N);
  HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int32_t), st));
  bss_corr(h, t, y, st);
  bss_filters(h, t, y, status_dev, st);
  const int n = t.S * t.L, nj = t.C * t.L;
  hipLaunchKernelGGL(k_bss_take_cols, dim3(blocks((long long)n * t.S, 256)), dim3(256), 0, st, (const double*)((char*)h->ws + y.DmA), n, t.S, A_dev);
  hipLaunchKernelGGL(k_bss_take_cols, dim3(blocks((long long)t.J * nj * t.C, 256)), dim3(256), 0, st, (const double*)((char*)h->ws + y.DmB), t.J * nj, t.C, B_dev);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_bss_debug_project(etd_bss* h, const float* ref_dev, int J, int C, long long N, int window_index, const double* A_dev, const double* B_dev,
                                     double* ps_dev, double* pa_dev, void* stream) {
  if (!h || !ref_dev || !A_dev || !B_dev || !ps_dev || !pa_dev) ETD_FAIL(ETD_EINVAL, "bss_debug_project: null argument");
  hipStream_t st = (hipStream_t)stream;
  BssLayout y;
  ETD_TRY(bss_prepare(h, "bss_debug_project", J, C, N, &y, st));
  const BssTrack t = bss_track(h, ref_dev, ref_dev, J, C, N);
  if (window_index < 0 || window_index >= t.nwin) ETD_FAIL(ETD_EINVAL, "bss_debug_project: window %d of %d", window_index, t.nwin);
  char* ws = (char*)h->ws;
  const int n = t.S * t.L, nj = t.C * t.L;
  hipLaunchKernelGGL(k_bss_put_cols, dim3(blocks(n * 16, 256)), dim3(256), 0, st, A_dev, n, t.S, (double*)(ws + y.DmA));
  hipLaunchKernelGGL(k_bss_put_cols, dim3(blocks(t.J * nj * 16, 256)), dim3(256), 0, st, B_dev, t.J * nj, t.C, (double*)(ws + y.DmB));
  hipLaunchKernelGGL(k_bss_pack, dim3(blocks((long long)n * y.NC, 256)), dim3(256), 0, st, (const double*)(ws + y.DmA), (const double*)(ws + y.DmB), t.J, t.C, t.L, y.NC,
                     (double*)(ws + y.F));
  bss_project(h, t, y, window_index, 1, st);
  long long a, b;
  bss_window(window_index, t.nwin, t.window, t.hop, t.N, &a, &b);
  const long long Wout = b - a + t.L - 1;
  hipLaunchKernelGGL(k_bss_unpack_proj, dim3(blocks(t.S * Wout, 256)), dim3(256), 0, st, (const double*)(ws + y.P), t.S, y.NC, Wout, ps_dev, pa_dev);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
