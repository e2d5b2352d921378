// Exact full-resolution DTW between a cover and its origin (DESIGN.md 4e is the contract): the warping path, the optimal transposition and D[-1,-1].
// Stands in for AudioAligner._compute_warping_path behind the feature extraction (etude/data/aligner.py:106-133: quantized_chroma_to_CENS,
// compute_optimal_chroma_shift, sync_via_mrmsdtw, make_path_strictly_monotonic).
//
// A ragged batch of pairs runs in five launches, whatever the number of pairs:
//   k_dtw_prep      one thread per frame: L2-normalised chroma and DLNCO of a frame side by side, [N][24] (one 96-byte read per DTW column)
//   k_dtw_cens      one thread per (CENS frame, pitch): Hann smoothing, decimation, normalisation -> [M][12]
//   k_dtw<false>    one wave per (pair, shift): the 12 small path-free DTWs of the transposition search; only D[-1,-1] is kept
//   k_dtw_argmin    one thread per pair: the first minimum of the 12 totals -> `opt` in the pair table (no host round trip)
//   k_dtw<true>     one wave per pair: the final DTW with shift `opt`, 2-bit backpointers, backtracking and the strictly monotonic path
//
// Inside a problem (k_dtw): a skewed wavefront over row blocks of DTW_B rows.  Lane t owns DTW_R consecutive rows, whose features sit in registers, and at step s
// works on column s - t.  The D of its last row goes to lane t + 1 by a lane move (ds_bpermute: the LDS pipe, no LDS memory); a workgroup is ONE wave, so a step
// has no barrier, and a problem never waits for another workgroup.  Between row blocks the block's last D row (fp64, N2 values) travels through a workspace row: lane 63
// writes column j 63 steps after lane 0 of the same block read it.  Nothing wider than that row is stored of D.
// A shift s of sequence 2 is applied to sequence 1's rows when a lane loads them: <c1, roll(c2, s)> = sum_m c1[(m + s) % 12] c2[m], summed in the order of m.
#include "dtw.h"
#include "prof.h"

#include <cmath>

namespace {

struct DtwW { double w0, w1, w2; float alpha, oma; };

// The cost of one cell, fp32, in one fixed order; the ONLY place a cost is formed (k_dtw and the debug hook share it).  a: the row's features, rotated by the shift.
template <bool FINAL>
__device__ __forceinline__ float dtw_cost(const float* a, const float* b, float alpha, float oma) {
#pragma clang fp contract(off)
  float dot = 0.f;
#pragma unroll
  for (int m = 0; m < 12; ++m) dot = fmaf(a[m], b[m], dot);
  if (!FINAL) return 1.f - dot;
  float ss = 0.f;
#pragma unroll
  for (int m = 0; m < 12; ++m) {
    const float d = a[12 + m] - b[12 + m];
    ss = fmaf(d, d, ss);
  }
  const float t1 = alpha * (2.f - dot);
  const float t2 = oma * sqrtf(ss);
  return t1 + t2;
}

template <int NF>
__device__ __forceinline__ void dtw_load_col(const float* p, float* v) {
  const float4* q = (const float4*)p;
#pragma unroll
  for (int k = 0; k < NF / 4; ++k) {
    const float4 x = q[k];
    v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
  }
}

// features of row i of sequence 1, rotated by shift s (zeros for a row past the end: its cells are computed and never used)
template <int NF>
__device__ __forceinline__ void dtw_load_row(const float* F1, long long i, bool valid, int s, float* a) {
#pragma unroll
  for (int m = 0; m < 12; ++m) {
    int k = m + s;
    if (k >= 12) k -= 12;
    a[m] = valid ? F1[i * NF + k] : 0.f;
    if (NF == 24) a[12 + m] = valid ? F1[i * NF + 12 + k] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_dtw_prep(const DtwPair* __restrict__ tab, unsigned char* __restrict__ ws, float thr) {
  const DtwPair P = tab[blockIdx.y >> 1];
  const int side = blockIdx.y & 1;
  const long long N = side ? P.N2 : P.N1;
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* c = side ? P.c2 : P.c1;
  const float* o = side ? P.o2 : P.o1;
  float* f = (float*)(ws + (side ? P.off_f2 : P.off_f1)) + n * 24;
  float v[12], ss = 0.f;
#pragma unroll
  for (int m = 0; m < 12; ++m) {
    v[m] = c[m * N + n];
    ss = fmaf(v[m], v[m], ss);
  }
  const float nrm = sqrtf(ss);
#pragma unroll
  for (int m = 0; m < 12; ++m) f[m] = nrm < thr ? 0.28867513459481287f : v[m] / nrm;          // 1 / sqrt(12)
#pragma unroll
  for (int m = 0; m < 12; ++m) f[12 + m] = o[m * N + n];
}

#define DTW_CENS_FRAMES 16
__global__ __launch_bounds__(12 * DTW_CENS_FRAMES) void k_dtw_cens(const DtwPair* __restrict__ tab, unsigned char* __restrict__ ws, const float* __restrict__ win, int wlen,
                                                                   int dec, float thr) {
  __shared__ float sm[DTW_CENS_FRAMES][12];
  const DtwPair P = tab[blockIdx.y >> 1];
  const int side = blockIdx.y & 1, pch = threadIdx.x, fy = threadIdx.y;
  const long long N = side ? P.N2 : P.N1, M = side ? P.M2 : P.M1;
  const long long m = (long long)blockIdx.x * DTW_CENS_FRAMES + fy;
  const float* c = (side ? P.c2 : P.c1) + pch * N;
  float acc = 0.f;
  if (m < M) {
    const long long i0 = m * dec - (wlen - 1) / 2;
    for (int k = 0; k < wlen; ++k) {
      const long long i = i0 + k;
      if (i >= 0 && i < N) acc = fmaf(win[k], c[i], acc);
    }
  }
  sm[fy][pch] = acc;
  __syncthreads();
  if (m >= M) return;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 12; ++q) ss = fmaf(sm[fy][q], sm[fy][q], ss);
  const float nrm = sqrtf(ss);
  float* f = (float*)(ws + (side ? P.off_cens2 : P.off_cens1));
  f[m * 12 + pch] = nrm < thr ? 0.28867513459481287f : acc / nrm;
}

__global__ void k_dtw_argmin(DtwPair* tab, const unsigned char* __restrict__ ws, int n_pairs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const double* tot = (const double*)(ws + tab[p].off_totals);
  int best = 0;
  double bv = tot[0];
  for (int s = 1; s < 12; ++s)
    if (tot[s] < bv) { bv = tot[s]; best = s; }      // the first minimum wins
  tab[p].opt = best;
}

template <bool FINAL>
__global__ __launch_bounds__(DTW_LANES) void k_dtw(const DtwPair* tab, const DtwW W, unsigned char* ws, int* res) {
  constexpr int NF = FINAL ? 24 : 12;
  constexpr int R = DTW_R;
  const int t = threadIdx.x;
  const int p = FINAL ? (int)blockIdx.x : (int)(blockIdx.x / 12);
  const DtwPair P = tab[p];
  const int s = FINAL ? P.opt : (int)(blockIdx.x % 12);
  const int N1 = FINAL ? P.N1 : P.M1, N2 = FINAL ? P.N2 : P.M2;
  const float* F1 = (const float*)(ws + (FINAL ? P.off_f1 : P.off_cens1));
  const float* F2 = (const float*)(ws + (FINAL ? P.off_f2 : P.off_cens2));
  double* top = (double*)(ws + (FINAL ? P.off_top : P.off_top12 + s * P.top12_stride));
  double* total = FINAL ? (double*)(res + P.res_off + 4) : (double*)(ws + P.off_totals) + s;
  unsigned* bp = (unsigned*)(ws + P.off_bp);
  const long long stride = P.bp_stride;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);

  for (int i0 = 0; i0 < N1; i0 += DTW_B) {
    const int rows = N1 - i0 < DTW_B ? N1 - i0 : DTW_B;
    const int nl = (rows + R - 1) / R;                  // lanes with a row
    const bool first = i0 == 0, lastblk = i0 + DTW_B >= N1;
    const int ibase = i0 + t * R;
    float a[R][NF];
#pragma unroll
    for (int q = 0; q < R; ++q) dtw_load_row<NF>(F1, ibase + q, ibase + q < N1, s, a[q]);
    double left[R];
    unsigned word[R];
#pragma unroll
    for (int q = 0; q < R; ++q) { left[q] = INF; word[q] = 0u; }
    double upin = INF;      // D[ibase - 1][j] of this step's column j: from lane t - 1 (lane 0: the previous block's row)
    double upprev = INF;    // D[ibase - 1][j - 1]
    float cur[NF], nxt[NF];
#pragma unroll
    for (int m = 0; m < NF; ++m) { cur[m] = 0.f; nxt[m] = 0.f; }
    double topcur = INF;
    if (t == 0) {
      dtw_load_col<NF>(F2, cur);
      if (!first) topcur = top[0];
    }
    const int nsteps = N2 + nl - 1;
    int j = -t;
    for (int st = 0; st < nsteps; ++st, ++j) {
      const bool act = t < nl && j >= 0 && j < N2;
      const bool pre = t < nl && j + 1 >= 0 && j + 1 < N2;
      double topnxt = INF;
      if (pre) {
        dtw_load_col<NF>(F2 + (long long)(j + 1) * NF, nxt);
        if (t == 0 && !first) topnxt = top[j + 1];
      }
      double lastD = INF;
      if (act) {
        const double upfirst = t == 0 ? topcur : upin;
        double up = upfirst, dg = upprev;
        const bool origin = first && t == 0 && j == 0;
#pragma unroll
        for (int q = 0; q < R; ++q) {
          const double cd = (double)dtw_cost<FINAL>(a[q], cur, W.alpha, W.oma);
          const double a0 = up + W.w0 * cd, a1 = left[q] + W.w1 * cd, a2 = dg + W.w2 * cd;
          double d = a0;
          unsigned k = 0u;
          if (a1 < d) { d = a1; k = 1u; }
          if (a2 < d) { d = a2; k = 2u; }
          if (q == 0 && origin) d = cd;
          dg = left[q];
          left[q] = d;
          up = d;
          if (FINAL) word[q] |= k << (2 * (j & (DTW_BPW - 1)));
        }
        upprev = upfirst;
        lastD = left[R - 1];
        if (FINAL && ((j & (DTW_BPW - 1)) == DTW_BPW - 1 || j == N2 - 1)) {
#pragma unroll
          for (int q = 0; q < R; ++q) {
            if (ibase + q < N1) bp[(long long)(ibase + q) * stride + (j >> 4)] = word[q];
            word[q] = 0u;
          }
        }
        if (!lastblk && t == DTW_LANES - 1) top[j] = lastD;
        if (lastblk && j == N2 - 1) {
#pragma unroll
          for (int q = 0; q < R; ++q)
            if (ibase + q == N1 - 1) *total = left[q];
        }
      }
      upin = __shfl_up(lastD, 1, DTW_LANES);
#pragma unroll
      for (int m = 0; m < NF; ++m) cur[m] = nxt[m];
      topcur = topnxt;
    }
    __threadfence_block();      // the row lane 63 wrote is read by lane 0 of the next block
  }

  if (FINAL) {
    // ---- backtracking: (i, j) is the same in every lane; the lanes hold the backpointer words of 64 rows at the current word column, so one load serves ~16 steps
    __syncthreads();
    int* tmp = (int*)(ws + P.off_tmp);
    int* rawp = (int*)(ws + P.off_raw);
    int nraw = 1;
    if (t == 0) { rawp[0] = N1 - 1; rawp[1] = N2 - 1; }
    int i = N1 - 1, j = N2 - 1, cnt = 0, fi = 0, fj = 0;
    int base = -1, cjw = -1;
    unsigned cache = 0u;
    while (i > 0 || j > 0) {
      const int jw = j >> 4;
      if (jw != cjw || i > base || base - i >= DTW_LANES) {
        base = i; cjw = jw;
        cache = base - t >= 0 ? bp[(long long)(base - t) * stride + jw] : 0u;
      }
      const unsigned w = (unsigned)__shfl((int)cache, base - i, DTW_LANES);
      unsigned k = (w >> (2 * (j & (DTW_BPW - 1)))) & 3u;
      if (i == 0) k = 1u; else if (j == 0) k = 0u;      // (what the recursion stored there anyway: the walk cannot leave the matrix)
      // strictly monotonic path: an interior point stays when the step into it was the diagonal one -- both coordinates above those of its predecessor
      if (k >= 2u && !(i == N1 - 1 && j == N2 - 1)) {
        if (cnt == 0) { fi = i; fj = j; }
        if (t == 0) { tmp[2 * cnt] = i; tmp[2 * cnt + 1] = j; }
        ++cnt;
      }
      if (k == 0u) --i; else if (k == 1u) --j; else { --i; --j; }
      if (t == 0) { rawp[2 * nraw] = i; rawp[2 * nraw + 1] = j; }
      ++nraw;
    }
    // ... and the kept point before the last one goes when the last point is not above it in both coordinates (the first and the last point always stay)
    const int drop = cnt > 0 && !(fi < N1 - 1 && fj < N2 - 1) ? 1 : 0;
    const int kept = cnt - drop;
    const bool single = N1 == 1 && N2 == 1;
    const int L = single ? 1 : kept + 2;
    int* out = res + P.res_off;
    __threadfence_block();
    __syncthreads();
    for (int k = t; k < kept; k += DTW_LANES) {
      out[DTW_HDR + 1 + k] = tmp[2 * (cnt - 1 - k)];
      out[DTW_HDR + P.cap + 1 + k] = tmp[2 * (cnt - 1 - k) + 1];
    }
    if (t == 0) {
      out[DTW_HDR] = 0; out[DTW_HDR + P.cap] = 0;
      if (!single) { out[DTW_HDR + L - 1] = N1 - 1; out[DTW_HDR + P.cap + L - 1] = N2 - 1; }
      int ps = (12 - s) % 12;
      if (ps > 6) ps -= 12;
      out[0] = L; out[1] = s; out[2] = ps; out[3] = nraw; out[6] = 0; out[7] = 0;
    }
  }
}

// test hook: the cost matrix of one pair, through dtw_cost and the loaders of k_dtw
__global__ __launch_bounds__(256) void k_dtw_debug_cost(const DtwPair* __restrict__ tab, const DtwW W, const unsigned char* __restrict__ ws, int s, float* __restrict__ C) {
  const DtwPair P = tab[0];
  const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (long long)P.N1 * P.N2) return;
  const long long i = cell / P.N2, j = cell % P.N2;
  float a[24], b[24];
  dtw_load_row<24>((const float*)(ws + P.off_f1), i, true, s, a);
  dtw_load_col<24>((const float*)(ws + P.off_f2) + j * 24, b);
  C[cell] = dtw_cost<true>(a, b, W.alpha, W.oma);
}

long long up256(long long x) { return (x + 255) & ~255LL; }

}  // namespace

struct etd_dtw {
  etd_dtw_cfg cfg;
  std::vector<float> window;
  float* d_window = nullptr;
  DevPool pool;
  std::vector<DtwPair> tab;      // the table of the call in flight (host memory the upload reads)
};

namespace {

// fills tab (when not null), the workspace bytes and the result ints; ETD_EINVAL for a bad shape
int dtw_plan(const etd_dtw* h, int n, const int64_t* N1, const int64_t* N2, std::vector<DtwPair>* tab, long long* ws_bytes, long long* res_ints, int64_t* res_offsets) {
  if (!h || !N1 || !N2) ETD_FAIL(ETD_EINVAL, "dtw: null argument");
  if (n < 1 || n > DTW_MAX_PAIRS) ETD_FAIL(ETD_EINVAL, "dtw: %d pairs in one call (need 1 .. %d)", n, DTW_MAX_PAIRS);
  long long off = up256((long long)n * (long long)sizeof(DtwPair)), r = 0;
  if (tab) tab->assign((size_t)n, DtwPair{});
  for (int p = 0; p < n; ++p) {
    const long long a = N1[p], b = N2[p];
    if (a < 1 || b < 1) ETD_FAIL(ETD_EINVAL, "dtw: pair %d has %lld x %lld frames (need >= 1 on both sides)", p, a, b);
    if (a > DTW_MAX_FRAMES || b > DTW_MAX_FRAMES)
      ETD_FAIL(ETD_EINVAL, "dtw: pair %d has %lld x %lld frames, above the limit of %d per side", p, a, b, DTW_MAX_FRAMES);
    DtwPair P{};
    P.N1 = (int)a; P.N2 = (int)b;
    P.M1 = (int)((a - 1) / h->cfg.cens_decimation + 1); P.M2 = (int)((b - 1) / h->cfg.cens_decimation + 1);
    P.cap = (int)(a < b ? a : b) + 1;
    P.opt = 0;
    P.off_f1 = off; off += up256(96 * a);
    P.off_f2 = off; off += up256(96 * b);
    P.off_cens1 = off; off += up256(48LL * P.M1);
    P.off_cens2 = off; off += up256(48LL * P.M2);
    P.off_top = off; off += up256(8 * b);
    P.top12_stride = up256(8LL * P.M2);
    P.off_top12 = off; off += 12 * P.top12_stride;
    P.off_totals = off; off += up256(96);
    P.bp_stride = (b + DTW_BPW - 1) / DTW_BPW;
    P.off_bp = off; off += up256(4 * a * P.bp_stride);
    P.off_tmp = off; off += up256(8LL * P.cap);
    P.off_raw = off; off += up256(8 * (a + b));
    P.res_off = r; r += DTW_HDR + 2LL * P.cap;
    if (res_offsets) res_offsets[p] = P.res_off;
    if (tab) (*tab)[p] = P;
  }
  *ws_bytes = off; *res_ints = r;
  return ETD_OK;
}

DtwW dtw_weights(const double* w, float alpha) {
  DtwW W;
  W.w0 = w[0]; W.w1 = w[1]; W.w2 = w[2]; W.alpha = alpha; W.oma = 1.f - alpha;
  return W;
}

// the launches of one call; force_shift < 0: the transposition search decides the shift
int dtw_launch(etd_dtw* h, const float* const* ptrs, int n, const int64_t* N1, const int64_t* N2, void* ws_dev, long long ws_bytes, int32_t* res_dev, long long res_ints,
               int force_shift, bool final_dtw, hipStream_t st) {
  if (!h || !ptrs || !ws_dev || !res_dev) ETD_FAIL(ETD_EINVAL, "dtw: null argument");
  long long need_ws = 0, need_res = 0;
  ETD_TRY(dtw_plan(h, n, N1, N2, &h->tab, &need_ws, &need_res, nullptr));
  if (ws_bytes < need_ws) ETD_FAIL(ETD_EINVAL, "dtw: the workspace holds %lld bytes, this call needs %lld (etd_dtw_workspace_bytes)", ws_bytes, need_ws);
  if (res_ints < need_res) ETD_FAIL(ETD_EINVAL, "dtw: the result buffer holds %lld int32, this call needs %lld (etd_dtw_workspace_bytes)", res_ints, need_res);
  if (((uintptr_t)ws_dev & 255) || ((uintptr_t)res_dev & 7)) ETD_FAIL(ETD_EINVAL, "dtw: the workspace must be 256-byte aligned and the result buffer 8-byte aligned");
  long long maxN = 0, maxM = 0;
  for (int p = 0; p < n; ++p) {
    DtwPair& P = h->tab[p];
    for (int k = 0; k < 4; ++k)
      if (!ptrs[4 * p + k]) ETD_FAIL(ETD_EINVAL, "dtw: pair %d has a null feature pointer", p);
    P.c1 = ptrs[4 * p]; P.o1 = ptrs[4 * p + 1]; P.c2 = ptrs[4 * p + 2]; P.o2 = ptrs[4 * p + 3];
    if (force_shift >= 0) P.opt = force_shift;
    const long long mn = P.N1 > P.N2 ? P.N1 : P.N2, mm = P.M1 > P.M2 ? P.M1 : P.M2;
    maxN = mn > maxN ? mn : maxN; maxM = mm > maxM ? mm : maxM;
  }
  if (!h->d_window) ETD_TRY(h->pool.upload(&h->d_window, h->window.data(), h->window.size()));
  unsigned char* ws = (unsigned char*)ws_dev;
  DtwPair* tab = (DtwPair*)ws;
  HIP_TRY(hipMemcpyAsync(tab, h->tab.data(), (size_t)n * sizeof(DtwPair), hipMemcpyHostToDevice, st));
  const etd_dtw_cfg& c = h->cfg;
  double cells = 0, scells = 0, frames = 0;
  for (int p = 0; p < n; ++p) {
    cells += (double)N1[p] * (double)N2[p]; scells += 12.0 * h->tab[p].M1 * h->tab[p].M2; frames += (double)(N1[p] + N2[p]);
  }
  {
    ProfScope ps("k_dtw_prep", st, frames * 40, frames * 192);
    hipLaunchKernelGGL(k_dtw_prep, dim3((unsigned)((maxN + 255) / 256), (unsigned)(2 * n)), dim3(256), 0, st, tab, ws, c.norm_threshold);
  }
  if (force_shift < 0) {
    {
      ProfScope ps("k_dtw_cens", st, frames / c.cens_decimation * 24.0 * c.cens_window, frames * 48);
      hipLaunchKernelGGL(k_dtw_cens, dim3((unsigned)((maxM + DTW_CENS_FRAMES - 1) / DTW_CENS_FRAMES), (unsigned)(2 * n)), dim3(12, DTW_CENS_FRAMES), 0, st, tab, ws,
                         h->d_window, c.cens_window, c.cens_decimation, c.norm_threshold);
    }
    {
      ProfScope ps("k_dtw_shift", st, scells * 34, 0);
      hipLaunchKernelGGL(k_dtw<false>, dim3((unsigned)(12 * n)), dim3(DTW_LANES), 0, st, tab, dtw_weights(c.shift_weights, c.alpha), ws, res_dev);
    }
    hipLaunchKernelGGL(k_dtw_argmin, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tab, ws, n);
  }
  if (final_dtw) {
    ProfScope ps("k_dtw_final", st, cells * 72, cells / 4);
    hipLaunchKernelGGL(k_dtw<true>, dim3((unsigned)n), dim3(DTW_LANES), 0, st, tab, dtw_weights(c.step_weights, c.alpha), ws, res_dev);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

}  // namespace

extern "C" int etd_dtw_create(const etd_dtw_cfg* cfg, etd_dtw** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "dtw_create: null argument");
  ETD_CHECK_CFG(cfg, etd_dtw_cfg, "dtw_create");
  if (cfg->cens_window < 1 || cfg->cens_window > 4095 || !(cfg->cens_window & 1)) ETD_FAIL(ETD_EINVAL, "dtw_create: cens_window = %d must be odd, in 1 .. 4095", cfg->cens_window);
  if (cfg->cens_decimation < 1 || cfg->cens_decimation > 4096) ETD_FAIL(ETD_EINVAL, "dtw_create: cens_decimation = %d must be in 1 .. 4096", cfg->cens_decimation);
  for (int k = 0; k < 3; ++k)
    if (!(cfg->step_weights[k] > 0) || !std::isfinite(cfg->step_weights[k]) || !(cfg->shift_weights[k] > 0) || !std::isfinite(cfg->shift_weights[k]))
      ETD_FAIL(ETD_EINVAL, "dtw_create: step weight %d must be positive and finite", k);
  if (!(cfg->alpha >= 0.f && cfg->alpha <= 1.f)) ETD_FAIL(ETD_EINVAL, "dtw_create: alpha must be in 0 .. 1");
  if (!(cfg->norm_threshold >= 0.f) || !std::isfinite(cfg->norm_threshold)) ETD_FAIL(ETD_EINVAL, "dtw_create: norm_threshold must be finite and >= 0");
  etd_dtw* h = new etd_dtw();
  h->cfg = *cfg;
  // symmetric Hann window scaled to sum 1 (a window of one point is 1)
  const int n = cfg->cens_window;
  std::vector<double> w((size_t)n, 1.0);
  double sum = 0;
  for (int k = 0; k < n; ++k) {
    if (n > 1) w[k] = 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * k / (n - 1));
    sum += w[k];
  }
  h->window.resize((size_t)n);
  for (int k = 0; k < n; ++k) h->window[k] = (float)(w[k] / sum);
  *out = h;
  return ETD_OK;
}

extern "C" void etd_dtw_destroy(etd_dtw* h) {
  if (!h) return;
  if (h->d_window) {
    (void)hipDeviceSynchronize();
    h->pool.free_all();
  }
  delete h;
}

extern "C" int etd_dtw_limits(int* row_block, int* cells_per_word, long long* max_frames, int* max_pairs) {
  if (row_block) *row_block = DTW_B;
  if (cells_per_word) *cells_per_word = DTW_BPW;
  if (max_frames) *max_frames = DTW_MAX_FRAMES;
  if (max_pairs) *max_pairs = DTW_MAX_PAIRS;
  return ETD_OK;
}

extern "C" long long etd_dtw_workspace_bytes(const etd_dtw* h, int n_pairs, const int64_t* N1_host, const int64_t* N2_host, long long* result_ints, int64_t* result_offsets) {
  long long ws = 0, r = 0;
  const int rc = dtw_plan(h, n_pairs, N1_host, N2_host, nullptr, &ws, &r, result_offsets);
  if (rc != ETD_OK) return rc;
  if (result_ints) *result_ints = r;
  return ws;
}

extern "C" int etd_dtw_align(etd_dtw* h, const float* const* feat_ptrs, int n_pairs, const int64_t* N1_host, const int64_t* N2_host, void* workspace_dev,
                             long long workspace_bytes, int32_t* result_dev, long long result_ints, int32_t* result_host, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(dtw_launch(h, feat_ptrs, n_pairs, N1_host, N2_host, workspace_dev, workspace_bytes, result_dev, result_ints, -1, true, st));
  if (result_host) {
    long long ws = 0, r = 0;
    ETD_TRY(dtw_plan(h, n_pairs, N1_host, N2_host, nullptr, &ws, &r, nullptr));
    HIP_TRY(hipMemcpyAsync(result_host, result_dev, (size_t)r * 4, hipMemcpyDeviceToHost, st));      // the one copy to the host: 8 + 2 (min(N1, N2) + 1) ints per pair
  }
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}

namespace {

// one pair with buffers of the hook's own: prep (+ the final DTW with a given shift)
struct DtwScratch {
  void* ws = nullptr; int32_t* res = nullptr; long long ws_bytes = 0, res_ints = 0;
  ~DtwScratch() { if (ws) (void)hipFree(ws); if (res) (void)hipFree(res); }
};

int dtw_debug_run(etd_dtw* h, const float* const* ptrs, long long N1, long long N2, int shift, bool final_dtw, DtwScratch* S) {
  if (!h || !ptrs) ETD_FAIL(ETD_EINVAL, "dtw_debug: null argument");
  if (shift < 0 || shift > 11) ETD_FAIL(ETD_EINVAL, "dtw_debug: shift = %d must be in 0 .. 11", shift);
  const int64_t a = N1, b = N2;
  ETD_TRY(dtw_plan(h, 1, &a, &b, nullptr, &S->ws_bytes, &S->res_ints, nullptr));
  HIP_TRY(hipMalloc(&S->ws, (size_t)S->ws_bytes));
  HIP_TRY(hipMalloc((void**)&S->res, (size_t)S->res_ints * 4));
  ETD_TRY(dtw_launch(h, ptrs, 1, &a, &b, S->ws, S->ws_bytes, S->res, S->res_ints, shift, final_dtw, nullptr));
  return ETD_OK;
}

}  // namespace

extern "C" int etd_dtw_debug_cost(etd_dtw* h, const float* const* feat_ptrs, long long N1, long long N2, int shift, float* cost_dev) {
  if (!cost_dev) ETD_FAIL(ETD_EINVAL, "dtw_debug_cost: null argument");
  if (N1 >= 1 && N2 >= 1 && N1 * N2 > DTW_MAX_DEBUG_CELLS && N1 <= DTW_MAX_FRAMES && N2 <= DTW_MAX_FRAMES)
    ETD_FAIL(ETD_EINVAL, "dtw_debug_cost: %lld x %lld = %lld cells, above the hook's limit of 2^22", N1, N2, N1 * N2);
  DtwScratch S;
  ETD_TRY(dtw_debug_run(h, feat_ptrs, N1, N2, shift, false, &S));
  hipLaunchKernelGGL(k_dtw_debug_cost, dim3((unsigned)((N1 * N2 + 255) / 256)), dim3(256), 0, nullptr, (const DtwPair*)S.ws, dtw_weights(h->cfg.step_weights, h->cfg.alpha),
                     (const unsigned char*)S.ws, shift, cost_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return ETD_OK;
}

extern "C" int etd_dtw_debug_path(etd_dtw* h, const float* const* feat_ptrs, long long N1, long long N2, int shift, int32_t* path_host, long long cap, long long* n_out) {
  if (!path_host || !n_out) ETD_FAIL(ETD_EINVAL, "dtw_debug_path: null argument");
  DtwScratch S;
  ETD_TRY(dtw_debug_run(h, feat_ptrs, N1, N2, shift, true, &S));
  HIP_TRY(hipDeviceSynchronize());
  int32_t n = 0;
  HIP_TRY(hipMemcpy(&n, S.res + 3, 4, hipMemcpyDeviceToHost));
  *n_out = n;
  if (n > cap) ETD_FAIL(ETD_ENOMEM, "dtw_debug_path: the path has %d points, the buffer holds %lld", (int)n, cap);
  HIP_TRY(hipMemcpy(path_host, (const unsigned char*)S.ws + h->tab[0].off_raw, (size_t)n * 8, hipMemcpyDeviceToHost));
  return ETD_OK;
}

extern "C" int etd_dtw_debug_total(etd_dtw* h, const float* const* feat_ptrs, long long N1, long long N2, int shift, double* total_host) {
  if (!total_host) ETD_FAIL(ETD_EINVAL, "dtw_debug_total: null argument");
  DtwScratch S;
  ETD_TRY(dtw_debug_run(h, feat_ptrs, N1, N2, shift, true, &S));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(total_host, S.res + 4, 8, hipMemcpyDeviceToHost));
  return ETD_OK;
}
