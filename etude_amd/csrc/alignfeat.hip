// Alignment features on the GPU: mono audio at 22 050 Hz -> quantised chroma [12][T] and DLNCO [12][T] at 50 Hz, the input of etd_dtw_align (DESIGN.md 4f is the
// contract; modelled on synctoolbox's audio_to_pitch_features / pitch_to_chroma / quantize_chroma / audio_to_pitch_onset_features / pitch_onset_features_to_DLNCO).
//
// The hot path is the bank of 88 zero-phase elliptic band-passes (4 or 5 second-order sections each, fp64 recurrence) over three rate tiers.  A recurrence is sequential
// in time, so its time axis is split EXACTLY: a band's signal is cut into chunks of AF_L samples, and for each direction
//   k_af_iir<.., false>  every chunk runs from the zero state and keeps only its end state e_c            (one lane per chunk, 64 consecutive chunks of a band per wave)
//   k_af_prop            per band, serially over its chunks: s_0 = 0, s_{c+1} = A^L s_c + e_c             (A^L: 12 x 12 fp64 per band, built on the host)
//   k_af_iir<.., true>   every chunk reruns from its true start state s_c and writes the output
// (the cascade is linear in (state, input), so this is the sequential filter in exact arithmetic, with a fixed order of operations).  The backward pass is the same
// three launches over the reversed forward output.  Around them: two decimation launches (481-tap fp32 fmaf chains), pitch energy, chroma, onset novelty, peaks, the
// per-frame chroma-onset sum and one workgroup per song for the DLNCO tail (its maximum over frames is a maximum inside ONE workgroup).  No atomics, no flags, no
// spinning; a song's features depend on its own samples and filter tables alone.
#include "alignfeat.h"
#include "prof.h"

#include <cmath>

namespace {

struct AfArgs {
  const AfSong* tab; int n_songs;
  char* ws;
  const float* fir;                 // [481]
  const double* sos;                // [banks][88][6][6]: b0 b1 b2 1 a1 a2
  const int* nsec;                  // [banks][88]
  const double* apow;               // [banks][88][12][12]
  const double* hann;               // [100] periodic Hann of 100, then [50] of 50
  float* chroma; float* dlnco;
};

__host__ __device__ __forceinline__ int af_tier_of(int b) { return b < AF_B2 ? 2 : (b < AF_B2 + AF_B1 ? 1 : 0); }
__host__ __device__ __forceinline__ int af_d(int tier) { return tier == 0 ? 1 : (tier == 1 ? 5 : 25); }
__host__ __device__ __forceinline__ int af_w(int tier) { return tier == 2 ? 50 : 100; }
// a per-tier field by selects: an index that is not a constant would make the compiler copy the table entry to private memory
__host__ __device__ __forceinline__ long long af_pick(const long long* v, int tier) { return tier == 0 ? v[0] : (tier == 1 ? v[1] : v[2]); }
// elements of a per-band array before band b, v = the per-tier count
__host__ __device__ __forceinline__ long long af_boff(int b, const long long* v) {
  return b < AF_B2 ? (long long)b * v[2] : AF_B2 * v[2] + (b < AF_B2 + AF_B1 ? (long long)(b - AF_B2) * v[1] : AF_B1 * v[1] + (long long)(b - AF_B2 - AF_B1) * v[0]);
}
__host__ __device__ __forceinline__ long long af_btotal(const long long* v) { return AF_B2 * v[2] + AF_B1 * v[1] + AF_B0 * v[0]; }
// the inverse: element i of a per-band array -> (band, index inside the band); i < af_btotal(v)
__device__ __forceinline__ void af_unoff(long long i, const long long* v, int& b, long long& r) {
  const long long t2 = AF_B2 * v[2], t1 = t2 + AF_B1 * v[1];
  if (i < t2) { b = (int)(i / v[2]); r = i - (long long)b * v[2]; }
  else if (i < t1) { const long long l = i - t2; const int k = (int)(l / v[1]); b = AF_B2 + k; r = l - (long long)k * v[1]; }
  else { const long long l = i - t1; const int k = (int)(l / v[0]); b = AF_B2 + AF_B1 + k; r = l - (long long)k * v[0]; }
}
// the frame of novelty index m on a tier: min(T - 1, floor(50 time + 1/2)), time = (m hop + w / 2) / f_tier, as integers: (w (m + 1) 25 d + 11025) / 22050
__host__ __device__ __forceinline__ long long af_frame(long long m, int tier, long long T) {
  const long long f = ((long long)af_w(tier) * 25 * af_d(tier) * (m + 1) + 11025) / 22050;
  return f < T - 1 ? f : T - 1;
}

// ---- decimation by 5: y[m] = sum_n h[n] x[5 m - n], n = -240 .. 240 ascending, zeros outside the signal (a term with a zero sample leaves the chain's value unchanged)
__global__ __launch_bounds__(AF_THREADS) void k_af_decim(const AfArgs a, int tier) {
  const AfSong& sg = a.tab[blockIdx.y];
  const long long nin = af_pick(sg.n, tier - 1), nout = af_pick(sg.n, tier);
  const float* src = tier == 1 ? sg.wav : (const float*)(a.ws + sg.off_x1);
  float* dst = (float*)(a.ws + (tier == 1 ? sg.off_x1 : sg.off_x2));
  for (long long m = (long long)blockIdx.x * AF_THREADS + threadIdx.x; m < nout; m += (long long)gridDim.x * AF_THREADS) {
    const long long c = AF_DEC * m;
    long long n0 = c - (nin - 1), n1 = c;                  // 0 <= c - n <= nin - 1
    if (n0 < -AF_HALF) n0 = -AF_HALF;
    if (n1 > AF_HALF) n1 = AF_HALF;
    float acc = 0.f;
    for (long long n = n0; n <= n1; ++n) acc = fmaf(a.fir[n + AF_HALF], src[c - n], acc);
    dst[m] = acc;
  }
}

// ---- the filter: one lane per chunk.  BACK: the input is the forward output u read from its end, the output is y.  OUT: start from the stored state and write.
template <bool BACK, bool OUT>
__global__ __launch_bounds__(AF_IIR_THREADS) void k_af_iir(const AfArgs a) {
  const long long blk = blockIdx.x;
  const int s = song_of(a.tab, a.n_songs, blk);
  const AfSong& sg = a.tab[s];
  const long long local = blk - sg.blk0;
  int band; long long cb;
  af_unoff(local, sg.bpb, band, cb);
  const int tier = af_tier_of(band);
  const long long c = cb * AF_IIR_THREADS + threadIdx.x;
  if (c >= af_pick(sg.nc, tier)) return;
  const long long nt = af_pick(sg.n, tier);
  const long long bi = (long long)sg.bank * AF_BANDS + band;
  const double* cf = a.sos + bi * (AF_MAX_SEC * 6);
  const int ns = a.nsec[bi];
  double b0[AF_MAX_SEC], b1[AF_MAX_SEC], b2[AF_MAX_SEC], a1[AF_MAX_SEC], a2[AF_MAX_SEC], z[AF_NS];
#pragma unroll
  for (int k = 0; k < AF_MAX_SEC; ++k) {
    b0[k] = cf[k * 6 + 0]; b1[k] = cf[k * 6 + 1]; b2[k] = cf[k * 6 + 2]; a1[k] = cf[k * 6 + 4]; a2[k] = cf[k * 6 + 5];
  }
  double* st = (double*)(a.ws + sg.off_st) + (af_boff(band, sg.nc) + c) * AF_NS;
#pragma unroll
  for (int k = 0; k < AF_NS; ++k) z[k] = OUT ? st[k] : 0.0;
  const float* xin = tier == 0 ? sg.wav : (const float*)(a.ws + (tier == 1 ? sg.off_x1 : sg.off_x2));
  const long long bo = af_boff(band, sg.n);
  double* u = (double*)(a.ws + sg.off_u) + bo;
  float* y = (float*)(a.ws + sg.off_y) + bo;
  const long long r0 = c * AF_L;
  const long long r1 = r0 + AF_L < nt ? r0 + AF_L : nt;
  for (long long r = r0; r < r1; ++r) {
    const long long idx = BACK ? nt - 1 - r : r;
    double v = BACK ? u[idx] : (double)xin[idx];
#pragma unroll
    for (int k = 0; k < AF_MAX_SEC; ++k) {
      if (k < ns) {                                        // (uniform over the wave: one band per workgroup)
        const double o = b0[k] * v + z[2 * k];
        z[2 * k] = b1[k] * v - a1[k] * o + z[2 * k + 1];
        z[2 * k + 1] = b2[k] * v - a2[k] * o;
        v = o;
      }
    }
    if (OUT) {
      if (BACK) y[idx] = (float)v; else u[idx] = v;
    }
  }
  if (!OUT) {
#pragma unroll
    for (int k = 0; k < AF_NS; ++k) st[k] = z[k];
  }
}

// ---- chunk-start states: one workgroup of 16 lanes per (band, song); lane r < 12 owns row r of A^L and component r of the state.  In place: slot c holds e_c and
// receives s_c.  s_{c+1}[r] = (sum_j A^L[r][j] s_c[j], j ascending) + e_c[r].
__global__ __launch_bounds__(16) void k_af_prop(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const int band = blockIdx.x, r = threadIdx.x, tier = af_tier_of(band);
  const long long nc = af_pick(sg.nc, tier);
  const double* A = a.apow + ((long long)sg.bank * AF_BANDS + band) * (AF_NS * AF_NS);
  double row[AF_NS];
#pragma unroll
  for (int j = 0; j < AF_NS; ++j) row[j] = r < AF_NS ? A[r * AF_NS + j] : 0.0;
  double* st = (double*)(a.ws + sg.off_st) + af_boff(band, sg.nc) * AF_NS;
  double sv = 0.0;
  for (long long c = 0; c < nc; ++c) {
    double e = 0.0;
    if (r < AF_NS) { e = st[c * AF_NS + r]; st[c * AF_NS + r] = sv; }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < AF_NS; ++j) acc += row[j] * __shfl(sv, j, 16);
    sv = acc + e;
  }
}

// ---- pitch energy: E[b][t] = d sum_{k = lo .. hi} y[k]^2 in fp64, k ascending, rounded to fp32 once
__global__ __launch_bounds__(AF_THREADS) void k_af_energy(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const long long total = AF_BANDS * sg.T;
  float* E = (float*)(a.ws + sg.off_E);
  for (long long i = (long long)blockIdx.x * AF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AF_THREADS) {
    const int band = (int)(i / sg.T);
    const long long t = i - (long long)band * sg.T;
    const int tier = af_tier_of(band), d = af_d(tier);
    const long long nt = af_pick(sg.n, tier);
    const float* y = (const float*)(a.ws + sg.off_y) + af_boff(band, sg.n);
    long long lo = t >= 1 ? (AF_HOP * (t - 1) + d - 1) / d : 0;
    long long hi = (AF_HOP * (t + 1)) / d;
    if (hi > nt - 1) hi = nt - 1;
    double acc = 0.0;
    for (long long k = lo; k <= hi; ++k) { const double v = (double)y[k]; acc += v * v; }
    E[i] = (float)((double)d * acc);
  }
}

// ---- chroma: pitch classes summed in ascending pitch order (fp32), L1-normalised, quantised
__global__ __launch_bounds__(AF_THREADS) void k_af_chroma(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const float* E = (const float*)(a.ws + sg.off_E);
  float* out = a.chroma + sg.out_off;
  for (long long t = (long long)blockIdx.x * AF_THREADS + threadIdx.x; t < sg.T; t += (long long)gridDim.x * AF_THREADS) {
    // (rolled loops over the classes, the class sums parked in the output: straight-line code of twelve sums is paired by the SLP vectoriser into packed adds with a
    // crossed op_sel, the form tests/test_isa_guard.py keeps out of this library)
    float sum = 0.f;
#pragma unroll 1
    for (int q = 0; q < 12; ++q) {
      float c = 0.f;
#pragma unroll 1
      for (int b = (q + 12 - 21 % 12) % 12; b < AF_BANDS; b += 12) c += E[(long long)b * sg.T + t];          // (21 + b) % 12 == q, ascending
      out[(long long)q * sg.T + t] = c;
      sum += c;
    }
#pragma unroll 1
    for (int q = 0; q < 12; ++q) {
      const float v = sum < 1e-3f ? 1.f / 12.f : out[(long long)q * sg.T + t] / sum;
      const int cnt = (v > 0.05f ? 1 : 0) + (v > 0.1f ? 1 : 0) + (v > 0.2f ? 1 : 0) + (v > 0.4f ? 1 : 0);
      out[(long long)q * sg.T + t] = 0.25f * (float)cnt;
    }
  }
}

// e[m] = sum_{k < w} hann_w[k] y[m hop + k]^2 in fp64, k ascending, y zero beyond the end; rounded to fp32 once
__device__ __forceinline__ float af_local_energy(const float* y, long long nt, long long m, int w, const double* hann) {
  const long long s0 = m * (w >> 1);
  double acc = 0.0;
  for (int k = 0; k < w; ++k) {
    if (s0 + k >= nt) break;
    const double v = (double)y[s0 + k];
    acc += hann[k] * (v * v);
  }
  return (float)acc;
}

// ---- onset novelty: n[m] = max(0, e[m] - e[m - 1]), e[-1] = 0
__global__ __launch_bounds__(AF_THREADS) void k_af_novelty(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const long long total = af_btotal(sg.nm);
  float* nov = (float*)(a.ws + sg.off_nov);
  for (long long i = (long long)blockIdx.x * AF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AF_THREADS) {
    int band; long long m;
    af_unoff(i, sg.nm, band, m);
    const int tier = af_tier_of(band), w = af_w(tier);
    const double* hann = a.hann + (tier == 2 ? 100 : 0);
    const float* y = (const float*)(a.ws + sg.off_y) + af_boff(band, sg.n);
    const float e1 = af_local_energy(y, af_pick(sg.n, tier), m, w, hann);
    const float e0 = m > 0 ? af_local_energy(y, af_pick(sg.n, tier), m - 1, w, hann) : 0.f;
    nov[i] = fmaxf(0.f, e1 - e0);
  }
}

// ---- peaks: n[m] > n[m - 1], n[m] >= n[m + 1] (missing neighbours are 0), n[m] > 0 -> height d n[m] and the frame; 0 marks "no peak"
__global__ __launch_bounds__(AF_THREADS) void k_af_peaks(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const long long total = af_btotal(sg.nm);
  const float* nov = (const float*)(a.ws + sg.off_nov);
  float* ph = (float*)(a.ws + sg.off_ph);
  int* pf = (int*)(a.ws + sg.off_pf);
  for (long long i = (long long)blockIdx.x * AF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AF_THREADS) {
    int band; long long m;
    af_unoff(i, sg.nm, band, m);
    const int tier = af_tier_of(band);
    const float v = nov[i];
    const float l = m > 0 ? nov[i - 1] : 0.f;
    const float r = m + 1 < af_pick(sg.nm, tier) ? nov[i + 1] : 0.f;
    const bool peak = v > l && v >= r && v > 0.f;
    ph[i] = peak ? (float)af_d(tier) * v : 0.f;
    pf[i] = (int)af_frame(m, tier, sg.T);
  }
}

// ---- CO[q][t]: the heights of class q's peaks whose frame is t, pitches ascending, then m ascending.  The m range searched is a superset (one index wider on both
// sides than the frame formula's inverse); the stored frame decides.
__global__ __launch_bounds__(AF_THREADS) void k_af_co(const AfArgs a) {
  const AfSong& sg = a.tab[blockIdx.y];
  const long long total = 12 * sg.T;
  const float* ph = (const float*)(a.ws + sg.off_ph);
  const int* pf = (const int*)(a.ws + sg.off_pf);
  float* co = (float*)(a.ws + sg.off_co);
  for (long long i = (long long)blockIdx.x * AF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AF_THREADS) {
    const int q = (int)(i / sg.T);
    const long long t = i - (long long)q * sg.T;
    float acc = 0.f;
    for (int b = (q + 12 - 21 % 12) % 12; b < AF_BANDS; b += 12) {          // (21 + b) % 12 == q
      const int tier = af_tier_of(b);
      const long long K = (long long)af_w(tier) * 25 * af_d(tier), nm = af_pick(sg.nm, tier);
      // the first m with K (m + 1) + 11025 >= 22050 t is ceil((22050 t - 11025) / K) - 1
      long long lo = t == 0 ? 0 : (22050 * t - 11025 + K - 1) / K - 2;
      long long hi = t == sg.T - 1 ? nm - 1 : (22050 * (t + 1) - 11025 + K - 1) / K;
      if (lo < 0) lo = 0;
      if (hi > nm - 1) hi = nm - 1;
      const long long o = af_boff(b, sg.nm);
      for (long long m = lo; m <= hi; ++m)
        if (pf[o + m] == (int)t) { const float h = ph[o + m]; if (h > 0.f) acc += h; }
    }
    co[i] = acc;
  }
}

// ---- the DLNCO tail, one workgroup per song: L = log(1 + 10000 CO); g = column norms; G = max(0.1, max of g over +-20 frames); LN = L / G;
// D[:, t] = sum_{i < 10} sqrt(1 / (i + 1)) LN[:, t - i]; DLNCO = D / max_t ||D[:, t]|| (D itself when that maximum is 0)
__global__ __launch_bounds__(AF_THREADS) void k_af_tail(const AfArgs a) {
  __shared__ float red[AF_THREADS / 64];
  const AfSong& sg = a.tab[blockIdx.x];
  const long long T = sg.T;
  const int tid = threadIdx.x;
  float* Lb = (float*)(a.ws + sg.off_co);
  float* g = (float*)(a.ws + sg.off_g);
  float* G = (float*)(a.ws + sg.off_G);
  float* D = (float*)(a.ws + sg.off_D);
  float* out = a.dlnco + sg.out_off;
  for (long long t = tid; t < T; t += AF_THREADS) {
    float ss = 0.f;
    for (int q = 0; q < 12; ++q) {
      const float v = logf(1.f + 10000.f * Lb[q * T + t]);
      Lb[q * T + t] = v;
      ss += v * v;
    }
    g[t] = sqrtf(ss);
  }
  __syncthreads();
  for (long long t = tid; t < T; t += AF_THREADS) {
    const long long t0 = t - 20 > 0 ? t - 20 : 0, t1 = t + 20 < T - 1 ? t + 20 : T - 1;
    float mx = 0.1f;
    for (long long k = t0; k <= t1; ++k) mx = fmaxf(mx, g[k]);
    G[t] = mx;
  }
  __syncthreads();
  float best = 0.f;
  for (long long t = tid; t < T; t += AF_THREADS) {
    float ss = 0.f;
    for (int q = 0; q < 12; ++q) {
      float acc = 0.f;
      for (int i = 0; i < 10; ++i) {
        if (t - i < 0) break;
        acc += sqrtf(1.f / (float)(i + 1)) * (Lb[q * T + t - i] / G[t - i]);
      }
      D[q * T + t] = acc;
      ss += acc * acc;
    }
    best = fmaxf(best, sqrtf(ss));
  }
  best = wave_max(best);
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  float mx = red[0];
  for (int w = 1; w < AF_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
  for (long long i = tid; i < 12 * T; i += AF_THREADS) out[i] = mx > 0.f ? D[i] / mx : D[i];
}

inline long long af_ceil(long long a, long long b) { return (a + b - 1) / b; }

}  // namespace

struct etd_alignfeat {
  etd_alignfeat_cfg cfg;
  std::vector<float> fir;
  std::vector<double> sos, apow, hann;
  std::vector<int> nsec;
  DevPool pool;
  float* d_fir = nullptr;
  double *d_sos = nullptr, *d_apow = nullptr, *d_hann = nullptr;
  int* d_nsec = nullptr;
};

namespace {

// fills tab (when not null) and the totals; ETD_EINVAL for a bad shape
int af_plan(const etd_alignfeat* h, int n_songs, const int64_t* N_host, std::vector<AfSong>* tab, long long* ws_bytes, long long* blocks, long long* maxT) {
  if (!h || !N_host) ETD_FAIL(ETD_EINVAL, "alignfeat: null argument");
  if (n_songs < 1 || n_songs > AF_MAX_SONGS) ETD_FAIL(ETD_EINVAL, "alignfeat: %d songs in one call (need 1 .. %d)", n_songs, AF_MAX_SONGS);
  WsCursor ws{ws_align((long long)n_songs * (long long)sizeof(AfSong))};
  long long blk = 0, out = 0, mt = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long N = N_host[s];
    if (N < 1) ETD_FAIL(ETD_EINVAL, "alignfeat: song %d has N = %lld (need >= 1)", s, N);
    if (N > AF_MAX_N) ETD_FAIL(ETD_EINVAL, "alignfeat: song %d has N = %lld (> %lld)", s, N, (long long)AF_MAX_N);
    AfSong g;
    memset(&g, 0, sizeof(g));
    g.n[0] = N; g.n[1] = af_ceil(N, AF_DEC); g.n[2] = af_ceil(g.n[1], AF_DEC);
    for (int t = 0; t < 3; ++t) {
      g.nc[t] = af_ceil(g.n[t], AF_L);
      g.nm[t] = af_ceil(g.n[t], af_w(t) / 2);
      g.bpb[t] = af_ceil(g.nc[t], AF_IIR_THREADS);
    }
    g.T = af_ceil(N, AF_HOP);
    g.blk0 = blk;
    blk += af_btotal(g.bpb);
    const long long samples = af_btotal(g.n), chunks = af_btotal(g.nc), nov = af_btotal(g.nm);
    g.off_x1 = ws.take(4 * g.n[1]); g.off_x2 = ws.take(4 * g.n[2]);
    g.off_u = ws.take(8 * samples); g.off_y = ws.take(4 * samples);
    g.off_st = ws.take(8 * AF_NS * chunks);
    g.off_E = ws.take(4 * AF_BANDS * g.T);
    g.off_nov = ws.take(4 * nov); g.off_ph = ws.take(4 * nov); g.off_pf = ws.take(4 * nov);
    g.off_co = ws.take(48 * g.T); g.off_g = ws.take(4 * g.T); g.off_G = ws.take(4 * g.T); g.off_D = ws.take(48 * g.T);
    g.out_off = out;
    out += 12 * g.T;
    mt = g.T > mt ? g.T : mt;
    if (blk > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "alignfeat: more than 2^31 - 1 workgroups in one call");
    if (tab) (*tab)[s] = g;
  }
  if (ws_bytes) *ws_bytes = ws.off;
  if (blocks) *blocks = blk;
  if (maxT) *maxT = mt;
  return ETD_OK;
}

int af_upload(etd_alignfeat* h) {
  DevPool& P = h->pool;
  return P.upload_once([&]() -> int {
    ETD_TRY(P.upload(&h->d_fir, h->fir.data(), h->fir.size()));
    ETD_TRY(P.upload(&h->d_sos, h->sos.data(), h->sos.size()));
    ETD_TRY(P.upload(&h->d_apow, h->apow.data(), h->apow.size()));
    ETD_TRY(P.upload(&h->d_hann, h->hann.data(), h->hann.size()));
    return P.upload(&h->d_nsec, h->nsec.data(), h->nsec.size());
  });
}

unsigned af_grid(long long count) {
  long long g = af_ceil(count > 0 ? count : 1, AF_THREADS);
  return (unsigned)(g > (1 << 20) ? (1 << 20) : g);
}

}  // namespace

extern "C" int etd_alignfeat_limits(int* chunk, int* max_sections, long long* max_samples, int* max_songs, int* max_banks) {
  if (chunk) *chunk = AF_L;
  if (max_sections) *max_sections = AF_MAX_SEC;
  if (max_samples) *max_samples = AF_MAX_N;
  if (max_songs) *max_songs = AF_MAX_SONGS;
  if (max_banks) *max_banks = AF_MAX_BANKS;
  return ETD_OK;
}

extern "C" int etd_alignfeat_create(const etd_alignfeat_cfg* cfg, const float* fir_host, const double* sos_host, const int32_t* n_sections, const double* apow_host,
                                    etd_alignfeat** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "alignfeat_create: null argument");
  ETD_CHECK_CFG(cfg, etd_alignfeat_cfg, "alignfeat_create");
  if (cfg->sample_rate != 22050 || cfg->hop != AF_HOP || cfg->fir_taps != AF_TAPS || cfg->decimation != AF_DEC)
    ETD_FAIL(ETD_EINVAL, "alignfeat_create: this build is fixed to 22050 Hz, hop %d, %d taps, decimation %d (got %d, %d, %d, %d)", AF_HOP, AF_TAPS, AF_DEC,
             cfg->sample_rate, cfg->hop, cfg->fir_taps, cfg->decimation);
  if (cfg->chunk != AF_L) ETD_FAIL(ETD_EINVAL, "alignfeat_create: chunk = %d, this build's chunk (the power in apow) is %d", cfg->chunk, AF_L);
  if (cfg->n_banks < 1 || cfg->n_banks > AF_MAX_BANKS) ETD_FAIL(ETD_EINVAL, "alignfeat_create: n_banks = %d must be in 1 .. %d", cfg->n_banks, AF_MAX_BANKS);
  if (!fir_host || !sos_host || !n_sections || !apow_host) ETD_FAIL(ETD_EINVAL, "alignfeat_create: null table");
  if (!finite_all(fir_host, AF_TAPS)) ETD_FAIL(ETD_EINVAL, "alignfeat_create: the decimation filter holds a non-finite value");
  const long long nb = (long long)cfg->n_banks * AF_BANDS;
  for (long long b = 0; b < nb; ++b) {
    const int ns = n_sections[b];
    if (ns > AF_MAX_SEC) ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld has %d sections, more than %d", b, ns, AF_MAX_SEC);
    if (ns < 1) ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld has %d sections (need >= 1)", b, ns);
    for (int k = 0; k < ns; ++k) {
      const double* c = sos_host + (b * AF_MAX_SEC + k) * 6;
      if (!finite_all(c, 6)) ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld section %d holds a non-finite coefficient", b, k);
      if (c[3] != 1.0) ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld section %d has a0 = %g (need 1)", b, k, c[3]);
      if (!(std::fabs(c[5]) < 1.0) || !(std::fabs(c[4]) < 1.0 + c[5]))
        ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld section %d is unstable (a1 = %.17g, a2 = %.17g: a pole on or outside the unit circle)", b, k, c[4], c[5]);
    }
    if (!finite_all(apow_host + b * AF_NS * AF_NS, AF_NS * AF_NS)) ETD_FAIL(ETD_EINVAL, "alignfeat_create: band %lld's chunk matrix holds a non-finite value", b);
  }
  etd_alignfeat* h = new etd_alignfeat();
  h->cfg = *cfg;
  h->fir.assign(fir_host, fir_host + AF_TAPS);
  h->sos.assign(sos_host, sos_host + nb * AF_MAX_SEC * 6);
  h->apow.assign(apow_host, apow_host + nb * AF_NS * AF_NS);
  h->nsec.assign(n_sections, n_sections + nb);
  const double pi = 3.14159265358979323846;
  h->hann.resize(150);
  for (int k = 0; k < 100; ++k) h->hann[k] = 0.5 - 0.5 * cos(2.0 * pi * k / 100.0);
  for (int k = 0; k < 50; ++k) h->hann[100 + k] = 0.5 - 0.5 * cos(2.0 * pi * k / 50.0);
  *out = h;
  return ETD_OK;
}

extern "C" void etd_alignfeat_destroy(etd_alignfeat* h) {
  if (!h) return;
  h->pool.release_uploaded();
  delete h;
}

extern "C" long long etd_alignfeat_num_frames(const etd_alignfeat* h, long long N) {
  if (!h || N < 1) { g_etd_err = "alignfeat_num_frames: null handle or N < 1"; return ETD_EINVAL; }
  return af_ceil(N, AF_HOP);
}

extern "C" long long etd_alignfeat_workspace_bytes(const etd_alignfeat* h, int n_songs, const int64_t* N_host) {
  long long bytes = 0;
  const int rc = af_plan(h, n_songs, N_host, nullptr, &bytes, nullptr, nullptr);
  return rc != ETD_OK ? rc : bytes;
}

extern "C" int etd_alignfeat_debug_layout(const etd_alignfeat* h, int n_songs, const int64_t* N_host, int song, int64_t* out, int n_out) {
  std::vector<AfSong> tab((size_t)(n_songs > 0 && n_songs <= AF_MAX_SONGS ? n_songs : 0));
  ETD_TRY(af_plan(h, n_songs, N_host, &tab, nullptr, nullptr, nullptr));
  if (song < 0 || song >= n_songs || !out || n_out != 24) ETD_FAIL(ETD_EINVAL, "alignfeat_debug_layout: song %d of %d, or out is not int64 [24]", song, n_songs);
  const AfSong& g = tab[song];
  const long long v[24] = {g.T, g.n[0], g.n[1], g.n[2], g.nc[0], g.nc[1], g.nc[2], g.nm[0], g.nm[1], g.nm[2], g.off_x1, g.off_x2, g.off_u, g.off_y, g.off_st,
                           g.off_E, g.off_nov, g.off_ph, g.off_pf, g.off_co, g.off_g, g.off_G, g.off_D, g.out_off};
  for (int i = 0; i < 24; ++i) out[i] = v[i];
  return ETD_OK;
}

extern "C" int etd_alignfeat_run(etd_alignfeat* h, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, const int32_t* bank_host, float* chroma_dev,
                                 float* dlnco_dev, void* workspace_dev, long long workspace_bytes, void* stream) {
  if (!h || !wav_ptrs || !bank_host || !chroma_dev || !dlnco_dev || !workspace_dev) ETD_FAIL(ETD_EINVAL, "alignfeat_run: null argument");
  hipStream_t st = (hipStream_t)stream;
  std::vector<AfSong> tab((size_t)(n_songs > 0 && n_songs <= AF_MAX_SONGS ? n_songs : 0));
  long long need = 0, blocks = 0, maxT = 0;
  ETD_TRY(af_plan(h, n_songs, N_host, &tab, &need, &blocks, &maxT));
  if (workspace_bytes < need) ETD_FAIL(ETD_EINVAL, "alignfeat_run: the workspace holds %lld bytes, this call needs %lld", workspace_bytes, need);
  if ((uintptr_t)workspace_dev & 255) ETD_FAIL(ETD_EINVAL, "alignfeat_run: the workspace is not 256-byte aligned");
  long long max_n1 = 0, max_n2 = 0, max_nov = 0;
  double samples = 0.0;
  for (int s = 0; s < n_songs; ++s) {
    if (!wav_ptrs[s]) ETD_FAIL(ETD_EINVAL, "alignfeat_run: song %d has a null pointer", s);
    if (bank_host[s] < 0 || bank_host[s] >= h->cfg.n_banks) ETD_FAIL(ETD_EINVAL, "alignfeat_run: song %d names filterbank %d of %d", s, bank_host[s], h->cfg.n_banks);
    tab[s].wav = wav_ptrs[s];
    tab[s].bank = bank_host[s];
    max_n1 = tab[s].n[1] > max_n1 ? tab[s].n[1] : max_n1;
    max_n2 = tab[s].n[2] > max_n2 ? tab[s].n[2] : max_n2;
    const long long nov = af_btotal(tab[s].nm);
    max_nov = nov > max_nov ? nov : max_nov;
    samples += (double)af_btotal(tab[s].n);
  }
  ETD_TRY(af_upload(h));
  ETD_TRY(upload_table(st, workspace_dev, tab));
  AfArgs a;
  a.tab = (const AfSong*)workspace_dev; a.n_songs = n_songs; a.ws = (char*)workspace_dev;
  a.fir = h->d_fir; a.sos = h->d_sos; a.nsec = h->d_nsec; a.apow = h->d_apow; a.hann = h->d_hann;
  a.chroma = chroma_dev; a.dlnco = dlnco_dev;
  const unsigned ns = (unsigned)n_songs;
  {
    ProfScope ps("k_af_decim", st, 2.0 * AF_TAPS * (double)(max_n1 + max_n2) * n_songs, 0);
    hipLaunchKernelGGL(k_af_decim, dim3(af_grid(max_n1), ns), dim3(AF_THREADS), 0, st, a, 1);
    hipLaunchKernelGGL(k_af_decim, dim3(af_grid(max_n2), ns), dim3(AF_THREADS), 0, st, a, 2);
  }
  {
    // 9 fp64 operations per section and sample, about 4.4 sections per band; every sample is swept four times
    ProfScope ps("k_af_iir", st, 4.0 * 9.0 * 4.4 * samples, samples * (4 + 8 + 8 + 8 + 8 + 4));
    hipLaunchKernelGGL((k_af_iir<false, false>), dim3((unsigned)blocks), dim3(AF_IIR_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_prop, dim3(AF_BANDS, ns), dim3(16), 0, st, a);
    hipLaunchKernelGGL((k_af_iir<false, true>), dim3((unsigned)blocks), dim3(AF_IIR_THREADS), 0, st, a);
    hipLaunchKernelGGL((k_af_iir<true, false>), dim3((unsigned)blocks), dim3(AF_IIR_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_prop, dim3(AF_BANDS, ns), dim3(16), 0, st, a);
    hipLaunchKernelGGL((k_af_iir<true, true>), dim3((unsigned)blocks), dim3(AF_IIR_THREADS), 0, st, a);
  }
  {
    ProfScope ps("k_af_features", st, 0, samples * 4 * 4);
    hipLaunchKernelGGL(k_af_energy, dim3(af_grid(AF_BANDS * maxT), ns), dim3(AF_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_chroma, dim3(af_grid(maxT), ns), dim3(AF_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_novelty, dim3(af_grid(max_nov), ns), dim3(AF_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_peaks, dim3(af_grid(max_nov), ns), dim3(AF_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_co, dim3(af_grid(12 * maxT), ns), dim3(AF_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_af_tail, dim3(ns), dim3(AF_THREADS), 0, st, a);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
