// Tuning estimation on the GPU: mono audio at 22 050 Hz -> the deviation from 440 Hz equal temperament in whole cents, -50 .. 49, and the comb similarity behind it
// (DESIGN.md 4g is the contract; modelled on synctoolbox's estimate_tuning with its defaults: a long-window STFT, log compression, the sum over time, a cubic spline
// onto a 1-cent log-frequency axis, a local average, rectification and a comb of 100-cent teeth shifted cent by cent).
//
// A ragged batch of songs runs in three launches, whatever the number of songs:
//   k_tn_frames  one workgroup per TN_GROUP = 8 consecutive frames of one song: window -> real FFT of 16 384 points in LDS -> power -> log(1 + 100 P), summed over the
//                group's frames into the group's partial row (a thread owns its bins)
//   k_tn_sum     Y[k] = the groups' partial sums added in ascending order
//   k_tn_tail    one workgroup per song, fp64: the not-a-knot spline through Y (its tridiagonal system by one lane, in LDS), the 8 400 log-frequency values, the local
//                average, rectification, the comb, the first maximum
// No atomics, no flags, no spinning: a song's numbers depend on its own samples and the tables alone, in a fixed order.
//
// The FFT is the packed-real Stockham plan of csrc/lds_rfft.h at M = 8 192 complex points (log2 M = 13: the radix-2 stage, then six radix-4 stages) and 1 024 threads.
// The two buffer pairs take 4 x 8 449 floats = 135 184 bytes, so the table exp(-2 pi i n / M) (64 KB) cannot sit in LDS next to them as it does for the stem features:
// it is read from global memory (it stays in the L2).
#include "tuning.h"
#include "prof.h"

#include <cmath>

namespace {

struct TnArgs {
  const TnSong* tab; int n_songs;
  char* ws;
  const float* window;              // [16384]
  const float2* twM;                // exp(-2 pi i n / 8192), n < 8192
  const float2* twS;                // exp(-2 pi i k / 16384), k <= 8192
  const double* rp; const double* cp;       // [8193]: the reciprocal pivots of the spline's elimination and (upper diagonal) x (reciprocal pivot)
  const int* iv; const double* tt;          // [8400]: the knot interval of fl[i] and fl[i] - (its left knot)
  int32_t* tuning; double* sim;
  // the power tap: frames tap_frame[q] of song tap_song -> tap_P[q][8193] (null = off)
  float* tap_P; int tap_song, tap_n; int tap_frame[TN_MAX_TAPS];
};

// one radix-4 pass of the frame kernel, Ns = 2^LG points per transform so far, and its barrier; 2 butterflies per thread
template <int LG>
__device__ __forceinline__ void tn_stage(const float* sr, const float* si, float* dr, float* di, const float2* __restrict__ tw, int tid) {
  for (int j = tid; j < (TN_M >> 2); j += TN_THREADS) rfft::radix4(sr, si, dr, di, rfft::TwGlobal{tw}, TN_M, 1 << LG, TN_M >> (LG + 2), j);
  __syncthreads();
}

__global__ __launch_bounds__(TN_THREADS) void k_tn_frames(const TnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int M = TN_M, PM = RFFT_PM(TN_M);
  const int tid = threadIdx.x;
  float *ar = sm, *ai = sm + PM, *br = sm + 2 * PM, *bi = sm + 3 * PM;
  const long long b = blockIdx.x;
  const int s = song_of(a.tab, a.n_songs, b);
  const TnSong& sg = a.tab[s];
  const long long g = b - sg.blk0, N = sg.N, F = sg.F;
  const float* wav = sg.wav;
  float* part = (float*)(a.ws + sg.off_part) + g * TN_BINS;
  for (int q = 0; q < TN_GROUP; ++q) {
    const long long f = g * TN_GROUP + q;
    if (f >= F) break;                                 // (uniform over the workgroup)
    // ---- window, even / odd samples -> real / imaginary part of buffer A; zero outside the signal
    const long long base = (long long)TN_HOP * (f - 1);
    for (int i = tid; i < M; i += TN_THREADS) {
      const long long i0 = base + 2 * i, i1 = i0 + 1;
      const float v0 = (i0 >= 0 && i0 < N) ? wav[i0] * a.window[2 * i] : 0.f;
      const float v1 = (i1 >= 0 && i1 < N) ? wav[i1] * a.window[2 * i + 1] : 0.f;
      ar[RFFT_PAD(i)] = v0; ai[RFFT_PAD(i)] = v1;
    }
    __syncthreads();
    // ---- Stockham FFT of M complex points (the plan of lds_rfft.h, its sizes constants): A -> B -> A ... seven passes, so Z lands in B
    for (int j = tid; j < (M >> 1); j += TN_THREADS) rfft::radix2(ar, ai, br, bi, M, j);
    __syncthreads();
    tn_stage<1>(br, bi, ar, ai, a.twM, tid);
    tn_stage<3>(ar, ai, br, bi, a.twM, tid);
    tn_stage<5>(br, bi, ar, ai, a.twM, tid);
    tn_stage<7>(ar, ai, br, bi, a.twM, tid);
    tn_stage<9>(br, bi, ar, ai, a.twM, tid);
    tn_stage<11>(ar, ai, br, bi, a.twM, tid);
    // ---- split pass: power, compression, the group's sum.  It reads B alone and the next frame's samples go to A, so no barrier stands between them.
    int slot = -1;
    if (a.tap_P && s == a.tap_song) {
#pragma unroll
      for (int t = 0; t < TN_MAX_TAPS; ++t)
        if (t < a.tap_n && (long long)a.tap_frame[t] == f) slot = t;
    }
    // (a thread owns bins k = tid + 1024 j and keeps their running sums in the group's partial row: rolled, with the nine sums in registers the kernel spills)
#pragma unroll 1
    for (int j = 0; j < TN_BPT; ++j) {
      const int k = tid + j * TN_THREADS;
      if (k <= M) {
        const float P = rfft::split_power(br, bi, a.twS, M, k);
        float p100;
        asm volatile("v_mul_f32 %0, %1, %2" : "=v"(p100) : "v"(P), "v"(100.f));          // (a product of its own: 1 + 100 P is not to become one fused operation)
        const float c = logf(1.f + p100);
        part[k] = q == 0 ? c : part[k] + c;
        if (slot >= 0) a.tap_P[(long long)slot * TN_BINS + k] = P;
      }
    }
  }
}

// Y[k] = ((G_0[k] + G_1[k]) + G_2[k]) + ... in fp32
__global__ __launch_bounds__(TN_TAIL_THREADS) void k_tn_sum(const TnArgs a) {
  const TnSong& sg = a.tab[blockIdx.y];
  const int k = blockIdx.x * TN_TAIL_THREADS + threadIdx.x;
  if (k >= TN_BINS) return;
  const float* part = (const float*)(a.ws + sg.off_part);
  float y = part[k];
  for (long long g = 1; g < sg.G; ++g) y += part[g * TN_BINS + k];
  ((float*)(a.ws + sg.off_Y))[k] = y;
}

// steps 4-6, one workgroup per song, everything fp64.  The spline in its first-derivative form on uniform knots (spacing h): slopes s_j = (Y[j+1] - Y[j]) / h;
// rows  d_0 + 2 d_1 = (5 s_0 + s_1) / 2,  d_{i-1} + 4 d_i + d_{i+1} = 3 (s_{i-1} + s_i),  2 d_{n-2} + d_{n-1} = (s_{n-3} + 5 s_{n-2}) / 2  (not-a-knot at both ends);
// the pivots depend on the knots alone, so their reciprocals rp and the scaled upper diagonal cp are host tables, and the elimination is
//   dp_0 = b_0 rp_0,  dp_i = (b_i - l_i dp_{i-1}) rp_i  (l = 1, the last row's 2),  d_{n-1} = dp_{n-1},  d_i = dp_i - cp_i d_{i+1}
// by ONE lane over the right-hand side in LDS (16 k dependent steps; songs run side by side).
__global__ __launch_bounds__(TN_TAIL_THREADS) void k_tn_tail(const TnArgs a) {
  extern __shared__ __attribute__((aligned(16))) double d[];        // [8193]: the right-hand side, then dp, then the knot derivatives
  __shared__ double sims[TN_THETA];
  const TnSong& sg = a.tab[blockIdx.x];
  const int tid = threadIdx.x, n = TN_BINS;
  const double h = (double)TN_FS / (double)TN_NFFT;
  const float* Y = (const float*)(a.ws + sg.off_Y);
  double* Yi = (double*)(a.ws + sg.off_Yi);
  double* R = (double*)(a.ws + sg.off_R);
  for (int i = tid; i < n; i += TN_TAIL_THREADS) {
    double v;
    if (i == 0) {
      const double s0 = ((double)Y[1] - (double)Y[0]) / h, s1 = ((double)Y[2] - (double)Y[1]) / h;
      v = (5.0 * s0 + s1) / 2.0;
    } else if (i == n - 1) {
      const double s0 = ((double)Y[n - 2] - (double)Y[n - 3]) / h, s1 = ((double)Y[n - 1] - (double)Y[n - 2]) / h;
      v = (s0 + 5.0 * s1) / 2.0;
    } else {
      const double s0 = ((double)Y[i] - (double)Y[i - 1]) / h, s1 = ((double)Y[i + 1] - (double)Y[i]) / h;
      v = 3.0 * (s0 + s1);
    }
    d[i] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double prev = d[0] * a.rp[0];
    d[0] = prev;
#pragma unroll 8
    for (int i = 1; i < n - 1; ++i) {
      prev = (d[i] - prev) * a.rp[i];
      d[i] = prev;
    }
    prev = (d[n - 1] - 2.0 * prev) * a.rp[n - 1];
    d[n - 1] = prev;
#pragma unroll 8
    for (int i = n - 2; i >= 0; --i) {
      prev = d[i] - a.cp[i] * prev;
      d[i] = prev;
    }
  }
  __syncthreads();
  for (int i = tid; i < TN_LOGF; i += TN_TAIL_THREADS) {
    const int j = a.iv[i];                             // 0 .. n - 2 (checked when the table is built)
    const double t = a.tt[i];
    const double y0 = (double)Y[j], s = ((double)Y[j + 1] - y0) / h, d0 = d[j], d1 = d[j + 1];
    const double c2 = (3.0 * s - 2.0 * d0 - d1) / h, c3 = (d0 + d1 - 2.0 * s) / (h * h);
    Yi[i] = y0 + t * (d0 + t * (c2 + t * c3));
  }
  __syncthreads();                                     // (Yi was written by this workgroup: its own stores are visible to it after the barrier)
  for (int i = tid; i < TN_LOGF; i += TN_TAIL_THREADS) {
    const int lo = i - TN_AVG > 0 ? i - TN_AVG : 0, hi = i + TN_AVG < TN_LOGF - 1 ? i + TN_AVG : TN_LOGF - 1;
    double sum = 0.0;
    for (int j = lo; j <= hi; ++j) sum += Yi[j];
    const double r = Yi[i] - sum * (1.0 / (2 * TN_AVG + 1));
    R[i] = r > 0.0 ? r : 0.0;
  }
  __syncthreads();
  if (tid < TN_THETA) {
    const int theta = tid - TN_THETA / 2;
    double sum = 0.0;
    for (int m = 0; m < TN_COMB; ++m) {
      const int i = 100 * m + theta;
      if (i >= 0 && i < TN_LOGF) sum += R[i];
    }
    sims[tid] = sum;
    ((double*)(a.ws + sg.off_sim))[tid] = sum;
    a.sim[(long long)blockIdx.x * TN_THETA + tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int t = 1; t < TN_THETA; ++t)
      if (sims[t] > sims[best]) best = t;              // (the first maximum)
    a.tuning[blockIdx.x] = best - TN_THETA / 2;
  }
}

}  // namespace

struct etd_tuning {
  std::vector<float> window;
  std::vector<float2> twM, twS;
  std::vector<double> rp, cp, tt;
  std::vector<int> iv;
  DevPool pool;
  float* d_window = nullptr;
  float2 *d_twM = nullptr, *d_twS = nullptr;
  double *d_rp = nullptr, *d_cp = nullptr, *d_tt = nullptr;
  int* d_iv = nullptr;
  float* tap_P = nullptr; int tap_song = 0, tap_n = 0; int tap_frame[TN_MAX_TAPS] = {0};
};

namespace {

// fills tab (when not null) and the totals; ETD_EINVAL for a bad shape
int tn_plan(const etd_tuning* h, int n_songs, const int64_t* N_host, std::vector<TnSong>* tab, long long* ws_bytes, long long* blocks) {
  if (!h || !N_host) ETD_FAIL(ETD_EINVAL, "tuning: null argument");
  if (n_songs < 1 || n_songs > TN_MAX_SONGS) ETD_FAIL(ETD_EINVAL, "tuning: %d songs in one call (need 1 .. %d)", n_songs, TN_MAX_SONGS);
  WsCursor ws{ws_align((long long)n_songs * (long long)sizeof(TnSong))};
  long long blk = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long N = N_host[s];
    if (N < TN_MIN_N) ETD_FAIL(ETD_EINVAL, "tuning: song %d has N = %lld (need >= %d, two windows)", s, N, TN_MIN_N);
    if (N > TN_MAX_N) ETD_FAIL(ETD_EINVAL, "tuning: song %d has N = %lld (> %lld)", s, N, (long long)TN_MAX_N);
    TnSong g;
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.F = 1 + N / TN_HOP;
    g.G = (g.F + TN_GROUP - 1) / TN_GROUP;
    g.blk0 = blk;
    blk += g.G;
    g.off_part = ws.take(4LL * TN_BINS * g.G);
    g.off_Y = ws.take(4LL * TN_BINS);
    g.off_Yi = ws.take(8LL * TN_LOGF);
    g.off_R = ws.take(8LL * TN_LOGF);
    g.off_sim = ws.take(8LL * TN_THETA);
    if (tab) (*tab)[s] = g;
  }
  if (ws_bytes) *ws_bytes = ws.off;
  if (blocks) *blocks = blk;
  return ETD_OK;
}

int tn_upload(etd_tuning* h) {
  DevPool& P = h->pool;
  return P.upload_once([&]() -> int {
    ETD_TRY(P.upload(&h->d_window, h->window.data(), h->window.size()));
    ETD_TRY(P.upload(&h->d_twM, h->twM.data(), h->twM.size()));
    ETD_TRY(P.upload(&h->d_twS, h->twS.data(), h->twS.size()));
    ETD_TRY(P.upload(&h->d_rp, h->rp.data(), h->rp.size()));
    ETD_TRY(P.upload(&h->d_cp, h->cp.data(), h->cp.size()));
    ETD_TRY(P.upload(&h->d_tt, h->tt.data(), h->tt.size()));
    ETD_TRY(P.upload(&h->d_iv, h->iv.data(), h->iv.size()));
    // both kernels ask for more dynamic LDS than the 64 KB a launch gets without saying so
    HIP_TRY(hipFuncSetAttribute((const void*)k_tn_frames, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES));
    HIP_TRY(hipFuncSetAttribute((const void*)k_tn_tail, hipFuncAttributeMaxDynamicSharedMemorySize, TN_BINS * (int)sizeof(double)));
    return ETD_OK;
  });
}

}  // namespace

extern "C" int etd_tuning_limits(long long* min_samples, long long* max_samples, int* max_songs) {
  if (min_samples) *min_samples = TN_MIN_N;
  if (max_samples) *max_samples = TN_MAX_N;
  if (max_songs) *max_songs = TN_MAX_SONGS;
  return ETD_OK;
}

extern "C" int etd_tuning_create(const etd_tuning_cfg* cfg, etd_tuning** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "tuning_create: null argument");
  ETD_CHECK_CFG(cfg, etd_tuning_cfg, "tuning_create");
  if (cfg->sample_rate != TN_FS || cfg->n_fft != TN_NFFT || cfg->hop != TN_HOP)
    ETD_FAIL(ETD_EINVAL, "tuning_create: this build is fixed to %d Hz, n_fft %d, hop %d (got %d, %d, %d)", TN_FS, TN_NFFT, TN_HOP, cfg->sample_rate, cfg->n_fft, cfg->hop);
  etd_tuning* h = new etd_tuning();
  const double pi = 3.14159265358979323846;
  h->window.resize(TN_NFFT);
  for (int n = 0; n < TN_NFFT; ++n) h->window[n] = (float)(0.5 - 0.5 * cos(2.0 * pi * n / TN_NFFT));
  rfft_twiddles(TN_M, h->twM, h->twS);
  // the elimination's pivots: p_0 = 1 (upper 2), p_i = 4 - cp_{i-1} (upper 1), p_{n-1} = 1 - 2 cp_{n-2}
  const int n = TN_BINS;
  h->rp.resize(n); h->cp.resize(n);
  h->rp[0] = 1.0; h->cp[0] = 2.0;
  for (int i = 1; i < n - 1; ++i) { h->rp[i] = 1.0 / (4.0 - h->cp[i - 1]); h->cp[i] = h->rp[i]; }
  h->rp[n - 1] = 1.0 / (1.0 - 2.0 * h->cp[n - 2]); h->cp[n - 1] = 0.0;
  // the log-frequency axis: fl[i] = f24 2^(i / 1200), its knot interval and the offset inside it
  const double hk = (double)TN_FS / (double)TN_NFFT, f24 = 440.0 * pow(2.0, (24.0 - 69.0) / 12.0);
  h->iv.resize(TN_LOGF); h->tt.resize(TN_LOGF);
  for (int i = 0; i < TN_LOGF; ++i) {
    const double fl = f24 * pow(2.0, (double)i / 1200.0);
    int j = (int)floor(fl / hk);
    if (j > n - 2) j = n - 2;
    if (j < 0) j = 0;
    h->iv[i] = j;
    h->tt[i] = fl - (double)j * hk;
  }
  *out = h;
  return ETD_OK;
}

extern "C" void etd_tuning_destroy(etd_tuning* h) {
  if (!h) return;
  h->pool.release_uploaded();
  delete h;
}

extern "C" long long etd_tuning_workspace_bytes(const etd_tuning* h, int n_songs, const int64_t* N_host) {
  long long bytes = 0;
  const int rc = tn_plan(h, n_songs, N_host, nullptr, &bytes, nullptr);
  return rc != ETD_OK ? rc : bytes;
}

extern "C" int etd_tuning_debug_layout(const etd_tuning* h, int n_songs, const int64_t* N_host, int song, int64_t* out, int n_out) {
  std::vector<TnSong> tab((size_t)(n_songs > 0 && n_songs <= TN_MAX_SONGS ? n_songs : 0));
  ETD_TRY(tn_plan(h, n_songs, N_host, &tab, nullptr, nullptr));
  if (song < 0 || song >= n_songs || !out || n_out != 7) ETD_FAIL(ETD_EINVAL, "tuning_debug_layout: song %d of %d, or out is not int64 [7]", song, n_songs);
  const TnSong& g = tab[song];
  const long long v[7] = {g.F, g.G, g.off_part, g.off_Y, g.off_Yi, g.off_R, g.off_sim};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return ETD_OK;
}

extern "C" int etd_tuning_debug_power(etd_tuning* h, int song, const int32_t* frames_host, int n_frames, float* power_dev) {
  if (!h) ETD_FAIL(ETD_EINVAL, "tuning_debug_power: null handle");
  if (!power_dev) { h->tap_P = nullptr; h->tap_n = 0; return ETD_OK; }
  if (!frames_host || n_frames < 1 || n_frames > TN_MAX_TAPS || song < 0)
    ETD_FAIL(ETD_EINVAL, "tuning_debug_power: %d frames of song %d (need 1 .. %d frames, song >= 0)", n_frames, song, TN_MAX_TAPS);
  for (int i = 0; i < n_frames; ++i) {
    if (frames_host[i] < 0) ETD_FAIL(ETD_EINVAL, "tuning_debug_power: frame %d is negative", frames_host[i]);
    h->tap_frame[i] = frames_host[i];
  }
  h->tap_P = power_dev; h->tap_song = song; h->tap_n = n_frames;
  return ETD_OK;
}

extern "C" int etd_tuning_run(etd_tuning* h, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, int32_t* tuning_dev, double* sim_dev, void* workspace_dev,
                              long long workspace_bytes, void* stream) {
  if (!h || !wav_ptrs || !workspace_dev) ETD_FAIL(ETD_EINVAL, "tuning_run: null argument");
  if (!tuning_dev || !sim_dev) ETD_FAIL(ETD_EINVAL, "tuning_run: null output (tuning_dev and sim_dev are both written)");
  hipStream_t st = (hipStream_t)stream;
  std::vector<TnSong> tab((size_t)(n_songs > 0 && n_songs <= TN_MAX_SONGS ? n_songs : 0));
  long long need = 0, blocks = 0;
  ETD_TRY(tn_plan(h, n_songs, N_host, &tab, &need, &blocks));
  if (workspace_bytes < need) ETD_FAIL(ETD_EINVAL, "tuning_run: the workspace holds %lld bytes, this call needs %lld", workspace_bytes, need);
  if ((uintptr_t)workspace_dev & 255) ETD_FAIL(ETD_EINVAL, "tuning_run: the workspace is not 256-byte aligned");
  if (blocks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "tuning_run: more than 2^31 - 1 workgroups in one call");
  double frames = 0.0;
  for (int s = 0; s < n_songs; ++s) {
    if (!wav_ptrs[s]) ETD_FAIL(ETD_EINVAL, "tuning_run: song %d has a null pointer", s);
    tab[s].wav = wav_ptrs[s];
    frames += (double)tab[s].F;
  }
  if (h->tap_P) {
    if (h->tap_song >= n_songs) ETD_FAIL(ETD_EINVAL, "tuning_run: the power tap names song %d of %d", h->tap_song, n_songs);
    for (int i = 0; i < h->tap_n; ++i)
      if (h->tap_frame[i] >= tab[h->tap_song].F) ETD_FAIL(ETD_EINVAL, "tuning_run: the power tap names frame %d of %lld", h->tap_frame[i], tab[h->tap_song].F);
  }
  ETD_TRY(tn_upload(h));
  ETD_TRY(upload_table(st, workspace_dev, tab));
  TnArgs a;
  a.tab = (const TnSong*)workspace_dev; a.n_songs = n_songs; a.ws = (char*)workspace_dev;
  a.window = h->d_window; a.twM = h->d_twM; a.twS = h->d_twS; a.rp = h->d_rp; a.cp = h->d_cp; a.iv = h->d_iv; a.tt = h->d_tt;
  a.tuning = tuning_dev; a.sim = sim_dev;
  a.tap_P = h->tap_P; a.tap_song = h->tap_song; a.tap_n = h->tap_n;
  for (int i = 0; i < TN_MAX_TAPS; ++i) a.tap_frame[i] = h->tap_frame[i];
  {
    // 5 M log2 M flops of the M-point complex FFT + the split pass and the logarithm; bytes: every sample twice (the windows overlap by half)
    ProfScope ps("k_tn_frames", st, frames * (5.0 * TN_M * TN_LGM + 20.0 * TN_M), frames * TN_NFFT * 4.0);
    hipLaunchKernelGGL(k_tn_frames, dim3((unsigned)blocks), dim3(TN_THREADS), (size_t)TN_LDS_BYTES, st, a);
  }
  {
    ProfScope ps("k_tn_sum", st, 0, (double)blocks * TN_BINS * 4.0);
    hipLaunchKernelGGL(k_tn_sum, dim3((TN_BINS + TN_TAIL_THREADS - 1) / TN_TAIL_THREADS, (unsigned)n_songs), dim3(TN_TAIL_THREADS), 0, st, a);
  }
  {
    ProfScope ps("k_tn_tail", st, 0, 0);
    hipLaunchKernelGGL(k_tn_tail, dim3((unsigned)n_songs), dim3(TN_TAIL_THREADS), (size_t)TN_BINS * sizeof(double), st, a);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
