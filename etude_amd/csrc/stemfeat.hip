// Stem mel-dB features on the GPU: separated stems [instr][channels][N] -> [instr][T][n_mels] dB features, the input of etd_beat_forward (DESIGN.md 4d is the
// contract).  Replaces the host step of scripts/run_separation.py:124-141, 163-183 (channel mean, librosa.stft, |X|^2, Slaney mel, power_to_db(ref=np.max)).
//
// A ragged batch of songs runs in three launches, whatever the number of songs and stems:
//   k_sf_frames  one workgroup per SF_FRAMES consecutive frames of one (song, stem): channel mean -> window -> real FFT in LDS -> power -> CSR mel; writes the mel
//                POWER into the output buffer and the workgroup's maximum into a side array
//   k_sf_max     one workgroup per (song, stem): the maximum of its workgroups' maxima (exact in any order)
//   k_sf_db      in place: 10 log10(max(amin, S)) - 10 log10(max(amin, ref)), clamped at -top_db
// Everything but the maximum is computed per frame from that stem's samples in a fixed order, so a stem's features are bit-identical alone and in any batch.
//
// The FFT is the packed-real Stockham plan of csrc/lds_rfft.h (M = n_fft / 2 = 32 .. 2048 complex points, 256 threads) with the table exp(-2 pi i n / M) copied into
// padded LDS once per workgroup, which is why a workgroup takes SF_FRAMES frames.
#include "stemfeat.h"
#include "prof.h"

#include <cmath>

namespace {

struct SfArgs {
  const SfSong* tab; int n_songs, instr, channels;
  int n_fft, lgM, hop, lead, reflect;
  const float* window; const float2* twM; const float2* twS;
  const int* mel_start; const int* mel_len; const int* mel_off; const float* mel_w; int n_mels;
  float* feat; float* wgmax;
};

// the workgroup's maximum of mx -> *dst, by thread 0 (red: one float per wave)
__device__ __forceinline__ void sf_block_max(float mx, float* red, int tid, float* dst) {
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    float v = red[0];
    for (int w = 1; w < SF_THREADS / 64; ++w) v = fmaxf(v, red[w]);
    *dst = v;
  }
}

__global__ __launch_bounds__(SF_THREADS) void k_sf_frames(const SfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ float red[SF_THREADS / 64];
  const int M = a.n_fft >> 1, PM = RFFT_PM(M), tid = threadIdx.x;
  float *sr = sm, *si = sm + PM, *dr = sm + 2 * PM, *di = sm + 3 * PM;
  float2* tw = (float2*)(sm + 4 * PM);                 // exp(-2 pi i n / M), n < M, at RFFT_PAD(n)
  const long long b = blockIdx.x;
  const int s = song_of(a.tab, a.n_songs, b);
  const SfSong sg = a.tab[s];
  const long long local = b - sg.blk0;
  const int stem = (int)(local / sg.cps);
  const long long t0 = (local - (long long)stem * sg.cps) * SF_FRAMES;
  const float* wav = sg.wav + (long long)stem * a.channels * sg.N;
  float* out = a.feat + sg.feat_off + (long long)stem * sg.T * a.n_mels;
  const float fch = (float)a.channels;
  for (int n = tid; n < M; n += SF_THREADS) tw[RFFT_PAD(n)] = a.twM[n];
  float mx = 0.f;                                      // (mel power is >= 0)
  for (int f = 0; f < SF_FRAMES; ++f) {
    const long long t = t0 + f;
    if (t >= sg.T) break;                              // (uniform over the workgroup)
    // ---- channel mean, window, even / odd samples -> real / imaginary part
    for (int i = tid; i < a.n_fft; i += SF_THREADS) {
      long long idx = t * a.hop - a.lead + i;
      bool inside = idx >= 0 && idx < sg.N;
      if (a.reflect) {                                 // (N > n_fft / 2 is checked on the host: one reflection lands inside)
        if (idx < 0) idx = -idx;
        if (idx >= sg.N) idx = 2 * (sg.N - 1) - idx;
        inside = true;
      }
      float v = 0.f;
      if (inside) {
        v = wav[idx];
        for (int c = 1; c < a.channels; ++c) v += wav[(long long)c * sg.N + idx];
        v = (v / fch) * a.window[i];
      }
      ((i & 1) ? si : sr)[RFFT_PAD(i >> 1)] = v;
    }
    __syncthreads();
    // ---- Stockham FFT of M complex points (the plan of lds_rfft.h): every pass goes from (sr, si) to (dr, di) and swaps them, so Z lands in (sr, si)
    int Ns = 1, lgNs = 0;
    if (a.lgM & 1) {
      for (int j = tid; j < (M >> 1); j += SF_THREADS) rfft::radix2(sr, si, dr, di, M, j);
      __syncthreads();
      float* q = sr; sr = dr; dr = q; q = si; si = di; di = q;
      Ns = 2; lgNs = 1;
    }
    for (; Ns < M; Ns <<= 2, lgNs += 2) {
      for (int j = tid; j < (M >> 2); j += SF_THREADS) rfft::radix4(sr, si, dr, di, rfft::TwLds{tw}, M, Ns, M >> (lgNs + 2), j);
      __syncthreads();
      float* q = sr; sr = dr; dr = q; q = si; si = di; di = q;
    }
    // ---- split pass; the power goes into the free pair
    float* pw = dr;                                    // [M + 1], unpadded
    for (int k = tid; k <= M; k += SF_THREADS) pw[k] = rfft::split_power(sr, si, a.twS, M, k);
    __syncthreads();
    for (int m = tid; m < a.n_mels; m += SF_THREADS) {
      const float acc = csr_band(pw, a.mel_start, a.mel_len, a.mel_off, a.mel_w, m);
      out[t * a.n_mels + m] = acc;
      mx = fmaxf(mx, acc);
    }
    __syncthreads();                                   // (the next frame's samples overwrite the buffers pw may live in)
  }
  sf_block_max(mx, red, tid, a.wgmax + b);
}

__global__ __launch_bounds__(SF_THREADS) void k_sf_max(const SfSong* __restrict__ tab, int instr, const float* __restrict__ wgmax, float* __restrict__ ref) {
  __shared__ float red[SF_THREADS / 64];
  const int s = blockIdx.x / instr, stem = blockIdx.x % instr, tid = threadIdx.x;
  const long long n = tab[s].cps;
  const float* p = wgmax + tab[s].blk0 + (long long)stem * n;
  float mx = 0.f;
  for (long long i = tid; i < n; i += SF_THREADS) mx = fmaxf(mx, p[i]);
  sf_block_max(mx, red, tid, ref + blockIdx.x);
}

// y = 10 log10(max(amin, S)) - 10 log10(max(amin, ref)); the stem's largest S gives exactly 0 (the same expression on both sides), so max(y) = 0 and power_to_db's
// second clamp max(y, max(y) - top_db) is max(y, -top_db).  A NaN or infinite S (a non-finite sample) stays NaN: fmaxf would drop it and hide it from the range check.
__global__ __launch_bounds__(SF_THREADS) void k_sf_db(const SfSong* __restrict__ tab, int instr, int n_mels, const float* __restrict__ ref, float amin, float top_db,
                                                       float* __restrict__ feat) {
  const int s = blockIdx.y / instr, stem = blockIdx.y % instr;
  const long long n = tab[s].T * n_mels;
  float* p = feat + tab[s].feat_off + (long long)stem * n;
  const float r = 10.f * log10f(fmaxf(amin, ref[blockIdx.y]));
  for (long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SF_THREADS) {
    const float S = p[i];
    float y = fmaxf(10.f * log10f(fmaxf(amin, S)) - r, -top_db);
    if (!(S <= 3.402823466e+38f)) y = __builtin_nanf("");
    p[i] = y;
  }
}

}  // namespace

struct etd_stemfeat {
  etd_stemfeat_cfg cfg;
  int M = 0, lgM = 0, lead = 0;
  // host tables (create needs no GPU); uploaded by the first run
  std::vector<float> window, mel_w;
  std::vector<float2> twM, twS;
  std::vector<int> mel_start, mel_len, mel_off;
  DevPool pool;
  float *d_window = nullptr, *d_mel_w = nullptr;
  float2 *d_twM = nullptr, *d_twS = nullptr;
  int *d_mel_start = nullptr, *d_mel_len = nullptr, *d_mel_off = nullptr;
  // per-call workspace, grown on demand: per-workgroup maxima + per-(song, stem) maxima, and the song table
  float* ws = nullptr; long long ws_floats = 0;
  SfSong* tab = nullptr; int tab_cap = 0;
};

namespace {

// fills tab (when not null) and the totals; ETD_EINVAL for a bad shape
int sf_plan(const etd_stemfeat* h, int n_songs, int instr, const int64_t* N_host, std::vector<SfSong>* tab, long long* blocks, long long* frames, long long* maxT) {
  if (!h || !N_host || n_songs < 1 || instr < 1) ETD_FAIL(ETD_EINVAL, "stemfeat: null argument, n_songs < 1 or instr < 1");
  if ((long long)n_songs * instr > 65535) ETD_FAIL(ETD_EINVAL, "stemfeat: more than 65535 (song, stem) pairs in one call (%d x %d)", n_songs, instr);
  long long b = 0, fr = 0, mt = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long N = N_host[s];
    if (N < 1) ETD_FAIL(ETD_EINVAL, "stemfeat: song %d has N = %lld (need >= 1)", s, N);
    if (N > (1LL << 40)) ETD_FAIL(ETD_EINVAL, "stemfeat: song %d has N = %lld (> 2^40)", s, N);
    if (h->cfg.framing == ETD_STEMFEAT_LIBROSA_REFLECT && N <= h->cfg.n_fft / 2)
      ETD_FAIL(ETD_EINVAL, "stemfeat: song %d has N = %lld <= n_fft / 2 = %d (reflect padding undefined)", s, N, h->cfg.n_fft / 2);
    const long long T = 1 + (N + 2 * h->lead - h->cfg.n_fft) / h->cfg.hop;
    const long long cps = (T + SF_FRAMES - 1) / SF_FRAMES;
    if (tab) (*tab)[s] = SfSong{nullptr, N, T, fr * instr * h->cfg.n_mels, b, cps};
    b += cps * instr; fr += T; mt = T > mt ? T : mt;
    if (b > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "stemfeat: more than 2^31 - 1 workgroups in one call");
  }
  *blocks = b; *frames = fr; *maxT = mt;
  return ETD_OK;
}

int sf_upload(etd_stemfeat* h) {
  DevPool& P = h->pool;
  return P.upload_once([&]() -> int {
    ETD_TRY(P.upload(&h->d_window, h->window.data(), h->window.size()));
    ETD_TRY(P.upload(&h->d_twM, h->twM.data(), h->twM.size()));
    ETD_TRY(P.upload(&h->d_twS, h->twS.data(), h->twS.size()));
    ETD_TRY(P.upload(&h->d_mel_start, h->mel_start.data(), h->mel_start.size()));
    ETD_TRY(P.upload(&h->d_mel_len, h->mel_len.data(), h->mel_len.size()));
    ETD_TRY(P.upload(&h->d_mel_off, h->mel_off.data(), h->mel_off.size()));
    return P.upload(&h->d_mel_w, h->mel_w.data(), h->mel_w.size());
  });
}

}  // namespace

extern "C" int etd_stemfeat_create(const etd_stemfeat_cfg* cfg, const float* window_host, const int32_t* mel_start, const int32_t* mel_len,
                                   const float* mel_w_host, etd_stemfeat** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "stemfeat_create: null argument");
  ETD_CHECK_CFG(cfg, etd_stemfeat_cfg, "stemfeat_create");
  const int n_fft = cfg->n_fft;
  if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1))) ETD_FAIL(ETD_EINVAL, "stemfeat_create: n_fft = %d must be a power of two in 64 .. 4096", n_fft);
  if (cfg->hop < 1 || cfg->hop > (1 << 20)) ETD_FAIL(ETD_EINVAL, "stemfeat_create: hop = %d must be in 1 .. 2^20", cfg->hop);
  if (cfg->n_mels < 1 || cfg->n_mels > 1024) ETD_FAIL(ETD_EINVAL, "stemfeat_create: n_mels = %d must be in 1 .. 1024", cfg->n_mels);
  if (cfg->framing != ETD_STEMFEAT_LIBROSA && cfg->framing != ETD_STEMFEAT_LIBROSA_REFLECT && cfg->framing != ETD_STEMFEAT_SPLEETER)
    ETD_FAIL(ETD_EINVAL, "stemfeat_create: framing = %d is not one of ETD_STEMFEAT_*", cfg->framing);
  if (!(cfg->amin > 0.f) || !std::isfinite(cfg->amin) || !(cfg->top_db > 0.f) || !std::isfinite(cfg->top_db))
    ETD_FAIL(ETD_EINVAL, "stemfeat_create: amin and top_db must be positive and finite");
  if (!window_host || !mel_start || !mel_len || !mel_w_host) ETD_FAIL(ETD_EINVAL, "stemfeat_create: null table");
  if (!finite_all(window_host, (size_t)n_fft)) ETD_FAIL(ETD_EINVAL, "stemfeat_create: the window holds a non-finite value");
  std::vector<int> off(cfg->n_mels);
  long long tot = 0;
  for (int m = 0; m < cfg->n_mels; ++m) {
    if (mel_start[m] < 0 || mel_len[m] < 0 || (long long)mel_start[m] + mel_len[m] > n_fft / 2 + 1)
      ETD_FAIL(ETD_EINVAL, "stemfeat_create: mel band %d covers bins [%d, %d + %d), outside 0 .. %d", m, mel_start[m], mel_start[m], mel_len[m], n_fft / 2);
    off[m] = (int)tot; tot += mel_len[m];
  }
  if (!finite_all(mel_w_host, (size_t)tot)) ETD_FAIL(ETD_EINVAL, "stemfeat_create: the mel weights hold a non-finite value");
  for (long long i = 0; i < tot; ++i)
    if (mel_w_host[i] < 0.f) ETD_FAIL(ETD_EINVAL, "stemfeat_create: mel weight %lld is negative", i);
  etd_stemfeat* h = new etd_stemfeat();
  h->cfg = *cfg;
  h->M = n_fft / 2;
  while ((1 << h->lgM) < h->M) ++h->lgM;
  h->lead = cfg->framing == ETD_STEMFEAT_SPLEETER ? n_fft : n_fft / 2;
  h->window.assign(window_host, window_host + n_fft);
  h->mel_start.assign(mel_start, mel_start + cfg->n_mels);
  h->mel_len.assign(mel_len, mel_len + cfg->n_mels);
  h->mel_off = off;
  h->mel_w.assign(mel_w_host, mel_w_host + tot);
  if (h->mel_w.empty()) h->mel_w.push_back(0.f);
  rfft_twiddles(h->M, h->twM, h->twS);
  *out = h;
  return ETD_OK;
}

extern "C" void etd_stemfeat_destroy(etd_stemfeat* h) {
  if (!h) return;
  if (h->pool.uploaded || h->ws || h->tab) {
    (void)hipDeviceSynchronize();   // kernels of this handle may still be in flight
    h->pool.free_all();
    if (h->ws) (void)hipFree(h->ws);
    if (h->tab) (void)hipFree(h->tab);
  }
  delete h;
}

extern "C" long long etd_stemfeat_num_frames(const etd_stemfeat* h, long long N) {
  if (!h || N < 1) { g_etd_err = "stemfeat_num_frames: null handle or N < 1"; return ETD_EINVAL; }
  return 1 + (N + 2 * h->lead - h->cfg.n_fft) / h->cfg.hop;
}

extern "C" long long etd_stemfeat_workspace_bytes(const etd_stemfeat* h, int n_songs, int instr, const int64_t* N_host) {
  long long blocks = 0, frames = 0, maxT = 0;
  const int rc = sf_plan(h, n_songs, instr, N_host, nullptr, &blocks, &frames, &maxT);
  if (rc != ETD_OK) return rc;
  return (blocks + (long long)n_songs * instr) * 4 + (long long)n_songs * (long long)sizeof(SfSong);
}

extern "C" int etd_stemfeat_run(etd_stemfeat* h, const float* const* wav_ptrs, int n_songs, int instr, int channels, const int64_t* N_host, float* feat_dev, void* stream) {
  if (!h || !wav_ptrs || !feat_dev || channels < 1) ETD_FAIL(ETD_EINVAL, "stemfeat_run: null argument or channels < 1");
  hipStream_t st = (hipStream_t)stream;
  std::vector<SfSong> tab((size_t)(n_songs > 0 ? n_songs : 0));
  long long blocks = 0, frames = 0, maxT = 0;
  ETD_TRY(sf_plan(h, n_songs, instr, N_host, &tab, &blocks, &frames, &maxT));
  for (int s = 0; s < n_songs; ++s) {
    if (!wav_ptrs[s]) ETD_FAIL(ETD_EINVAL, "stemfeat_run: song %d has a null pointer", s);
    tab[s].wav = wav_ptrs[s];
  }
  ETD_TRY(sf_upload(h));
  const long long pairs = (long long)n_songs * instr;
  if (blocks + pairs > h->ws_floats) {
    HIP_TRY(hipStreamSynchronize(st));
    if (h->ws) { (void)hipFree(h->ws); h->ws = nullptr; h->ws_floats = 0; }
    HIP_TRY(hipMalloc((void**)&h->ws, (size_t)(blocks + pairs) * 4));
    h->ws_floats = blocks + pairs;
  }
  if (n_songs > h->tab_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    if (h->tab) { (void)hipFree(h->tab); h->tab = nullptr; h->tab_cap = 0; }
    HIP_TRY(hipMalloc((void**)&h->tab, (size_t)n_songs * sizeof(SfSong)));
    h->tab_cap = n_songs;
  }
  ETD_TRY(upload_table(st, h->tab, tab));
  float* wgmax = h->ws;
  float* ref = h->ws + blocks;
  const etd_stemfeat_cfg& c = h->cfg;
  SfArgs a;
  a.tab = h->tab; a.n_songs = n_songs; a.instr = instr; a.channels = channels;
  a.n_fft = c.n_fft; a.lgM = h->lgM; a.hop = c.hop; a.lead = h->lead; a.reflect = c.framing == ETD_STEMFEAT_LIBROSA_REFLECT ? 1 : 0;
  a.window = h->d_window; a.twM = h->d_twM; a.twS = h->d_twS;
  a.mel_start = h->d_mel_start; a.mel_len = h->d_mel_len; a.mel_off = h->d_mel_off; a.mel_w = h->d_mel_w; a.n_mels = c.n_mels;
  a.feat = feat_dev; a.wgmax = wgmax;
  const double fr = (double)frames * instr;
  {
    // 5 N log2 N flops of an M-point complex FFT + the split pass + the CSR product; bytes: every sample once + the mel power written
    ProfScope ps("k_sf_frames", st, fr * (5.0 * h->M * h->lgM + 12.0 * h->M + 2.0 * (double)h->mel_w.size()),
                 fr * ((double)c.hop * channels * 4 + (double)c.n_mels * 4));
    const size_t lds = (size_t)SF_LDS_FLOATS(h->M) * sizeof(float);
    hipLaunchKernelGGL(k_sf_frames, dim3((unsigned)blocks), dim3(SF_THREADS), lds, st, a);
  }
  {
    ProfScope ps("k_sf_max", st, 0, (double)blocks * 4);
    hipLaunchKernelGGL(k_sf_max, dim3((unsigned)pairs), dim3(SF_THREADS), 0, st, h->tab, instr, wgmax, ref);
  }
  {
    ProfScope ps("k_sf_db", st, 0, fr * c.n_mels * 8);
    long long gx = (maxT * c.n_mels + SF_THREADS * 4 - 1) / (SF_THREADS * 4);
    if (gx > 65535) gx = 65535;
    hipLaunchKernelGGL(k_sf_db, dim3((unsigned)gx, (unsigned)pairs), dim3(SF_THREADS), 0, st, h->tab, instr, c.n_mels, ref, c.amin, c.top_db, feat_dev);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
