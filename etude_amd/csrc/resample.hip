// Audio loading on the GPU: the raw samples of a ragged batch of songs at one source rate (what sits in a WAV data chunk, or planar fp32 already on the device)
// -> fp32 [C][N'] (or [N'] as the mean of the channels) at the handle's target rate.  DESIGN.md 4q is the contract; tests/audio_np.py restates it in fp64.
//
// One launch per call, whatever the number of songs: k_resample_tiles, one workgroup per RsTile = RS_TILE consecutive outputs of one (song, channel).
//   staging   the input span of the tile, x[i0(n0) - half + 1 .. i0(n_last) + half], is decoded (and averaged over the channels of a mono song) into LDS, zero
//             outside [0, N): about RS_TILE down / up + K floats, so the LDS a workgroup needs follows the rate ratio and K, never down alone
//   filter    thread j owns output n = n0 + j:  y[n] = sum_k tab[p][k] x[i0 - half + 1 + k],  i0 = n down div up,  p = n down mod up, one fmaf chain with k ascending
// The table is kept [K][up] on the device: the phases of consecutive outputs are scattered (p advances by down mod up), so in the designed [up][K] order the 64 loads
// of one k would touch 64 rows K floats apart; transposed they fall into ONE row of `up` floats (588 bytes at 48 000 -> 22 050) that the whole workgroup shares.
// A handle whose rates are equal has no table: its tiles decode, deinterleave and (mono) average, one sample per thread.
// No atomics, no flags: an output depends on its own song's samples and the table alone.
#include "resample.h"
#include "prof.h"

namespace {

struct RsArgs {
  const RsSong* songs;
  const RsTile* tiles;
  const float* tab;                 // [K][up]
  long long up, down;
  int half, K, identity;
};

// element e (frame * C + channel) of an interleaved little-endian stream; what extractor.read_wav computes, bit for bit
__device__ __forceinline__ float rs_decode(const unsigned char* __restrict__ src, int fmt, long long e) {
  switch (fmt) {
    case ETD_PCM_U8: return ((float)src[e] - 128.f) * 0.0078125f;
    case ETD_PCM_S16: return (float)((const short*)src)[e] * 3.0517578125e-05f;                      // 2^-15
    case ETD_PCM_S24: {
      const unsigned char* b = src + 3 * e;                                                          // (unaligned: by bytes)
      const int v = (int)((unsigned)b[0] << 8 | (unsigned)b[1] << 16 | (unsigned)b[2] << 24) >> 8;
      return (float)v * 1.1920928955078125e-07f;                                                     // 2^-23
    }
    case ETD_PCM_S32: return (float)((const int*)src)[e] * 4.656612873077393e-10f;                   // 2^-31
    case ETD_PCM_F32: return ((const float*)src)[e];
    default: return (float)((const double*)src)[e];                                                  // ETD_PCM_F64
  }
}

// sample i (0 <= i < N) of channel c
__device__ __forceinline__ float rs_channel(const RsSong& sg, int c, long long i) {
  if (sg.fmt == ETD_PCM_F32_PLANAR) return ((const float*)sg.src)[(long long)c * sg.N + i];
  return rs_decode(sg.src, sg.fmt, i * sg.C + c);
}

// what the filter reads at i: channel c, or the fp32 sum over the channels in order times 1.f / C
__device__ __forceinline__ float rs_sample(const RsSong& sg, int c, long long i) {
  if (!sg.mono) return rs_channel(sg, c, i);
  float s = rs_channel(sg, 0, i);
  for (int q = 1; q < sg.C; ++q) s += rs_channel(sg, q, i);
  return s * sg.inv_c;
}

__global__ __launch_bounds__(RS_THREADS) void k_resample_tiles(const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const RsTile t = a.tiles[blockIdx.x];
  const RsSong sg = a.songs[t.song];
  const int tid = threadIdx.x;
  const long long left = sg.Nout - t.n0;
  const int cnt = left < RS_TILE ? (int)left : RS_TILE;                    // >= 1 (the plan emits no empty tile)
  const long long n = t.n0 + tid;
  float* dst = sg.dst + (long long)t.ch * sg.Nout;
  if (a.identity) {
    if (tid < cnt) dst[n] = rs_sample(sg, t.ch, n);
    return;
  }
  const long long first = (t.n0 * a.down) / a.up, last = ((t.n0 + cnt - 1) * a.down) / a.up;
  const long long base = first - a.half + 1;
  const int L = (int)(last - first) + a.K;                                 // <= the span the launch's LDS holds (rs_span)
  for (int i = tid; i < L; i += RS_THREADS) {
    const long long idx = base + i;
    xs[i] = (idx >= 0 && idx < sg.N) ? rs_sample(sg, t.ch, idx) : 0.f;
  }
  __syncthreads();
  if (tid >= cnt) return;
  const long long nd = n * a.down, i0 = nd / a.up;
  const int p = (int)(nd - i0 * a.up), up = (int)a.up;
  const float* x = xs + (int)(i0 - first);                                 // x[k] = the input at i0 - half + 1 + k
  const float* __restrict__ h = a.tab + p;
  float acc = 0.f;
#pragma unroll 8
  for (int k = 0; k < a.K; ++k) acc = fmaf(h[k * up], x[k], acc);         // (k up < 2^22: the table budget)
  dst[n] = acc;
}

}  // namespace

struct etd_resample {
  int sr_in = 0, sr_out = 0, quality = 0;
  long long up = 1, down = 1;
  int half = 0, K = 0;
  bool identity = false;
  std::vector<float> tab;           // [K][up]
  DevPool pool;
  float* d_tab = nullptr;
  long long lds_limit = 0;          // what the device reports, read with the upload
};

namespace {

long long rs_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// the floats of LDS a tile can need: i0(n0 + T - 1) - i0(n0) <= floor((T - 1) down / up) + 1, plus K
long long rs_span(const etd_resample* h) { return h->identity ? 0 : ((RS_TILE - 1) * h->down) / h->up + 1 + h->K; }

long long rs_out_len(const etd_resample* h, long long N) { return (N * h->up + h->down - 1) / h->down; }

int rs_width(int fmt) {
  switch (fmt) {
    case ETD_PCM_U8: return 1;
    case ETD_PCM_S16: return 2;
    case ETD_PCM_S24: return 3;
    case ETD_PCM_S32: case ETD_PCM_F32: case ETD_PCM_F32_PLANAR: return 4;
    case ETD_PCM_F64: return 8;
    default: return 0;
  }
}

// the shapes of a call -> the song table (shapes only) and one tile record per RS_TILE outputs of every (song, channel); either may be null
int rs_plan(const etd_resample* h, int n_songs, const int64_t* frames, const int32_t* channels, const int32_t* mono, std::vector<RsSong>* songs, std::vector<RsTile>* tiles,
            long long* n_tiles) {
  if (!h || !frames || !channels || !mono) ETD_FAIL(ETD_EINVAL, "resample: null argument");
  if (n_songs < 1 || n_songs > RS_MAX_SONGS) ETD_FAIL(ETD_EINVAL, "resample: %d songs in one call (need 1 .. %d)", n_songs, RS_MAX_SONGS);
  long long total = 0;
  for (int s = 0; s < n_songs; ++s) {
    const long long N = frames[s];
    const int C = channels[s];
    if (C < 1 || C > RS_MAX_CH) ETD_FAIL(ETD_EINVAL, "resample: song %d has %d channels (need 1 .. %d)", s, C, RS_MAX_CH);
    if (N < 1 || N > RS_MAX_N) ETD_FAIL(ETD_EINVAL, "resample: song %d has %lld frames (need 1 .. %lld)", s, N, (long long)RS_MAX_N);
    const long long Nout = rs_out_len(h, N), per = (Nout + RS_TILE - 1) / RS_TILE;
    const int out_ch = mono[s] ? 1 : C;
    if (songs) {
      RsSong g;
      memset(&g, 0, sizeof(g));
      g.N = N; g.Nout = Nout; g.C = C; g.mono = mono[s] ? 1 : 0; g.inv_c = 1.f / (float)C;
      (*songs)[s] = g;
    }
    if (tiles)
      for (int c = 0; c < out_ch; ++c)
        for (long long q = 0; q < per; ++q) tiles->push_back(RsTile{s, c, q * RS_TILE});
    total += per * out_ch;
  }
  if (total > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "resample: %lld workgroups in one call (need <= 2^31 - 1)", total);
  if (n_tiles) *n_tiles = total;
  return ETD_OK;
}

long long rs_ws_bytes(int n_songs, long long n_tiles) { return ws_align((long long)n_songs * (long long)sizeof(RsSong)) + ws_align(n_tiles * (long long)sizeof(RsTile)); }

int rs_upload(etd_resample* h) {
  DevPool& P = h->pool;
  return P.upload_once([&]() -> int {
    int dev = 0, lds = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    h->lds_limit = lds;
    const long long need = rs_span(h) * (long long)sizeof(float);
    if (need > h->lds_limit)
      ETD_FAIL(ETD_EINVAL, "resample: %d -> %d Hz needs %lld bytes of LDS per workgroup (%d outputs span %lld inputs), the device reports %lld", h->sr_in, h->sr_out, need,
               RS_TILE, rs_span(h), h->lds_limit);
    if (!h->identity) ETD_TRY(P.upload(&h->d_tab, h->tab.data(), h->tab.size()));
    // a launch gets 64 KB of dynamic LDS without saying so; every handle asks for the same ceiling, so one handle's call never lowers another's
    HIP_TRY(hipFuncSetAttribute((const void*)k_resample_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return ETD_OK;
  });
}

}  // namespace

extern "C" int etd_resample_create(const etd_resample_cfg* cfg, const float* table_host, etd_resample** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "resample_create: null argument");
  ETD_CHECK_CFG(cfg, etd_resample_cfg, "resample_create");
  if (cfg->sr_in < 1 || cfg->sr_in > RS_MAX_RATE || cfg->sr_out < 1 || cfg->sr_out > RS_MAX_RATE)
    ETD_FAIL(ETD_EINVAL, "resample_create: rates %d -> %d Hz (need 1 .. %d)", cfg->sr_in, cfg->sr_out, RS_MAX_RATE);
  if (cfg->quality != ETD_RESAMPLE_BEST && cfg->quality != ETD_RESAMPLE_FAST) ETD_FAIL(ETD_EINVAL, "resample_create: quality %d (0 = best, 1 = fast)", cfg->quality);
  const long long g = rs_gcd(cfg->sr_in, cfg->sr_out), up = cfg->sr_out / g, down = cfg->sr_in / g;
  const long long Z = cfg->quality == ETD_RESAMPLE_BEST ? 64 : 16;
  const long long half = up >= down ? Z : (Z * down + up - 1) / up;                                  // ceil(Z / s), s = min(1, up / down)
  if (cfg->up != up || cfg->down != down || cfg->half != half)
    ETD_FAIL(ETD_EINVAL, "resample_create: %d -> %d Hz is up %lld, down %lld, half %lld; the caller's table has up %d, down %d, half %d", cfg->sr_in, cfg->sr_out, up,
             down, half, cfg->up, cfg->down, cfg->half);
  const bool identity = up == 1 && down == 1;
  const long long K = 2 * half;
  if (!identity && up * K > RS_MAX_TABLE)
    ETD_FAIL(ETD_EINVAL, "resample_create: %d -> %d Hz needs a table of %lld x %lld = %lld entries, above the %lld a handle keeps: the rates share too small a divisor",
             cfg->sr_in, cfg->sr_out, up, K, up * K, (long long)RS_MAX_TABLE);
  if (!identity && !table_host) ETD_FAIL(ETD_EINVAL, "resample_create: null table");
  etd_resample* h = new etd_resample();
  h->sr_in = cfg->sr_in; h->sr_out = cfg->sr_out; h->quality = cfg->quality;
  h->up = up; h->down = down; h->half = (int)half; h->K = (int)K; h->identity = identity;
  if (!identity) {
    if (!finite_all(table_host, (size_t)(up * K))) { delete h; ETD_FAIL(ETD_EINVAL, "resample_create: the table holds a non-finite value"); }
    h->tab.resize((size_t)(up * K));
    for (long long p = 0; p < up; ++p)
      for (long long k = 0; k < K; ++k) h->tab[(size_t)(k * up + p)] = table_host[p * K + k];
  }
  *out = h;
  return ETD_OK;
}

extern "C" void etd_resample_destroy(etd_resample* h) {
  if (!h) return;
  h->pool.release_uploaded();
  delete h;
}

extern "C" long long etd_resample_out_len(const etd_resample* h, long long N) {
  if (!h) ETD_FAIL(ETD_EINVAL, "resample_out_len: null handle");
  if (N < 0 || N > RS_MAX_N) ETD_FAIL(ETD_EINVAL, "resample_out_len: N = %lld (need 0 .. %lld)", N, (long long)RS_MAX_N);
  return rs_out_len(h, N);
}

extern "C" long long etd_resample_workspace_bytes(const etd_resample* h, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* mono_host) {
  long long n_tiles = 0;
  const int rc = rs_plan(h, n_songs, frames_host, channels_host, mono_host, nullptr, nullptr, &n_tiles);
  return rc != ETD_OK ? rc : rs_ws_bytes(n_songs, n_tiles);
}

extern "C" int etd_resample_debug_layout(const etd_resample* h, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* mono_host, int64_t* out,
                                         long long capacity, long long* n_tiles) {
  if (!n_tiles) ETD_FAIL(ETD_EINVAL, "resample_debug_layout: null n_tiles");
  std::vector<RsSong> songs((size_t)(n_songs > 0 && n_songs <= RS_MAX_SONGS ? n_songs : 0));
  std::vector<RsTile> tiles;
  ETD_TRY(rs_plan(h, n_songs, frames_host, channels_host, mono_host, &songs, &tiles, n_tiles));
  if (*n_tiles > capacity || !out) ETD_FAIL(ETD_ENOMEM, "resample_debug_layout: %lld tiles, out holds %lld", *n_tiles, out ? capacity : 0LL);
  for (size_t i = 0; i < tiles.size(); ++i) {
    const long long left = songs[tiles[i].song].Nout - tiles[i].n0;
    out[4 * i] = tiles[i].song; out[4 * i + 1] = tiles[i].ch; out[4 * i + 2] = tiles[i].n0; out[4 * i + 3] = left < RS_TILE ? left : RS_TILE;
  }
  return ETD_OK;
}

extern "C" int etd_resample_run(etd_resample* h, const void* const* src_ptrs, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* format_host,
                                const int32_t* mono_host, const int64_t* bytes_host, float* const* out_ptrs, void* workspace_dev, long long workspace_bytes, void* stream) {
  if (!h || !src_ptrs || !format_host || !bytes_host || !out_ptrs || !workspace_dev) ETD_FAIL(ETD_EINVAL, "resample_run: null argument");
  hipStream_t st = (hipStream_t)stream;
  std::vector<RsSong> songs((size_t)(n_songs > 0 && n_songs <= RS_MAX_SONGS ? n_songs : 0));
  std::vector<RsTile> tiles;
  long long n_tiles = 0;
  ETD_TRY(rs_plan(h, n_songs, frames_host, channels_host, mono_host, &songs, &tiles, &n_tiles));
  const long long need = rs_ws_bytes(n_songs, n_tiles);
  if (workspace_bytes < need) ETD_FAIL(ETD_EINVAL, "resample_run: the workspace holds %lld bytes, this call needs %lld", workspace_bytes, need);
  if ((uintptr_t)workspace_dev & 255) ETD_FAIL(ETD_EINVAL, "resample_run: the workspace is not 256-byte aligned");
  double in_bytes = 0.0, outs = 0.0;
  for (int s = 0; s < n_songs; ++s) {
    RsSong& g = songs[s];
    const int w = rs_width(format_host[s]);
    if (!w) ETD_FAIL(ETD_EINVAL, "resample_run: song %d has sample format %d (need 0 .. %d)", s, format_host[s], ETD_PCM_F32_PLANAR);
    if (bytes_host[s] != g.N * g.C * w)
      ETD_FAIL(ETD_EINVAL, "resample_run: song %d holds %lld bytes, %lld frames x %d channels x %d bytes are %lld", s, (long long)bytes_host[s], g.N, g.C, w, g.N * g.C * w);
    if (!src_ptrs[s] || !out_ptrs[s]) ETD_FAIL(ETD_EINVAL, "resample_run: song %d has a null pointer", s);
    if (w != 3 && ((uintptr_t)src_ptrs[s] & (uintptr_t)(w - 1))) ETD_FAIL(ETD_EINVAL, "resample_run: the samples of song %d are not aligned to their %d bytes", s, w);
    g.src = (const unsigned char*)src_ptrs[s]; g.dst = out_ptrs[s]; g.fmt = format_host[s];
    in_bytes += (double)bytes_host[s];
    outs += (double)g.Nout * (g.mono ? 1 : g.C);
  }
  ETD_TRY(rs_upload(h));
  // the two tables in one copy: songs, then (256-byte aligned) tiles
  const long long off_tiles = ws_align((long long)n_songs * (long long)sizeof(RsSong));
  std::vector<unsigned char> host((size_t)(off_tiles + n_tiles * (long long)sizeof(RsTile)));
  memcpy(host.data(), songs.data(), songs.size() * sizeof(RsSong));
  memcpy(host.data() + off_tiles, tiles.data(), tiles.size() * sizeof(RsTile));
  ETD_TRY(upload_table(st, workspace_dev, host));
  RsArgs a;
  a.songs = (const RsSong*)workspace_dev; a.tiles = (const RsTile*)((const char*)workspace_dev + off_tiles); a.tab = h->d_tab;
  a.up = h->up; a.down = h->down; a.half = h->half; a.K = h->K; a.identity = h->identity ? 1 : 0;
  {
    ProfScope ps("k_resample_tiles", st, h->identity ? 0.0 : outs * 2.0 * h->K, in_bytes + outs * 4.0);
    hipLaunchKernelGGL(k_resample_tiles, dim3((unsigned)n_tiles), dim3(RS_THREADS), (size_t)(rs_span(h) * (long long)sizeof(float)), st, a);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
