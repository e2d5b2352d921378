// Training data of the source separator on the GPU (DESIGN.md 4o is the contract, tests/separator_data_np.py restates it): the handle keeps every track's magnitudes
// S [1 + I][frames][F][C] on the device and cuts augmented batches from them.
//
//   k_sd_sum     the mix of a track given by its stems alone: the fp32 sum of the stems' samples in instrument order
//   k_sd_gather  one launch per batch: unit (track, t0, a, q) -> mix [B][T][F][C] and target [I][B][T][F][C].  Time stretch to T' = floor(T a) frames by align-corners
//                linear interpolation, centre crop or zero pad back to T, then the frequency axis to F' = floor(F q) bins likewise, bins below min(F, F') kept.  One
//                thread owns the C channels of one (t, f) for the mix and every stem; f runs across the lanes, so the loads of a row are near-contiguous and the
//                stores contiguous; (unit, t) is fixed per workgroup, so the time position and weight sit in scalar registers.  No LDS, no atomics.
//
// The device never draws a random number: the draws are the caller's.
#include "separator_data.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

__global__ __launch_bounds__(SD_THREADS) void k_sd_sum(const SdStems s, int I, long long n, float* __restrict__ mix) {
  const long long e = (long long)blockIdx.x * SD_THREADS + threadIdx.x;
  if (e >= n) return;
  float acc = s.p[0][e];
  for (int i = 1; i < I; ++i) acc += s.p[i][e];
  mix[e] = acc;
}

__device__ __forceinline__ float sd_lerp(float u, float v, float w) { return fmaf(w, v - u, u); }

// grid (T x fblocks, B).  Positions and weights in double, the weight rounded once; a position that is a whole number has weight 0 and lerp returns u exactly.
__global__ __launch_bounds__(SD_THREADS) void k_sd_gather(const SdUnit* __restrict__ units, int T, int F, int C, int I, int fblocks, float* __restrict__ mix,
                                                         float* __restrict__ target) {
  const int b = blockIdx.y, B = gridDim.y;
  const int t = blockIdx.x / fblocks, f = (blockIdx.x - t * fblocks) * SD_THREADS + threadIdx.x;
  if (f >= F) return;
  const SdUnit un = units[b];
  // ---- time: output frame t reads stretched frame r of T', which sits at position r (T - 1) / (T' - 1) of the window
  const int r = un.Tp >= T ? t + (un.Tp - T) / 2 : t - (T - un.Tp) / 2;
  const bool tin = r >= 0 && r < un.Tp;
  int i0 = 0, i1 = 0;
  float wt = 0.f;
  if (tin) {
    const double pt = (double)r * (double)(T - 1) / (double)(un.Tp - 1);
    i0 = min((int)pt, T - 1); i1 = min(i0 + 1, T - 1);
    wt = (float)(pt - (double)i0);
  }
  // ---- frequency: bin f < min(F, F') sits at position f (F - 1) / (F' - 1)
  const bool fin = f < min(F, un.Fp);
  int j0 = 0, j1 = 0;
  float wf = 0.f;
  if (fin) {
    const double pf = (double)f * (double)(F - 1) / (double)(un.Fp - 1);
    j0 = min((int)pf, F - 1); j1 = min(j0 + 1, F - 1);
    wf = (float)(pf - (double)j0);
  }
  const long long plane = (long long)T * F * C, o = ((long long)b * T + t) * F * C + (long long)f * C;
  const bool live = tin && fin;
  const long long fr0 = (long long)un.t0 + i0, fr1 = (long long)un.t0 + i1;      // frames from Tf on are zeros and are not read
  const bool r0 = live && fr0 < un.Tf, r1 = live && fr1 < un.Tf;
  for (int k = 0; k <= I; ++k) {
    float* dst = k == 0 ? mix + o : target + (long long)(k - 1) * B * plane + o;
    const float* src = un.S + (long long)k * un.ks;
    const float* row0 = src + fr0 * F * C;
    const float* row1 = src + fr1 * F * C;
    for (int c = 0; c < C; ++c) {
      float v = 0.f;
      if (live) {
        const float u00 = r0 ? row0[j0 * C + c] : 0.f, u01 = r0 ? row0[j1 * C + c] : 0.f;
        const float u10 = r1 ? row1[j0 * C + c] : 0.f, u11 = r1 ? row1[j1 * C + c] : 0.f;
        v = sd_lerp(sd_lerp(u00, u10, wt), sd_lerp(u01, u11, wt), wf);
      }
      dst[c] = v;
    }
  }
}

}  // namespace

struct SdTrack { float* S = nullptr; long long Tf = 0, frames = 0, bytes = 0; };

struct etd_sepdata {
  etd_sepdata_cfg cfg;
  std::vector<SdTrack> tracks;
  long long held = 0;
  SdUnit* units_dev = nullptr; int units_cap = 0;
};

namespace {
long long sd_budget(const etd_sepdata* h) { return h->cfg.max_bytes > 0 ? h->cfg.max_bytes : (16LL << 30); }
long long sd_frames(const etd_sepdata* h, long long Tf) { return (Tf + h->cfg.T - 1) / h->cfg.T * h->cfg.T; }
long long sd_track_bytes(const etd_sepdata* h, long long Tf) {
  return (long long)(1 + h->cfg.n_instr) * sd_frames(h, Tf) * h->cfg.F * h->cfg.n_channels * 4;
}
}  // namespace

extern "C" int etd_sepdata_create(const etd_sepdata_cfg* cfg, etd_sepdata** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "sepdata_create: null argument");
  ETD_CHECK_CFG(cfg, etd_sepdata_cfg, "sepdata_create");
  const etd_sepdata_cfg& c = *cfg;
  if (c.n_instr < 1 || c.n_instr > ETD_SEP_MAX_INSTR) ETD_FAIL(ETD_EINVAL, "sepdata_create: n_instr = %d outside 1 .. %d", c.n_instr, ETD_SEP_MAX_INSTR);
  if (c.n_channels < 1 || c.n_channels > ETD_SEP_MAX_CHANNELS) ETD_FAIL(ETD_EINVAL, "sepdata_create: n_channels = %d outside 1 .. %d", c.n_channels, ETD_SEP_MAX_CHANNELS);
  if (c.T < 2 || c.T > 65536 || c.F < 2 || c.F > 65536) ETD_FAIL(ETD_EINVAL, "sepdata_create: T = %d and F = %d must be in 2 .. 65536", c.T, c.F);
  if (c.max_bytes < 0) ETD_FAIL(ETD_EINVAL, "sepdata_create: max_bytes = %lld is negative", c.max_bytes);
  etd_sepdata* h = new etd_sepdata();
  h->cfg = c;
  *out = h;
  return ETD_OK;
}

extern "C" void etd_sepdata_destroy(etd_sepdata* h) {
  if (!h) return;
  if (!h->tracks.empty() || h->units_dev) {
    (void)hipDeviceSynchronize();      // a gather of this handle may still be in flight
    for (auto& t : h->tracks) (void)hipFree(t.S);
    if (h->units_dev) (void)hipFree(h->units_dev);
  }
  delete h;
}

extern "C" long long etd_sepdata_track_bytes(const etd_sepdata* h, long long Tf) {
  if (!h || Tf < 1 || Tf > 0x7fffffffLL) { g_etd_err = "sepdata_track_bytes: null handle or Tf outside 1 .. 2^31 - 1"; return ETD_EINVAL; }
  return sd_track_bytes(h, Tf);
}
extern "C" long long etd_sepdata_bytes(const etd_sepdata* h) { return h ? h->held : ETD_EINVAL; }
extern "C" int etd_sepdata_num_tracks(const etd_sepdata* h) { return h ? (int)h->tracks.size() : ETD_EINVAL; }
extern "C" long long etd_sepdata_track_frames(const etd_sepdata* h, int track) {
  if (!h || track < 0 || track >= (int)h->tracks.size()) { g_etd_err = "sepdata_track_frames: null handle or no such track"; return ETD_EINVAL; }
  return h->tracks[(size_t)track].Tf;
}

extern "C" int etd_sepdata_add_track(etd_sepdata* h, long long Tf, float** mag_dev, int* track) {
  if (!h || !mag_dev || !track) ETD_FAIL(ETD_EINVAL, "sepdata_add_track: null argument");
  if (Tf < 1 || Tf > 0x7fffffffLL - h->cfg.T) ETD_FAIL(ETD_EINVAL, "sepdata_add_track: Tf = %lld outside 1 .. 2^31 - 1 - T", Tf);
  const long long need = sd_track_bytes(h, Tf);
  if (h->held + need > sd_budget(h))
    ETD_FAIL(ETD_EINVAL, "sepdata_add_track: track %d of %lld frames needs %lld bytes, %lld of the budget of %lld are held", (int)h->tracks.size(), Tf, need, h->held,
             sd_budget(h));
  SdTrack t;
  HIP_TRY(hipMalloc((void**)&t.S, (size_t)need + 256));
  t.Tf = Tf; t.frames = sd_frames(h, Tf); t.bytes = need;
  h->tracks.push_back(t);
  h->held += need;
  *mag_dev = t.S;
  *track = (int)h->tracks.size() - 1;
  return ETD_OK;
}

extern "C" int etd_sepdata_sum_stems(etd_sepdata* h, const float* const* stems_dev, long long n, float* mix_dev, void* stream) {
  if (!h || !stems_dev || !mix_dev || n < 1) ETD_FAIL(ETD_EINVAL, "sepdata_sum_stems: null argument or n < 1");
  SdStems s{};
  for (int i = 0; i < h->cfg.n_instr; ++i) {
    if (!stems_dev[i]) ETD_FAIL(ETD_EINVAL, "sepdata_sum_stems: stem %d is a null pointer", i);
    s.p[i] = stems_dev[i];
  }
  const long long blocks = (n + SD_THREADS - 1) / SD_THREADS;
  if (blocks > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "sepdata_sum_stems: n = %lld needs %lld workgroups (> 2^31 - 1)", n, blocks);
  hipLaunchKernelGGL(k_sd_sum, dim3((unsigned)blocks), dim3(SD_THREADS), 0, (hipStream_t)stream, s, h->cfg.n_instr, n, mix_dev);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_sepdata_gather(etd_sepdata* h, int B, const int32_t* track, const int64_t* t0, const double* a, const double* q, float* mix_dev, float* target_dev,
                                  void* stream) {
  if (!h || !track || !t0 || !a || !q || !mix_dev || !target_dev) ETD_FAIL(ETD_EINVAL, "sepdata_gather: null argument");
  if (B < 1 || B > 65535) ETD_FAIL(ETD_EINVAL, "sepdata_gather: B = %d units outside 1 .. 65535", B);
  const etd_sepdata_cfg& c = h->cfg;
  std::vector<SdUnit> units((size_t)B);
  for (int u = 0; u < B; ++u) {
    if (track[u] < 0 || track[u] >= (int)h->tracks.size()) ETD_FAIL(ETD_EINVAL, "sepdata_gather: unit %d: track %d, the handle holds %d", u, track[u], (int)h->tracks.size());
    const SdTrack& tr = h->tracks[(size_t)track[u]];
    if (t0[u] < 0 || t0[u] >= tr.Tf) ETD_FAIL(ETD_EINVAL, "sepdata_gather: unit %d: t0 = %lld outside 0 .. %lld of track %d", u, (long long)t0[u], tr.Tf - 1, track[u]);
    if (!std::isfinite(a[u]) || !std::isfinite(q[u]) || !(a[u] > 0.0) || !(q[u] > 0.0) || a[u] > 64.0 || q[u] > 64.0)
      ETD_FAIL(ETD_EINVAL, "sepdata_gather: unit %d: a = %g and q = %g must be finite and in (0, 64]", u, a[u], q[u]);
    const double Tp = floor((double)c.T * a[u]), Fp = floor((double)c.F * q[u]);
    if (Tp < 2.0) ETD_FAIL(ETD_EINVAL, "sepdata_gather: unit %d: T' = floor(%d x %g) = %d is below 2", u, c.T, a[u], (int)Tp);
    if (Fp < 2.0) ETD_FAIL(ETD_EINVAL, "sepdata_gather: unit %d: F' = floor(%d x %g) = %d is below 2", u, c.F, q[u], (int)Fp);
    SdUnit& d = units[(size_t)u];
    d.S = tr.S; d.ks = tr.frames * c.F * c.n_channels; d.Tf = (int)tr.Tf; d.t0 = (int)t0[u]; d.Tp = (int)Tp; d.Fp = (int)Fp;
  }
  hipStream_t st = (hipStream_t)stream;
  if (B > h->units_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    if (h->units_dev) { (void)hipFree(h->units_dev); h->units_dev = nullptr; h->units_cap = 0; }
    HIP_TRY(hipMalloc((void**)&h->units_dev, sizeof(SdUnit) * (size_t)B));
    h->units_cap = B;
  }
  ETD_TRY(upload_table(st, h->units_dev, units));
  const int fblocks = (c.F + SD_THREADS - 1) / SD_THREADS;
  hipLaunchKernelGGL(k_sd_gather, dim3((unsigned)(c.T * fblocks), (unsigned)B), dim3(SD_THREADS), 0, st, h->units_dev, c.T, c.F, c.n_channels, c.n_instr, fblocks,
                     mix_dev, target_dev);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
