// Note renderer: a ragged batch of note lists -> mono fp32 waveforms of this project's own piano voice.  DESIGN.md 4l is the contract; tests/render_np.py
// restates it in fp64 numpy.
//
// Three kernels, no atomics, no sum that depends on scheduling:
//   k_render_prep   one thread per note: f_k / sr, the phase at the note's first sample, A_k and the decay rates of the surviving partials, all formed in fp64
//   k_render        gather: one workgroup per RN_BLOCK consecutive samples of ONE cover, one 16-byte store per thread, zeros included.  A block's candidate notes are
//                   the index range [lo, hi) of its cover's onset-sorted notes (host: two sweeps over monotone arrays, two ints per block); inside the range a note
//                   that misses the block is skipped by a test on workgroup-uniform values.  Per (note, partial, sample) the phase in revolutions is ONE fp64 FMA of
//                   the sample's distance from the note's first sample, reduced to [-0.5, 0.5] in fp64; sine, exponentials and sums are fp32.  A sample adds its
//                   cover's notes in onset order and each note's partials in ascending k, so it does not depend on the batch, the block or the launch.
//   k_render_peaks  one workgroup per cover: max |x|
#include <algorithm>
#include <cmath>
#include <vector>

#include "prof.h"
#include "render.h"
#include "../../include/etude_hip_debug.h"

namespace {

// sin(2 pi r) for |r| <= 0.25 as r P(r^2): the Taylor series through r^13 (the r^15 term is below 7e-10 there), Horner in fp32
__device__ __forceinline__ float rn_sin_rev(float r) {
  constexpr double W = 6.283185307179586476925286766559;
  constexpr double W2 = W * W;
  constexpr float c1 = (float)W;
  constexpr float c3 = (float)(-W * W2 / 6.0);
  constexpr float c5 = (float)(W * W2 * W2 / 120.0);
  constexpr float c7 = (float)(-W * W2 * W2 * W2 / 5040.0);
  constexpr float c9 = (float)(W * W2 * W2 * W2 * W2 / 362880.0);
  constexpr float c11 = (float)(-W * W2 * W2 * W2 * W2 * W2 / 39916800.0);
  constexpr float c13 = (float)(W * W2 * W2 * W2 * W2 * W2 * W2 / 6227020800.0);
  const float z = r * r;
  float p = fmaf(c13, z, c11);
  p = fmaf(p, z, c9);
  p = fmaf(p, z, c7);
  p = fmaf(p, z, c5);
  p = fmaf(p, z, c3);
  p = fmaf(p, z, c1);
  return r * p;
}

__global__ __launch_bounds__(RN_THREADS) void k_render_prep(const RnHead* __restrict__ heads, RnNote* __restrict__ recs, int n_notes, RnVoice v) {
  const int i = (int)(blockIdx.x * RN_THREADS + threadIdx.x);
  if (i >= n_notes) return;
  const RnHead h = heads[i];
  RnNote& r = recs[i];
  r.n_first = h.n_first; r.n_end = h.n_end;
  r.d0 = (double)h.n_first / v.sr - h.onset;
  r.dur = h.offset - h.onset;
  r.pad = 0;
  const double f0 = 440.0 * exp2((double)(h.pitch - 69) / 12.0 + h.cents / 1200.0);
  const double B = v.inharmonicity * exp2((double)(h.pitch - 60) / v.inharmonicity_step);
  const double T = v.decay_base * exp2(-(double)(h.pitch - 21) / v.decay_halving);
  const double av = pow((double)h.velocity / 127.0, v.velocity_power);
  int K = 0;
  for (int k = 1; k <= RN_MAX_PARTIALS; ++k) {
    const double fk = (double)k * f0 * sqrt(1.0 + B * (double)(k * k));
    const bool live = k <= v.partials && fk < v.nyquist_hz && K == k - 1;      // (f_k ascends with k: the survivors are the first K)
    if (live) K = k;
    const double Tk = T / (1.0 + v.decay_partial * (double)(k - 1));
    r.fsr[k - 1] = live ? fk / v.sr : 0.0;
    r.ph0[k - 1] = live ? fk * r.d0 : 0.0;
    r.amp[k - 1] = live ? (float)(av * pow((double)k, -v.partial_rolloff)) : 0.f;
    r.dec[k - 1] = live && v.decay_on ? (float)(-1.4426950408889634074 / Tk) : 0.f;
  }
  r.K = K;
}

__global__ __launch_bounds__(RN_THREADS) void k_render(const RnCover* __restrict__ tab, int n_covers, const int2* __restrict__ ranges, const RnNote* __restrict__ recs,
                                                       float* __restrict__ out, long long blk_base, RnVoice v) {
  const long long b = blk_base + (long long)blockIdx.x;
  const int c = song_of(tab, n_covers, b);
  const long long blk0 = tab[c].blk0, N = tab[c].N;
  const int note0 = tab[c].note0;
  float* dst = out + tab[c].out_off;
  const long long s0 = (b - blk0) * RN_BLOCK, s1 = s0 + RN_BLOCK;      // the block's samples in its cover (s0 < N: the host counted ceil(N / RN_BLOCK) blocks)
  const long long n = s0 + (long long)threadIdx.x * RN_PER_THREAD;
  const int2 rg = ranges[b];
  float acc[RN_PER_THREAD];
#pragma unroll
  for (int j = 0; j < RN_PER_THREAD; ++j) acc[j] = 0.f;

  for (int i = rg.x; i < rg.y; ++i) {
    const RnNote* __restrict__ r = recs + (note0 + i);      // (uniform address: the record arrives through scalar loads)
    const long long nf = r->n_first, ne = r->n_end;
    if (ne <= s0 || nf >= s1) continue;                       // uniform
    const double d0 = r->d0, dur = r->dur;
    const int K = r->K;
    double dn[RN_PER_THREAD];
    float tau[RN_PER_THREAD], g[RN_PER_THREAD], sum[RN_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RN_PER_THREAD; ++j) {
      const long long nj = n + j;
      const bool on = nj >= nf && nj < ne;
      dn[j] = (double)(nj - nf);
      const double td = fma(dn[j], v.inv_sr, d0);             // seconds since the onset, fp64
      tau[j] = fmaxf((float)td, 0.f);
      const float u = (float)(td - dur);                      // seconds since the offset
      const float att = fminf(tau[j] * v.inv_attack, 1.f);
      float rel = 1.f;
      if (v.release_on && u > 0.f) rel = __builtin_amdgcn_exp2f(u * v.rel_c) * fmaxf(1.f - u * v.inv_rel_len, 0.f);
      g[j] = on ? att * rel : 0.f;
      sum[j] = 0.f;
    }
    for (int k = 0; k < K; ++k) {
      const double fsr = r->fsr[k], ph0 = r->ph0[k];
      const float amp = r->amp[k], dk = r->dec[k];
#pragma unroll
      for (int j = 0; j < RN_PER_THREAD; ++j) {
        const double ph = fma(dn[j], fsr, ph0);               // revolutions since the onset
        float fr = (float)(ph - __builtin_rint(ph));          // [-0.5, 0.5], then fp32
        if (fabsf(fr) > 0.25f) fr = copysignf(0.5f, fr) - fr; // exact: sin(2 pi r) = sin(2 pi (+-0.5 - r))
        const float e = __builtin_amdgcn_exp2f(tau[j] * dk);
        sum[j] = fmaf(amp * e, rn_sin_rev(fr), sum[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < RN_PER_THREAD; ++j) acc[j] += g[j] * sum[j];
  }

  if (n + RN_PER_THREAD <= N) {
    f32x4 o = {v.gain * acc[0], v.gain * acc[1], v.gain * acc[2], v.gain * acc[3]};
    *reinterpret_cast<f32x4*>(dst + n) = o;                   // (out_off and n are multiples of 4: 16-byte aligned)
  } else {
#pragma unroll
    for (int j = 0; j < RN_PER_THREAD; ++j)
      if (n + j < N) dst[n + j] = v.gain * acc[j];
  }
}

__global__ __launch_bounds__(RN_THREADS) void k_render_peaks(const float* __restrict__ x, const int64_t* __restrict__ offsets, const int64_t* __restrict__ Ns,
                                                             float* __restrict__ peaks) {
  __shared__ float part[RN_THREADS / 64];
  const float* p = x + offsets[blockIdx.x];
  const long long N = Ns[blockIdx.x];
  const int t = (int)threadIdx.x;
  long long head = (4 - (long long)(((uintptr_t)p >> 2) & 3)) & 3;      // scalar until the pointer is 16-byte aligned
  if (head > N) head = N;
  float m = 0.f;
  if (t < head) m = fabsf(p[t]);
  const long long nv = (N - head) / 4;
  const f32x4* pv = reinterpret_cast<const f32x4*>(p + head);
  for (long long i = t; i < nv; i += RN_THREADS) {
    const f32x4 q = pv[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(q[0]), fabsf(q[1]))), fmaxf(fabsf(q[2]), fabsf(q[3])));
  }
  const long long tail = head + 4 * nv;
  if (tail + t < N) m = fmaxf(m, fabsf(p[tail + t]));
  m = wave_max(m);
  if ((t & 63) == 0) part[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    float r = part[0];
    for (int w = 1; w < RN_THREADS / 64; ++w) r = fmaxf(r, part[w]);
    peaks[blockIdx.x] = r;
  }
}

inline long long rn_blocks(long long N) { return (N + RN_BLOCK - 1) / RN_BLOCK; }
inline long long rn_up(long long x, long long a) { return (x + a - 1) / a * a; }      // (samples to RN_ALIGN; workspace bytes go through ws_align)

}  // namespace

struct etd_render {
  etd_render_cfg cfg;
  RnVoice v;
  double rel_len;                  // R of the support: release_len, or 0 with the release off
  bool used = false;
  std::vector<unsigned char> stage;
};

namespace {

struct RnLayout { long long off_tab, off_rng, off_head, off_rec, upload, total, blocks, notes; };

// what a call is refused for, and where its pieces sit in the workspace
int rn_layout(const etd_render* h, int n_covers, const int64_t* note_off, const int64_t* Ns, RnLayout* L) {
  if (!h || !note_off || !Ns) ETD_FAIL(ETD_EINVAL, "render: null argument");
  if (n_covers < 1 || n_covers > RN_MAX_COVERS) ETD_FAIL(ETD_EINVAL, "render: %d covers in one call (need 1 .. %d)", n_covers, RN_MAX_COVERS);
  if (note_off[0] != 0) ETD_FAIL(ETD_EINVAL, "render: note_offsets_host[0] = %lld (need 0)", (long long)note_off[0]);
  long long blocks = 0;
  for (int b = 0; b < n_covers; ++b) {
    const long long k = note_off[b + 1] - note_off[b];
    if (k < 0) ETD_FAIL(ETD_EINVAL, "render: note_offsets_host decreases at cover %d", b);
    if (k > RN_MAX_NOTES) ETD_FAIL(ETD_EINVAL, "render: cover %d has %lld notes (> %d)", b, k, RN_MAX_NOTES);
    if (Ns[b] < 0 || Ns[b] > RN_MAX_SAMPLES) ETD_FAIL(ETD_EINVAL, "render: cover %d has %lld samples (need 0 .. %lld)", b, (long long)Ns[b], (long long)RN_MAX_SAMPLES);
    blocks += rn_blocks(Ns[b]);
  }
  L->blocks = blocks; L->notes = note_off[n_covers];
  L->off_tab = 0;
  L->off_rng = ws_align((long long)n_covers * (long long)sizeof(RnCover));
  L->off_head = ws_align(L->off_rng + blocks * (long long)sizeof(int2));
  L->upload = L->off_head + L->notes * (long long)sizeof(RnHead);
  L->off_rec = ws_align(L->upload);
  L->total = ws_align(L->off_rec + L->notes * (long long)sizeof(RnNote));
  return ETD_OK;
}

}  // namespace

extern "C" int etd_render_limits(int* max_notes, long long* max_samples, int* max_partials, int* max_covers, int* block) {
  if (max_notes) *max_notes = RN_MAX_NOTES;
  if (max_samples) *max_samples = RN_MAX_SAMPLES;
  if (max_partials) *max_partials = RN_MAX_PARTIALS;
  if (max_covers) *max_covers = RN_MAX_COVERS;
  if (block) *block = RN_BLOCK;
  return ETD_OK;
}

extern "C" int etd_render_create(const etd_render_cfg* cfg, etd_render** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "render_create: null argument");
  ETD_CHECK_CFG(cfg, etd_render_cfg, "render_create");
  if (cfg->sample_rate < 8000 || cfg->sample_rate > 48000) ETD_FAIL(ETD_EINVAL, "render_create: sample_rate = %d (need 8000 .. 48000)", cfg->sample_rate);
  if (cfg->partials < 1 || cfg->partials > RN_MAX_PARTIALS) ETD_FAIL(ETD_EINVAL, "render_create: partials = %d (need 1 .. %d)", cfg->partials, RN_MAX_PARTIALS);
  const double pos[] = {cfg->inharmonicity_step, cfg->attack, cfg->decay_base, cfg->decay_halving, cfg->release_tau, cfg->release_len, cfg->gain, cfg->nyquist_fraction};
  const char* pos_name[] = {"inharmonicity_step", "attack", "decay_base", "decay_halving", "release_tau", "release_len", "gain", "nyquist_fraction"};
  for (int i = 0; i < 8; ++i)
    if (!(pos[i] > 0.0) || !std::isfinite(pos[i])) ETD_FAIL(ETD_EINVAL, "render_create: %s = %g (need a finite value above 0)", pos_name[i], pos[i]);
  const double nonneg[] = {cfg->inharmonicity, cfg->partial_rolloff, cfg->velocity_power, cfg->decay_partial};
  const char* nonneg_name[] = {"inharmonicity", "partial_rolloff", "velocity_power", "decay_partial"};
  for (int i = 0; i < 4; ++i)
    if (!(nonneg[i] >= 0.0) || !std::isfinite(nonneg[i])) ETD_FAIL(ETD_EINVAL, "render_create: %s = %g (need a finite value, 0 or above)", nonneg_name[i], nonneg[i]);
  if (cfg->nyquist_fraction > 0.5) ETD_FAIL(ETD_EINVAL, "render_create: nyquist_fraction = %g (need at most 0.5)", cfg->nyquist_fraction);
  if (cfg->release_len > 60.0) ETD_FAIL(ETD_EINVAL, "render_create: release_len = %g s (need at most 60)", cfg->release_len);
  etd_render* h = new etd_render();
  h->cfg = *cfg;
  RnVoice& v = h->v;
  v.sr = (double)cfg->sample_rate; v.inv_sr = 1.0 / v.sr;
  v.inharmonicity = cfg->inharmonicity; v.inharmonicity_step = cfg->inharmonicity_step; v.partial_rolloff = cfg->partial_rolloff; v.velocity_power = cfg->velocity_power;
  v.decay_base = cfg->decay_base; v.decay_halving = cfg->decay_halving; v.decay_partial = cfg->decay_partial; v.nyquist_hz = cfg->nyquist_fraction * v.sr;
  v.inv_attack = (float)(1.0 / cfg->attack); v.rel_c = (float)(-1.4426950408889634074 / cfg->release_tau); v.inv_rel_len = (float)(1.0 / cfg->release_len);
  v.gain = (float)cfg->gain;
  v.partials = cfg->partials; v.decay_on = cfg->flags & 1; v.release_on = (cfg->flags >> 1) & 1;
  h->rel_len = v.release_on ? cfg->release_len : 0.0;
  *out = h;
  return ETD_OK;
}

extern "C" void etd_render_destroy(etd_render* h) {
  if (!h) return;
  if (h->used) (void)hipDeviceSynchronize();      // kernels of this handle may still be in flight
  delete h;
}

extern "C" long long etd_render_bytes(const etd_render* h, int n_covers, const int64_t* note_offsets_host, const int64_t* num_samples_host) {
  RnLayout L;
  const int rc = rn_layout(h, n_covers, note_offsets_host, num_samples_host, &L);
  return rc != ETD_OK ? (long long)rc : L.total;
}

namespace {

// everything a call is refused for, then the plan in h->stage: cover table, per-note heads (which samples a note sounds on), per-block candidate ranges
int rn_plan(etd_render* h, const etd_note* notes_host, const int64_t* note_offsets_host, const double* cents_host, int n_covers, const int64_t* num_samples_host,
            const int64_t* sample_offsets_host, RnLayout* Lp) {
  RnLayout& L = *Lp;
  ETD_TRY(rn_layout(h, n_covers, note_offsets_host, num_samples_host, &L));
  if (!sample_offsets_host) ETD_FAIL(ETD_EINVAL, "render: null sample_offsets_host");
  if (L.notes > 0 && !notes_host) ETD_FAIL(ETD_EINVAL, "render: null notes_host");
  const double sr = h->v.sr, R = h->rel_len;
  long long end = 0;
  for (int b = 0; b < n_covers; ++b) {
    const long long off = sample_offsets_host[b];
    if (off < end || off % 4) ETD_FAIL(ETD_EINVAL, "render: cover %d starts at sample %lld of the flat buffer (need a multiple of 4 at or behind the previous cover's end %lld)", b, off, end);
    end = off + num_samples_host[b];
    if (cents_host && !(std::fabs(cents_host[b]) <= 50.0)) ETD_FAIL(ETD_EINVAL, "render: cover %d: tuning of %g cents (need |c| <= 50)", b, cents_host[b]);
    double prev = 0.0;
    for (long long i = note_offsets_host[b]; i < note_offsets_host[b + 1]; ++i) {
      const etd_note& q = notes_host[i];
      const long long k = i - note_offsets_host[b];
      if (!std::isfinite(q.onset) || !std::isfinite(q.offset) || q.onset < 0.0 || !(q.offset > q.onset))
        ETD_FAIL(ETD_EINVAL, "render: cover %d, note %lld: onset %g, offset %g (need finite times, 0 <= onset < offset)", b, k, q.onset, q.offset);
      if ((q.offset + R) * sr > 9.0e15) ETD_FAIL(ETD_EINVAL, "render: cover %d, note %lld: offset %g s is beyond any sample index", b, k, q.offset);
      if (q.pitch < 21 || q.pitch > 108) ETD_FAIL(ETD_EINVAL, "render: cover %d, note %lld: pitch %d (need 21 .. 108)", b, k, q.pitch);
      if (q.velocity < 1 || q.velocity > 127) ETD_FAIL(ETD_EINVAL, "render: cover %d, note %lld: velocity %d (need 1 .. 127)", b, k, q.velocity);
      if (q.onset < prev) ETD_FAIL(ETD_EINVAL, "render: cover %d, note %lld: onset %g is before its predecessor's %g (sort the notes by onset, stably)", b, k, q.onset, prev);
      prev = q.onset;
    }
  }
  h->stage.assign((size_t)L.upload, 0);
  RnCover* tab = reinterpret_cast<RnCover*>(h->stage.data() + L.off_tab);
  int2* rng = reinterpret_cast<int2*>(h->stage.data() + L.off_rng);
  RnHead* heads = reinterpret_cast<RnHead*>(h->stage.data() + L.off_head);
  std::vector<long long> runmax;
  long long blk = 0;
  for (int b = 0; b < n_covers; ++b) {
    const long long i0 = note_offsets_host[b], k = note_offsets_host[b + 1] - i0, N = num_samples_host[b], nb = rn_blocks(N);
    tab[b].blk0 = blk; tab[b].out_off = sample_offsets_host[b]; tab[b].N = N; tab[b].note0 = (int)i0; tab[b].n_notes = (int)k;
    runmax.resize((size_t)k);
    for (long long i = 0; i < k; ++i) {
      const etd_note& q = notes_host[i0 + i];
      RnHead& hd = heads[i0 + i];
      hd.onset = q.onset; hd.offset = q.offset; hd.cents = cents_host ? cents_host[b] : 0.0; hd.pitch = q.pitch; hd.velocity = q.velocity;
      long long nf = (long long)std::ceil(q.onset * sr);      // a first guess, then the restatement's own predicates decide
      if (nf < 0) nf = 0;
      while ((double)nf / sr < q.onset) ++nf;
      while (nf > 0 && (double)(nf - 1) / sr >= q.onset) --nf;
      long long ne = (long long)std::ceil((q.offset + R) * sr);
      if (ne < 0) ne = 0;
      while ((double)ne / sr - q.offset < R) ++ne;
      while (ne > 0 && (double)(ne - 1) / sr - q.offset >= R) --ne;
      if (ne < nf) ne = nf;
      hd.n_first = nf; hd.n_end = ne;
      runmax[(size_t)i] = i ? std::max(runmax[(size_t)i - 1], ne) : ne;
    }
    // candidates of the block [s0, s1): hi = the first note with n_first >= s1, lo = the first index at which the running maximum of n_end exceeds s0
    long long lo = 0, hi = 0;
    for (long long j = 0; j < nb; ++j) {
      const long long s0 = j * RN_BLOCK, s1 = s0 + RN_BLOCK;
      while (hi < k && heads[i0 + hi].n_first < s1) ++hi;
      while (lo < k && runmax[(size_t)lo] <= s0) ++lo;
      rng[blk + j].x = (int)std::min(lo, hi); rng[blk + j].y = (int)hi;
    }
    blk += nb;
  }
  return ETD_OK;
}

}  // namespace

extern "C" int etd_render_debug_plan(etd_render* h, const etd_note* notes_host, const int64_t* note_offsets_host, int n_covers, const int64_t* num_samples_host,
                                     int64_t* first_end_host, int32_t* ranges_host) {
  if (!h || !num_samples_host) ETD_FAIL(ETD_EINVAL, "render_debug_plan: null argument");
  std::vector<int64_t> offs((size_t)(n_covers > 0 && n_covers <= RN_MAX_COVERS ? n_covers : 0));
  long long end = 0;
  for (size_t b = 0; b < offs.size(); ++b) { offs[b] = end; end += rn_up(num_samples_host[b] > 0 ? num_samples_host[b] : 0, RN_ALIGN); }
  RnLayout L;
  ETD_TRY(rn_plan(h, notes_host, note_offsets_host, nullptr, n_covers, num_samples_host, offs.data(), &L));
  const int2* rng = reinterpret_cast<const int2*>(h->stage.data() + L.off_rng);
  const RnHead* heads = reinterpret_cast<const RnHead*>(h->stage.data() + L.off_head);
  for (long long i = 0; first_end_host && i < L.notes; ++i) { first_end_host[2 * i] = heads[i].n_first; first_end_host[2 * i + 1] = heads[i].n_end; }
  for (long long j = 0; ranges_host && j < L.blocks; ++j) { ranges_host[2 * j] = rng[j].x; ranges_host[2 * j + 1] = rng[j].y; }
  return ETD_OK;
}

extern "C" int etd_render_run(etd_render* h, const etd_note* notes_host, const int64_t* note_offsets_host, const double* cents_host, int n_covers,
                              const int64_t* num_samples_host, const int64_t* sample_offsets_host, float* out_dev, void* workspace_dev, long long workspace_bytes,
                              void* stream) {
  RnLayout L;
  ETD_TRY(rn_layout(h, n_covers, note_offsets_host, num_samples_host, &L));
  if (L.blocks > 0) {
    if (!out_dev || !workspace_dev) ETD_FAIL(ETD_EINVAL, "render_run: null out_dev or workspace_dev");
    if (workspace_bytes < L.total) ETD_FAIL(ETD_EINVAL, "render_run: the workspace holds %lld bytes, the call needs %lld (etd_render_bytes)", workspace_bytes, L.total);
    if ((uintptr_t)out_dev % 16 || (uintptr_t)workspace_dev % 16) ETD_FAIL(ETD_EINVAL, "render_run: out_dev and workspace_dev must be 16-byte aligned");
  }
  ETD_TRY(rn_plan(h, notes_host, note_offsets_host, cents_host, n_covers, num_samples_host, sample_offsets_host, &L));
  if (L.blocks == 0) return ETD_OK;                // nothing to write
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace_dev;
  ETD_TRY(upload_table(st, ws, h->stage));          // (rn_plan sized the stage to L.upload bytes)
  h->used = true;
  RnNote* recs = reinterpret_cast<RnNote*>(ws + L.off_rec);
  if (L.notes > 0) {
    ProfScope ps("k_render_prep", st, 0, (double)L.notes * (double)(sizeof(RnHead) + sizeof(RnNote)));
    hipLaunchKernelGGL(k_render_prep, dim3((unsigned)((L.notes + RN_THREADS - 1) / RN_THREADS)), dim3(RN_THREADS), 0, st,
                       reinterpret_cast<const RnHead*>(ws + L.off_head), recs, (int)L.notes, h->v);
    HIP_TRY(hipGetLastError());
  }
  for (long long b0 = 0; b0 < L.blocks; b0 += RN_MAX_LAUNCH_BLOCKS) {
    const long long nb = std::min<long long>(RN_MAX_LAUNCH_BLOCKS, L.blocks - b0);
    ProfScope ps("k_render", st, 0, (double)nb * RN_BLOCK * 4.0);
    hipLaunchKernelGGL(k_render, dim3((unsigned)nb), dim3(RN_THREADS), 0, st, reinterpret_cast<const RnCover*>(ws + L.off_tab), n_covers,
                       reinterpret_cast<const int2*>(ws + L.off_rng), recs, out_dev, b0, h->v);
    HIP_TRY(hipGetLastError());
  }
  return ETD_OK;
}

extern "C" int etd_render_peaks(etd_render* h, const float* samples_dev, const int64_t* sample_offsets_dev, const int64_t* num_samples_dev, int n_covers, float* peaks_dev,
                                void* stream) {
  if (!h || !sample_offsets_dev || !num_samples_dev || !peaks_dev) ETD_FAIL(ETD_EINVAL, "render_peaks: null argument");
  if (n_covers < 1 || n_covers > RN_MAX_COVERS) ETD_FAIL(ETD_EINVAL, "render_peaks: %d covers in one call (need 1 .. %d)", n_covers, RN_MAX_COVERS);
  hipStream_t st = (hipStream_t)stream;
  h->used = true;
  {
    ProfScope ps("k_render_peaks", st);
    hipLaunchKernelGGL(k_render_peaks, dim3((unsigned)n_covers), dim3(RN_THREADS), 0, st, samples_dev, sample_offsets_dev, num_samples_dev, peaks_dev);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
