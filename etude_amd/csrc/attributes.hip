// Bar attributes on the GPU: a ragged batch of (condition bar, target bar) pairs of token ids -> the six counts of EtudeDataset._extract_bar_features, the four relative
// attributes of _compute_musical_attributes (etude/data/dataset.py:204-270) and, with edges, their np.digitize bins.  DESIGN.md 4i is the contract; tests/attributes_np.py
// restates it in plain Python and fp64 numpy.
//
// ONE launch per batch, one wavefront per pair, AT_WAVES pairs per workgroup.  A wavefront walks its two bars in chunks of 64 tokens: a ballot of the Pos tokens and one
// cross-lane read give every token the value of the last Pos at or before it (the chunk's last one is carried into the next chunk), counts are popcounts of ballots, and
// the notes go into the wavefront's own table in LDS, one 8-byte entry per Pos value the vocabulary holds: the 12-bit pitch-class mask of the source notes (atomic or) and
// the target's note and overlap counts, 16 bits each in one word (atomic add).  Integer atomics only: their result does not depend on the order.  The entries that hold a
// note are then compacted in place, in ascending Pos value, into their ratios, and ONE lane adds them in numpy's order and forms the four attributes.  No __syncthreads:
// the wavefronts of a workgroup share nothing, so a pair's numbers depend on its two bars alone: bit-identical alone, in any batch and from run to run.
#include "attributes.h"
#include "prof.h"
#include "np_sum.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

// LDS writes of this wavefront before, reads after (the lanes of one wavefront run in lockstep; this keeps the compiler from moving accesses across)
__device__ __forceinline__ void at_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int at_wave_add(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One bar: tokens ids[0 .. n).  M: the wavefront's table as 32-bit words (2 p: mask, 2 p + 1: counts).  Every lane returns the bar's counts; bad: a lane met an id outside [0, V).
template <bool TGT>
__device__ __forceinline__ void at_bar(const AtArgs& a, const int32_t* ids, int n, unsigned* M, int lane, int& notes, int& poss, int& dur, bool& bad) {
  int carry = -1;                                            // the reference's current_pos
  int d = 0;
  notes = 0; poss = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {                       // (n is uniform: every lane runs every chunk)
    const int i = c0 + lane;
    int ty = -1, val = 0;
    if (i < n) {
      const int id = ids[i];
      if (id >= 0 && id < a.V) { const int2 e = a.table[id]; ty = e.x; val = e.y; }
      else bad = true;
    }
    const u64 pm = __ballot(ty == a.ty_pos);
    const u64 below = pm & ((2ULL << lane) - 1ULL);          // the Pos tokens at or before this lane (lane 63: the shift wraps to 0, the mask is all ones)
    const int from_lane = below ? 63 - __clzll((long long)below) : 0;
    const int pv = __shfl(val, from_lane, 64);
    const int cur = below ? pv : carry;
    const int last_lane = pm ? 63 - __clzll((long long)pm) : 0;
    const int lv = __shfl(val, last_lane, 64);
    if (pm) carry = lv;
    poss += __popcll(pm);
    const bool is_note = ty == a.ty_note && cur != -1;
    notes += __popcll(__ballot(is_note));
    if (ty == a.ty_dur) d += val;
    if (is_note) {
      const unsigned p = (unsigned)(cur - a.pos_min);
      if (p < (unsigned)a.npos) {                            // (always: the table spans every Pos value of the vocabulary)
        const int pc = ((val % 12) + 12) % 12;               // Python's %
        if (!TGT) atomicOr(&M[2 * p], 1u << pc);
        else atomicAdd(&M[2 * p + 1], 1u + (((M[2 * p] >> pc) & 1u) << 16));
      }
    }
  }
  dur = at_wave_add(d);
}

__device__ __forceinline__ double at_idiv(int n, int d) { return d ? (double)n / (double)d : 0.0; }                  // safe_div(int, int)
__device__ __forceinline__ double at_fdiv1(double n, double d) { return d != 0.0 ? n / d : 1.0; }                    // safe_div(float, float, default=1.0)

__global__ __launch_bounds__(AT_THREADS) void k_attr(const AtArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char at_lds[];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const long long pair = (long long)blockIdx.x * AT_WAVES + w;
  if (pair >= a.n_pairs) return;                             // (the whole wavefront)
  u64* T = (u64*)at_lds + (size_t)w * a.npos;
  unsigned* M = (unsigned*)T;
  for (int p = lane; p < a.npos; p += 64) T[p] = 0;
  int st = 0;
  // the two bars of the pair
  long long sb = a.src_idx ? (long long)a.src_idx[pair] : pair, tb = a.tgt_idx ? (long long)a.tgt_idx[pair] : pair;
  long long so = 0, to = 0;
  int sn_tok = 0, tn_tok = 0;
  if (sb < 0 || sb >= a.n_src) st |= AT_BAD_INDEX;
  else { so = a.src_off[sb]; sn_tok = (int)(a.src_off[sb + 1] - so); }
  if (tb < 0 || tb >= a.n_tgt) st |= AT_BAD_INDEX;
  else { to = a.tgt_off[tb]; tn_tok = (int)(a.tgt_off[tb + 1] - to); }
  sn_tok = sn_tok < 0 ? 0 : (sn_tok > AT_MAX_TOKENS ? AT_MAX_TOKENS : sn_tok);      // (the host check refuses both; the kernel still stays inside its table's counts)
  tn_tok = tn_tok < 0 ? 0 : (tn_tok > AT_MAX_TOKENS ? AT_MAX_TOKENS : tn_tok);
  at_wave_sync();
  bool bad = false;
  int s_notes, s_pos, s_dur, t_notes, t_pos, t_dur;
  at_bar<false>(a, a.src_ids + so, sn_tok, M, lane, s_notes, s_pos, s_dur, bad);
  at_wave_sync();                                            // the masks are complete before the target's notes read them
  at_bar<true>(a, a.tgt_ids + to, tn_tok, M, lane, t_notes, t_pos, t_dur, bad);
  at_wave_sync();
  if (__ballot(bad)) st |= AT_BAD_ID;
  // the positions that hold a note, ascending, compacted in place into their ratios (entry k <= p is written after entry p was read)
  int n_pos = 0;
  for (int c0 = 0; c0 < a.npos; c0 += 64) {
    const int p = c0 + lane;
    const u64 e = p < a.npos ? T[p] : 0;
    const unsigned mask = (unsigned)e, tc = (unsigned)(e >> 32) & 0xffffu, ov = (unsigned)(e >> 48);
    const bool key = mask != 0 || tc != 0;
    const u64 km = __ballot(key);
    at_wave_sync();
    if (key) {
      const int k = n_pos + __popcll(km & ((1ULL << lane) - 1ULL));
      const double r = tc ? (double)ov / (double)tc : 0.0;   // only the source holds it: 0.0
      T[k] = (u64)__double_as_longlong(r);
    }
    n_pos += __popcll(km);
    at_wave_sync();
  }
  if (lane == 0) {
    double overlap = 0.0;
    if (n_pos > 0) overlap = np_sum_all(n_pos, [&](int i) { return __longlong_as_double((long long)T[i]); }) / (double)n_pos;      // np.mean
    double v[4];
    v[0] = at_fdiv1(at_idiv(t_notes, t_pos), at_idiv(s_notes, s_pos));
    v[1] = s_pos ? (double)t_pos / (double)s_pos : 1.0;
    v[2] = at_fdiv1(at_idiv(t_dur, t_notes), at_idiv(s_dur, s_notes));
    v[3] = overlap;
    int32_t* f = a.feat + 6 * pair;
    f[0] = s_notes; f[1] = s_pos; f[2] = s_dur; f[3] = t_notes; f[4] = t_pos; f[5] = t_dur;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.attr[4 * pair + j] = v[j];
    if (a.bins) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int b = 1;                                           // no edges: the reference's default bin
        if (a.n_edges[j] > 0) {
          b = 0;                                             // np.digitize(right=False) on ascending edges: the edges that are not above the value
#pragma unroll
          for (int q = 0; q < AT_MAX_EDGES; ++q) b += (q < a.n_edges[j] && !(v[j] < a.edges[j][q])) ? 1 : 0;
        }
        a.bins[4 * pair + j] = b;
      }
    }
    a.status[pair] = st | (n_pos << AT_NPOS_SHIFT);
  }
}

}  // namespace

struct etd_attr {
  etd_attr_cfg cfg;
  std::vector<int32_t> table;      // (type, value) pairs
  int V = 0, pos_min = 0, npos = 1;
  int2* table_dev = nullptr;
  bool attr_set = false;
};

extern "C" int etd_attr_limits(int* max_bar_tokens, int* max_pairs, int* max_pos_range, int* max_edges) {
  if (max_bar_tokens) *max_bar_tokens = AT_MAX_TOKENS;
  if (max_pairs) *max_pairs = AT_MAX_PAIRS;
  if (max_pos_range) *max_pos_range = AT_MAX_POS_RANGE;
  if (max_edges) *max_edges = AT_MAX_EDGES;
  return ETD_OK;
}

extern "C" int etd_attr_create(const etd_attr_cfg* cfg, const int32_t* event_table_host, int vocab_size, etd_attr** out) {
  if (!cfg || !event_table_host || !out) ETD_FAIL(ETD_EINVAL, "attr_create: null argument");
  ETD_CHECK_CFG(cfg, etd_attr_cfg, "attr_create");
  if (vocab_size < 1) ETD_FAIL(ETD_EINVAL, "attr_create: vocab_size = %d (need >= 1)", vocab_size);
  if (cfg->type_pos < 0 || cfg->type_note < 0 || cfg->type_duration < 0 || cfg->type_pos == cfg->type_note || cfg->type_pos == cfg->type_duration || cfg->type_note == cfg->type_duration)
    ETD_FAIL(ETD_EINVAL, "attr_create: the event types of Pos, Note and Duration must be three different codes >= 0 (got %d, %d, %d)", cfg->type_pos, cfg->type_note, cfg->type_duration);
  long long lo = 0, hi = 0, dmax = 0;
  bool any = false;
  for (int i = 0; i < vocab_size; ++i) {
    const long long ty = event_table_host[2 * i], v = event_table_host[2 * i + 1];
    if (ty == cfg->type_pos) {
      if (!any || v < lo) lo = v;
      if (!any || v > hi) hi = v;
      any = true;
    } else if (ty == cfg->type_duration) {
      const long long m = v < 0 ? -v : v;
      if (m > dmax) dmax = m;
    }
  }
  if (any && hi - lo + 1 > AT_MAX_POS_RANGE)
    ETD_FAIL(ETD_EINVAL, "attr_create: the vocabulary's Pos values span %lld .. %lld, %lld values (> %d, what a pair's table in LDS holds)", lo, hi, hi - lo + 1, AT_MAX_POS_RANGE);
  if (dmax * AT_MAX_TOKENS > 2147483647LL)
    ETD_FAIL(ETD_EINVAL, "attr_create: a Duration value of %lld times %d tokens leaves the int32 total_duration_in_16ths", dmax, AT_MAX_TOKENS);
  etd_attr* h = new etd_attr();
  h->cfg = *cfg;
  h->V = vocab_size;
  h->table.assign(event_table_host, event_table_host + 2 * (size_t)vocab_size);
  h->pos_min = any ? (int)lo : 0;
  h->npos = any ? (int)(hi - lo + 1) : 1;
  // the table goes to the device now where there is one (run allocates nothing); without a GPU the handle still serves etd_attr_check
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
    auto fail = [&](int rc) { if (h->table_dev) (void)hipFree(h->table_dev); delete h; return rc; };
    ETD_TRY_OR(fail, ETD_HIP_RC(hipMalloc((void**)&h->table_dev, sizeof(int2) * (size_t)vocab_size)));
    ETD_TRY_OR(fail, ETD_HIP_RC(hipMemcpy(h->table_dev, h->table.data(), sizeof(int2) * (size_t)vocab_size, hipMemcpyHostToDevice)));
  } else {
    (void)hipGetLastError();
  }
  *out = h;
  return ETD_OK;
}

extern "C" void etd_attr_destroy(etd_attr* h) {
  if (!h) return;
  if (h->attr_set) (void)hipDeviceSynchronize();      // kernels of this handle may still be in flight
  if (h->table_dev) (void)hipFree(h->table_dev);
  delete h;
}

extern "C" int etd_attr_check(const etd_attr* h, const int64_t* offsets_host, int n_bars) {
  if (!h || !offsets_host) ETD_FAIL(ETD_EINVAL, "attr: null argument");
  if (n_bars < 1 || n_bars > AT_MAX_PAIRS) ETD_FAIL(ETD_EINVAL, "attr: %d bars in one call (need 1 .. %d)", n_bars, AT_MAX_PAIRS);
  if (offsets_host[0] != 0) ETD_FAIL(ETD_EINVAL, "attr: offsets_host[0] = %lld (need 0)", (long long)offsets_host[0]);
  for (int b = 0; b < n_bars; ++b) {
    const long long n = offsets_host[b + 1] - offsets_host[b];
    if (n < 0) ETD_FAIL(ETD_EINVAL, "attr: offsets_host decreases at bar %d", b);
    if (n > AT_MAX_TOKENS) ETD_FAIL(ETD_EINVAL, "attr: bar %d has %lld tokens (> %d, what a position's 16-bit counts hold)", b, n, AT_MAX_TOKENS);
  }
  return ETD_OK;
}

extern "C" int etd_attr_run(etd_attr* h, const int32_t* src_ids_dev, const int64_t* src_offsets_dev, const int64_t* src_offsets_host, int n_src_bars,
                            const int32_t* src_index_dev, const int32_t* tgt_ids_dev, const int64_t* tgt_offsets_dev, const int64_t* tgt_offsets_host, int n_tgt_bars,
                            const int32_t* tgt_index_dev, int n_pairs, const double* edges_host, const int32_t* n_edges_host, int32_t* features_dev, double* attributes_dev,
                            int32_t* bins_dev, int32_t* status_dev, void* stream) {
  if (!h || !src_offsets_dev || !src_offsets_host || !tgt_offsets_dev || !tgt_offsets_host) ETD_FAIL(ETD_EINVAL, "attr_run: null argument");
  if (!features_dev || !attributes_dev || !status_dev) ETD_FAIL(ETD_EINVAL, "attr_run: null output (features_dev, attributes_dev and status_dev are all written)");
  if (n_pairs < 1 || n_pairs > AT_MAX_PAIRS) ETD_FAIL(ETD_EINVAL, "attr_run: %d pairs in one call (need 1 .. %d)", n_pairs, AT_MAX_PAIRS);
  ETD_TRY(etd_attr_check(h, src_offsets_host, n_src_bars));
  ETD_TRY(etd_attr_check(h, tgt_offsets_host, n_tgt_bars));
  if (!src_index_dev && n_src_bars != n_pairs) ETD_FAIL(ETD_EINVAL, "attr_run: %d source bars for %d pairs and no src_index_dev", n_src_bars, n_pairs);
  if (!tgt_index_dev && n_tgt_bars != n_pairs) ETD_FAIL(ETD_EINVAL, "attr_run: %d target bars for %d pairs and no tgt_index_dev", n_tgt_bars, n_pairs);
  if ((src_offsets_host[n_src_bars] > 0 && !src_ids_dev) || (tgt_offsets_host[n_tgt_bars] > 0 && !tgt_ids_dev)) ETD_FAIL(ETD_EINVAL, "attr_run: null ids");
  if ((edges_host != nullptr) != (bins_dev != nullptr) || (edges_host && !n_edges_host))
    ETD_FAIL(ETD_EINVAL, "attr_run: edges_host, n_edges_host and bins_dev go together: all three, or none for raw values only");
  AtArgs a;
  memset(&a, 0, sizeof(a));
  if (edges_host) {
    for (int j = 0; j < 4; ++j) {
      const int n = n_edges_host[j];
      if (n < 0 || n > AT_MAX_EDGES) ETD_FAIL(ETD_EINVAL, "attr_run: attribute %d has %d edges (need 0 .. %d)", j, n, AT_MAX_EDGES);
      for (int q = 0; q < n; ++q) {
        const double e = edges_host[AT_MAX_EDGES * j + q];
        if (!std::isfinite(e) || (q > 0 && !(e > edges_host[AT_MAX_EDGES * j + q - 1])))
          ETD_FAIL(ETD_EINVAL, "attr_run: the edges of attribute %d must be finite and ascending (np.unique's output)", j);
        a.edges[j][q] = e;
      }
      a.n_edges[j] = n;
    }
  }
  if (!h->table_dev) ETD_FAIL(ETD_EINVAL, "attr_run: this handle was created without a GPU (its event table is on the host only); create it where the device is");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)AT_WAVES * 8 * (size_t)h->npos;
  if (!h->attr_set) {
    // a wide vocabulary needs more dynamic LDS than the 64 KB a launch gets without saying so
    if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void*)k_attr, hipFuncAttributeMaxDynamicSharedMemorySize, AT_WAVES * 8 * AT_MAX_POS_RANGE));
    h->attr_set = true;
  }
  a.src_ids = src_ids_dev; a.src_off = src_offsets_dev; a.src_idx = src_index_dev; a.n_src = n_src_bars;
  a.tgt_ids = tgt_ids_dev; a.tgt_off = tgt_offsets_dev; a.tgt_idx = tgt_index_dev; a.n_tgt = n_tgt_bars;
  a.table = h->table_dev; a.V = h->V; a.pos_min = h->pos_min; a.npos = h->npos; a.n_pairs = n_pairs;
  a.ty_pos = h->cfg.type_pos; a.ty_note = h->cfg.type_note; a.ty_dur = h->cfg.type_duration;
  a.feat = features_dev; a.attr = attributes_dev; a.bins = bins_dev; a.status = status_dev;
  {
    ProfScope ps("k_attr", st, 0, (double)(src_offsets_host[n_src_bars] + tgt_offsets_host[n_tgt_bars]) * 4.0 + 76.0 * n_pairs);
    hipLaunchKernelGGL(k_attr, dim3((unsigned)((n_pairs + AT_WAVES - 1) / AT_WAVES)), dim3(AT_THREADS), lds, st, a);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
