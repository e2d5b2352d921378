// Host tables of the DBN trackers: state space, transition and observation model of madmom 0.16's beat / bar HMMs, restated from its published
// description.  Plain C++: etd_dbn_describe and etd_dbn_workspace_bytes run without a GPU.  Every transcendental is libm's (exp / log / pow on one double at a
// time) and every sum runs left to right, so the tables are reproducible by `math.exp` / `math.log` arithmetic (tests/dbn_np.py).
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.h"
#include "dbn.h"

namespace {
// intervals of one beat: arange(round(min), round(max) + 1) (round half to even), or the log-spaced subset of num_tempi entries
int dbn_intervals(const etd_dbn_cfg* c, std::vector<int32_t>& ivl) {
  const double min_interval = 60.0 * c->fps / c->max_bpm, max_interval = 60.0 * c->fps / c->min_bpm;
  const long long lo = (long long)std::nearbyint(min_interval), hi = (long long)std::nearbyint(max_interval);
  if (lo < 1) ETD_FAIL(ETD_EINVAL, "dbn: max_bpm %g at %g fps gives a shortest beat interval of %lld frames (need >= 1)", c->max_bpm, c->fps, lo);
  if (hi - lo + 1 > 100000) ETD_FAIL(ETD_EINVAL, "dbn: %lld intervals per beat (min_bpm %g at %g fps)", hi - lo + 1, c->min_bpm, c->fps);
  ivl.clear();
  for (long long i = lo; i <= hi; ++i) ivl.push_back((int32_t)i);
  if (c->num_tempi > 0 && c->num_tempi < (int)ivl.size()) {
    const double a = std::log2(min_interval), b = std::log2(max_interval);
    for (int n = c->num_tempi;; ++n) {
      std::vector<int32_t> u;
      const double step = n > 1 ? (b - a) / (double)(n - 1) : 0.0;
      for (int k = 0; k < n; ++k) {
        const double y = (k == n - 1 && n > 1) ? b : (double)k * step + a;          // numpy.linspace: the last sample is `stop` itself
        u.push_back((int32_t)std::nearbyint(std::pow(2.0, y)));
      }
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      if ((int)u.size() >= c->num_tempi) { ivl = u; break; }
    }
  }
  return ETD_OK;
}

void dbn_fill(DbnHmm& h, const std::vector<int32_t>& ivl, int num_beats, double tlambda, double olambda) {
  const double ninf = -std::numeric_limits<double>::infinity();
  h.num_beats = num_beats;
  h.n_int = (int)ivl.size();
  h.ivl = ivl;
  h.first.resize(h.n_int);
  int s = 0;
  for (int j = 0; j < h.n_int; ++j) { h.first[j] = s; s += ivl[j]; }
  h.per_beat = s;
  h.S = s * num_beats;
  h.init = std::log(1.0 / (double)h.S);
  // transitions between beats: exp(-lambda |to / from - 1|), entries <= spacing(1) are no edge, every from-row normalised
  const int n = h.n_int;
  h.lt.assign((size_t)n * n, ninf);
  h.flo.assign(n, n); h.fhi.assign(n, -1);
  std::vector<double> row(n);
  for (int f = 0; f < n; ++f) {
    double sum = 0.0;
    for (int t = 0; t < n; ++t) {
      double p = std::exp(-tlambda * std::fabs((double)ivl[t] / (double)ivl[f] - 1.0));
      if (p <= std::numeric_limits<double>::epsilon()) p = 0.0;
      row[t] = p;
      sum += p;
    }
    for (int t = 0; t < n; ++t) {
      if (row[t] == 0.0) continue;
      h.lt[(size_t)t * n + f] = std::log(row[t] / sum);
      h.flo[t] = std::min(h.flo[t], f);
      h.fhi[t] = std::max(h.fhi[t], f);
    }
  }
  // positions and observation pointers
  const double border = 1.0 / olambda;
  h.ptr.assign(h.S, 0); h.beatno.assign(h.S, 0); h.chain.assign(h.S, 0);
  for (int b = 0; b < num_beats; ++b)
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < ivl[j]; ++k) {
        const int st = b * h.per_beat + h.first[j] + k;
        const double pos = (double)k / (double)ivl[j] + (double)b;
        uint8_t p = 0;
        if (h.K == 2) p = pos < border ? 1 : 0;
        else { if (std::fmod(pos, 1.0) < border) p = 1; if (pos < border) p = 2; }
        h.ptr[st] = p;
        h.beatno[st] = (uint8_t)((int)pos + 1);
        h.chain[st] = (uint16_t)(b * n + j);
      }
}
}  // namespace

int dbn_build(const etd_dbn_cfg* c, std::vector<DbnHmm>& out, bool device_limits) {
  if (!c) ETD_FAIL(ETD_EINVAL, "dbn: null config");
  if (c->struct_bytes != (int)sizeof(etd_dbn_cfg)) ETD_FAIL(ETD_EINVAL, "dbn: etd_dbn_cfg is %d bytes for the caller, %d here", c->struct_bytes, (int)sizeof(etd_dbn_cfg));
  if (!(c->fps > 0.0) || !std::isfinite(c->fps)) ETD_FAIL(ETD_EINVAL, "dbn: fps must be positive, got %g", c->fps);
  if (!(c->min_bpm > 0.0) || !std::isfinite(c->max_bpm) || !(c->min_bpm < c->max_bpm)) ETD_FAIL(ETD_EINVAL, "dbn: need 0 < min_bpm < max_bpm, got %g and %g", c->min_bpm, c->max_bpm);
  if (!(c->observation_lambda > 1.0) || !std::isfinite(c->observation_lambda)) ETD_FAIL(ETD_EINVAL, "dbn: observation_lambda must be > 1, got %g", c->observation_lambda);
  if (!(c->transition_lambda >= 0.0) || !std::isfinite(c->transition_lambda)) ETD_FAIL(ETD_EINVAL, "dbn: transition_lambda must be >= 0, got %g", c->transition_lambda);
  if (!(c->threshold >= 0.0) || !std::isfinite(c->threshold)) ETD_FAIL(ETD_EINVAL, "dbn: threshold must be >= 0, got %g", c->threshold);
  if (c->correct != 1) ETD_FAIL(ETD_EINVAL, "dbn: only correct = 1 is implemented");
  if (c->num_tempi < 0) ETD_FAIL(ETD_EINVAL, "dbn: num_tempi must be >= 0");
  if (c->n_bars < 0 || c->n_bars > 8) ETD_FAIL(ETD_EINVAL, "dbn: n_bars must be 0..8, got %d", c->n_bars);
  for (int i = 0; i < c->n_bars; ++i)
    if (c->beats_per_bar[i] < 1 || c->beats_per_bar[i] > 8) ETD_FAIL(ETD_EINVAL, "dbn: beats_per_bar[%d] = %d is outside 1..8", i, c->beats_per_bar[i]);
  std::vector<int32_t> ivl;
  ETD_TRY(dbn_intervals(c, ivl));
  if (device_limits && (int)ivl.size() > DBN_MAX_INTERVALS) ETD_FAIL(ETD_EINVAL, "dbn: %d intervals per beat, at most %d (set num_tempi)", (int)ivl.size(), DBN_MAX_INTERVALS);
  out.clear();
  out.resize(1 + c->n_bars);
  for (int i = 0; i <= c->n_bars; ++i) {
    out[i].K = i == 0 ? 2 : 3;
    long long per_beat = 0;
    for (int v : ivl) per_beat += v;
    const long long S = per_beat * (i == 0 ? 1 : c->beats_per_bar[i - 1]);
    if (device_limits && S > DBN_MAX_STATES) ETD_FAIL(ETD_EINVAL, "dbn: HMM %d has %lld states, at most %d (raise min_bpm or set num_tempi)", i, S, DBN_MAX_STATES);
    if (S > (1 << 24)) ETD_FAIL(ETD_EINVAL, "dbn: HMM %d has %lld states", i, S);
    dbn_fill(out[i], ivl, i == 0 ? 1 : c->beats_per_bar[i - 1], c->transition_lambda, c->observation_lambda);
  }
  return ETD_OK;
}

static long long up16(long long x) { return (x + 15) / 16 * 16; }

DbnWs dbn_ws_layout(const DbnHmm& h, long long T) {
  DbnWs w;
  long long o = 0;
  w.out_cap = T / h.ivl[0] + 2;                                                   // one peak per beat period at most, + the partial ones at both ends
  w.dens = o; o += up16(T * h.K * 8);                                             // fp64 densities [T][K]
  w.seg = o; o += up16((T + 1) * 12);                                             // backtracked path as (first frame, last frame, first state) runs
  w.out = o; o += up16(w.out_cap * 8);                                            // (frame, beat number) results
  w.bp = o; o += up16(T * (long long)h.num_beats * h.n_int);                      // one byte per first state and frame
  w.rr = o; o += up16(T);                                                         // density index of the path's state per frame
  w.bn = o; o += up16(T);                                                         // beat number of the path's state per frame
  w.total = o;
  return w;
}

extern "C" int etd_dbn_describe(const etd_dbn_cfg* cfg, int hmm_index, int32_t* intervals_out, int cap, int* n_intervals, int* n_states, int* num_beats,
                                double* logtrans_out, uint8_t* pointers_out) {
  std::vector<DbnHmm> hm;
  ETD_TRY(dbn_build(cfg, hm, false));          // (any size: the 8 192-state / 255-interval limits are the device engine's, checked by etd_dbn_create)
  if (hmm_index < 0 || hmm_index >= (int)hm.size()) ETD_FAIL(ETD_EINVAL, "dbn_describe: hmm_index %d, the config has %d HMMs", hmm_index, (int)hm.size());
  const DbnHmm& h = hm[hmm_index];
  if (n_intervals) *n_intervals = h.n_int;
  if (n_states) *n_states = h.S;
  if (num_beats) *num_beats = h.num_beats;
  if (intervals_out) {
    if (cap < h.n_int) ETD_FAIL(ETD_ENOMEM, "dbn_describe: need room for %d intervals", h.n_int);
    std::copy(h.ivl.begin(), h.ivl.end(), intervals_out);
  }
  if (logtrans_out)
    for (int f = 0; f < h.n_int; ++f)
      for (int t = 0; t < h.n_int; ++t) logtrans_out[(size_t)f * h.n_int + t] = h.lt[(size_t)t * h.n_int + f];
  if (pointers_out) std::copy(h.ptr.begin(), h.ptr.end(), pointers_out);
  return ETD_OK;
}

extern "C" long long etd_dbn_workspace_bytes(const etd_dbn_cfg* cfg, long long T, int hmm_index) {
  std::vector<DbnHmm> hm;
  if (dbn_build(cfg, hm, true) != ETD_OK) return ETD_EINVAL;
  if (T < 0 || hmm_index < -1 || hmm_index >= (int)hm.size()) { g_etd_err = "dbn_workspace_bytes: bad T or hmm_index"; return ETD_EINVAL; }
  if (hmm_index >= 0) return dbn_ws_layout(hm[hmm_index], T).total;
  long long s = 0;
  for (const DbnHmm& h : hm) s += dbn_ws_layout(h, T).total;
  return s;
}
