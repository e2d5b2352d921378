// Native scheduler of the Decode stage: the bar loop of EtudeDecoder.generate (etude/models/etude_decoder.py:246-354)
// for MANY independent (song, attribute tuple) jobs, run as concurrent device streams (continuous batching).
// Host logic only -- prompt assembly (:257-296), history window (:346-348), token budget (:301,:352); every forward
// pass goes through the C ABI of this library (etd_decoder_begin_bars / _step / _poll / _read_many).
// Keeping this loop out of Python removes ~50 us of interpreter work per (job, bar) from the serving path.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/etude_hip_debug.h"
#include "common.h"

namespace {
constexpr int SRC_CLASS_ID = 1, TGT_CLASS_ID = 2;   // etude/data/dataset.py:18-19
constexpr int IGNORE_LABEL = -100;                  // F.cross_entropy's ignore index, the dataset's unscored rows (dataset.py:426)

struct Pair { const int32_t* x; int xn; std::vector<int32_t> y; int a[4]; };

struct Job {
  const etd_job* j;
  int bar = 0; long long total = 0; int slot = -1; int limit = 0;
  int n_out_known = 0;                    // tokens of the current bar the host knows of (last poll; 1 right after the bar's prefill)
  std::vector<Pair> hist;                 // <= n_ctx most recent (X, Y, attrs)
  std::vector<int32_t> out;               // [n_bars_done, len_0.., tokens...] built at the end
  std::vector<std::vector<int32_t>> bars; // generated bars ([Bar_BOS] + tokens)
};

// prompt of the job's current bar appended to ids/cls/attr rows; returns its length
int assemble(const Job& jb, const etd_sched_cfg& c, std::vector<int32_t>& ids, std::vector<int32_t>& cls, std::vector<int32_t> (&at)[4]) {
  const size_t start = ids.size();
  auto seg = [&](const int32_t* p, int n, int cl, const int* a4) {
    ids.insert(ids.end(), p, p + n);
    cls.insert(cls.end(), (size_t)n, cl);
    for (int k = 0; k < 4; ++k) at[k].insert(at[k].end(), (size_t)n, a4[k]);
  };
  const int32_t empty[2] = {c.bar_bos_id, c.bar_eos_id};
  const int neutral[4] = {1, 1, 1, 1};                                   // etude_decoder.py:250
  const int nh = (int)jb.hist.size();
  for (int i = 0; i < c.n_ctx_pairs - nh; ++i) { seg(empty, 2, SRC_CLASS_ID, neutral); seg(empty, 2, TGT_CLASS_ID, neutral); }
  for (const Pair& p : jb.hist) { seg(p.x, p.xn, SRC_CLASS_ID, p.a); seg(p.y.data(), (int)p.y.size(), TGT_CLASS_ID, p.a); }
  const etd_job& j = *jb.j;
  const int32_t* xb = j.x_ids + j.x_offsets[jb.bar];
  const int xn = j.x_offsets[jb.bar + 1] - j.x_offsets[jb.bar];
  const int* ya = j.attrs4 + 4 * jb.bar;
  seg(xb, xn, SRC_CLASS_ID, ya);
  size_t len = ids.size() - start;
  if ((long long)len > (long long)c.max_position_embeddings - c.max_bar_token_limit) {   // etude_decoder.py:285-289
    const size_t keep = (size_t)((double)c.max_position_embeddings * c.context_overlap_ratio);
    if (len > keep) {
      const size_t drop = len - keep;
      ids.erase(ids.begin() + start, ids.begin() + start + drop);
      cls.erase(cls.begin() + start, cls.begin() + start + drop);
      for (int k = 0; k < 4; ++k) at[k].erase(at[k].begin() + start, at[k].begin() + start + drop);
      len = keep;
    }
  }
  ids.push_back(c.bar_bos_id); cls.push_back(TGT_CLASS_ID);
  for (int k = 0; k < 4; ++k) at[k].push_back(ya[k]);
  return (int)len + 1;
}

// teacher-forced sequence of a cover bar y = [Bar_BOS] + tokens (etd_decoder_score_jobs): the bar's prompt as generate() builds it, then the tokens
// generate() fed back (y[1 : yn-1], target class, the bar's attributes); labels: what each row predicted -- -100 on the prompt rows but the last,
// then y[1:].  Appended to ids / cls / at / labels; returns the rows (0 for a [Bar_BOS]-only bar: nothing to score, nothing appended)
int assemble_scored(const Job& jb, const etd_sched_cfg& c, const int32_t* y, int yn, std::vector<int32_t>& ids, std::vector<int32_t>& cls,
                    std::vector<int32_t> (&at)[4], std::vector<int32_t>& labels) {
  if (yn <= 1) return 0;
  const size_t start = ids.size();
  const int P = assemble(jb, c, ids, cls, at);
  const int* ya = jb.j->attrs4 + 4 * jb.bar;
  ids.insert(ids.end(), y + 1, y + yn - 1);
  cls.insert(cls.end(), (size_t)(yn - 2), TGT_CLASS_ID);
  for (int k = 0; k < 4; ++k) at[k].insert(at[k].end(), (size_t)(yn - 2), ya[k]);
  labels.insert(labels.end(), (size_t)(P - 1), IGNORE_LABEL);
  labels.insert(labels.end(), y + 1, y + yn);
  return (int)(ids.size() - start);
}

int check_cover_bar(const etd_sched_cfg& c, const int32_t* y, int yn, const char* who, int job, int bar) {
  if (yn < 1 || !y || y[0] != c.bar_bos_id) ETD_FAIL(ETD_EINVAL, "%s: job %d bar %d does not start with Bar_BOS (id %d)", who, job, bar, c.bar_bos_id);
  if (yn - 1 > c.max_bar_token_limit) ETD_FAIL(ETD_EINVAL, "%s: job %d bar %d has %d tokens, more than max_bar_token_limit=%d", who, job, bar, yn - 1, c.max_bar_token_limit);
  return ETD_OK;
}
}  // namespace

// test hook (no GPU needed): the prompt the scheduler would build for one bar
extern "C" int etd_debug_assemble_prompt(const etd_sched_cfg* cfg, int n_hist, const int32_t* const* hx, const int32_t* hxn,
                                         const int32_t* const* hy, const int32_t* hyn, const int32_t* hattrs4, const int32_t* x, int xn,
                                         const int32_t* y_attrs4, int32_t* ids_out, int32_t* cls_out, int32_t* attrs4_out, int cap, int* T_out) {
  if (!cfg || n_hist < 0 || !x || !y_attrs4 || !ids_out || !cls_out || !attrs4_out || !T_out) ETD_FAIL(ETD_EINVAL, "assemble_prompt: bad arguments");
  if (cfg->struct_bytes != (int)sizeof(etd_sched_cfg)) ETD_FAIL(ETD_EINVAL, "assemble_prompt: etd_sched_cfg of %d bytes, expected %d", cfg->struct_bytes, (int)sizeof(etd_sched_cfg));
  const int32_t offs[2] = {0, xn};
  etd_job j{x, offs, 1, y_attrs4, nullptr};
  Job jb; jb.j = &j; jb.bar = 0;
  const int first = n_hist > cfg->n_ctx_pairs ? n_hist - cfg->n_ctx_pairs : 0;     // history_bar_pairs[-n:]
  for (int i = first; i < n_hist; ++i) {
    Pair p; p.x = hx[i]; p.xn = hxn[i]; p.y.assign(hy[i], hy[i] + hyn[i]); memcpy(p.a, hattrs4 + 4 * i, 16);
    jb.hist.push_back(std::move(p));
  }
  std::vector<int32_t> ids, cls, at[4];
  const int T = assemble(jb, *cfg, ids, cls, at);
  *T_out = T;
  if (T > cap) ETD_FAIL(ETD_ENOMEM, "assemble_prompt: need room for %d tokens", T);
  memcpy(ids_out, ids.data(), (size_t)T * 4); memcpy(cls_out, cls.data(), (size_t)T * 4);
  for (int k = 0; k < 4; ++k) memcpy(attrs4_out + (size_t)k * cap, at[k].data(), (size_t)T * 4);
  return ETD_OK;
}

extern "C" int etd_decoder_run_jobs(etd_dec* d, const etd_sched_cfg* cfg, const etd_job* jobs, int n_jobs, int32_t* out, long long out_cap,
                                    long long* job_offsets, long long* n_steps_out, void* stream) {
  if (!d || !cfg || !jobs || n_jobs < 1 || !out || !job_offsets) ETD_FAIL(ETD_EINVAL, "run_jobs: bad arguments");
  if (cfg->struct_bytes != (int)sizeof(etd_sched_cfg)) ETD_FAIL(ETD_EINVAL, "run_jobs: etd_sched_cfg of %d bytes, this library (ABI %d) expects %d -- caller built against another etude_hip.h", cfg->struct_bytes, ETD_ABI_VERSION, (int)sizeof(etd_sched_cfg));
  const etd_sched_cfg& c = *cfg;
  if (c.max_streams < 1 || c.n_ctx_pairs < 0 || c.max_bar_token_limit < 1 || c.max_prefill_rows < 1 || c.steps_per_poll < 1)
    ETD_FAIL(ETD_EINVAL, "run_jobs: bad scheduler config");
  if (!(c.temperature >= 0.f)) ETD_FAIL(ETD_EINVAL, "run_jobs: temperature must be >= 0");
  ETD_TRY(etd_decoder_set_sampling(d, c.temperature, c.top_p, c.seed, stream));
  std::vector<Job> J(n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    J[i].j = &jobs[i];
    if (jobs[i].n_bars < 0 || (jobs[i].n_bars > 0 && (!jobs[i].x_ids || !jobs[i].x_offsets || !jobs[i].attrs4))) ETD_FAIL(ETD_EINVAL, "run_jobs: job %d malformed", i);
  }
  // a job whose upstream stages are still running is not touched before its flag is set (acquire: the flag's writer filled the bars first)
  auto is_ready = [&](int i) { return !jobs[i].ready || __atomic_load_n(jobs[i].ready, __ATOMIC_ACQUIRE) != 0; };
  std::vector<int> free_slots;
  for (int s = c.max_streams - 1; s >= 0; --s) free_slots.push_back(s);
  std::vector<int> active;          // job indices holding a slot
  int next_job = 0;
  long long n_steps = 0;
  std::vector<int32_t> ids, cls, at[4], a4cat, slots, Ts, tg, eos, lim, dn, no, rd, cnt;

  // start the next bar of the given jobs (prefill in as few passes as the row budget allows); jobs that are finished are retired
  auto start_bars = [&](std::vector<int>& batch) -> int {
    std::vector<int> pend;
    for (int ji : batch) {
      Job& jb = J[ji];
      bool fin = jb.bar >= jb.j->n_bars;
      if (!fin) {
        const long long cap = (long long)c.max_output_tokens - jb.total;
        jb.limit = (int)std::min<long long>(c.force_bar_tokens > 0 ? c.force_bar_tokens : c.max_bar_token_limit, cap);
        if (jb.limit <= 0) { jb.bars.push_back({c.bar_bos_id}); fin = true; }   // the reference's inner loop breaks before its first forward
      }
      if (fin) {
        free_slots.push_back(jb.slot); jb.slot = -1;
        active.erase(std::remove(active.begin(), active.end(), ji), active.end());
      } else {
        pend.push_back(ji);
      }
    }
    size_t p = 0;
    while (p < pend.size()) {
      ids.clear(); cls.clear(); for (auto& v : at) v.clear();
      slots.clear(); Ts.clear(); tg.clear(); eos.clear(); lim.clear();
      while (p < pend.size()) {
        Job& jb = J[pend[p]];
        const size_t before = ids.size();
        const int T = assemble(jb, c, ids, cls, at);
        if (!slots.empty() && (long long)ids.size() > c.max_prefill_rows) {   // does not fit this pass: undo, flush
          ids.resize(before); cls.resize(before); for (auto& v : at) v.resize(before);
          break;
        }
        slots.push_back(jb.slot); Ts.push_back(T);
        const int* ya = jb.j->attrs4 + 4 * jb.bar;
        tg.insert(tg.end(), ya, ya + 4);
        eos.push_back(c.force_bar_tokens > 0 ? -1 : c.bar_eos_id);
        lim.push_back(jb.limit);
        ++p;
      }
      if (c.temperature > 0.f) {           // draw key of a stream = (job, bar): the same tokens whatever slot / pass the job lands in
        std::vector<unsigned long long> keys(slots.size());
        size_t q = p - slots.size();
        const int kstride = c.job_key_stride > 0 ? c.job_key_stride : 1;
        for (size_t i = 0; i < slots.size(); ++i, ++q) keys[i] = ((unsigned long long)(uint32_t)(c.job_key_offset + pend[q] * kstride) << 32) | (uint32_t)J[pend[q]].bar;
        ETD_TRY(etd_decoder_set_keys(d, (int)slots.size(), slots.data(), keys.data()));
      }
      const size_t M = ids.size();
      a4cat.resize(4 * M);
      for (int k = 0; k < 4; ++k) memcpy(a4cat.data() + (size_t)k * M, at[k].data(), M * 4);
      ETD_TRY(etd_decoder_begin_bars(d, (int)slots.size(), slots.data(), Ts.data(), ids.data(), cls.data(), a4cat.data(), tg.data(), eos.data(), lim.data(), stream));
    }
    return ETD_OK;
  };

  bool skip_poll = false;           // the bars of every active stream were (re)started or polled since the last step launch: nothing new to learn from a poll
  while (next_job < n_jobs || !active.empty()) {
    std::vector<int> fresh;
    while (next_job < n_jobs && !free_slots.empty() && is_ready(next_job)) {
      Job& jb = J[next_job];
      jb.slot = free_slots.back(); free_slots.pop_back();
      active.push_back(next_job);
      fresh.push_back(next_job++);
    }
    if (!fresh.empty()) { ETD_TRY(start_bars(fresh)); for (int ji : fresh) J[ji].n_out_known = 1; }
    if (active.empty()) {
      if (next_job < n_jobs && !is_ready(next_job)) std::this_thread::sleep_for(std::chrono::microseconds(100));   // idle until upstream delivers
      continue;
    }
    const int na = (int)active.size();
    std::sort(active.begin(), active.end(), [&](int a, int b) { return J[a].slot < J[b].slot; });
    slots.resize(na); dn.resize(na); no.resize(na);
    for (int i = 0; i < na; ++i) slots[i] = J[active[i]].slot;
    if (skip_poll) {
      // right after start_bars: a restarted stream has produced exactly its first token (the prefill's), the others are where
      // the last poll left them -- the step launches go out behind the prefill without a host round trip in between.  (A first
      // token that is already Bar_EOS just makes that row idle until the next poll.)
      for (int i = 0; i < na; ++i) { dn[i] = 0; no[i] = J[active[i]].n_out_known; }
      skip_poll = false;
    } else {
      ETD_TRY(etd_decoder_poll(d, slots.data(), na, dn.data(), no.data(), stream));
      for (int i = 0; i < na; ++i) J[active[i]].n_out_known = no[i];
    }
    std::vector<int> done_jobs;
    for (int i = 0; i < na; ++i) if (dn[i]) done_jobs.push_back(active[i]);
    if (!done_jobs.empty()) {
      const int nd = (int)done_jobs.size(), cap = 1024;
      std::vector<int32_t> ds(nd);
      for (int i = 0; i < nd; ++i) ds[i] = J[done_jobs[i]].slot;
      rd.resize((size_t)nd * cap); cnt.resize(nd);
      ETD_TRY(etd_decoder_read_many(d, nd, ds.data(), rd.data(), cap, cnt.data(), stream));
      std::vector<int> again;
      for (int i = 0; i < nd; ++i) {
        Job& jb = J[done_jobs[i]];
        const int32_t* t = rd.data() + (size_t)i * cap;
        std::vector<int32_t> y; y.reserve(cnt[i] + 1);
        y.push_back(c.bar_bos_id); y.insert(y.end(), t, t + cnt[i]);
        jb.total += cnt[i];
        const etd_job& j = *jb.j;
        Pair pr; pr.x = j.x_ids + j.x_offsets[jb.bar]; pr.xn = j.x_offsets[jb.bar + 1] - j.x_offsets[jb.bar]; pr.y = y;
        memcpy(pr.a, j.attrs4 + 4 * jb.bar, 16);
        jb.hist.push_back(std::move(pr));
        if ((int)jb.hist.size() > c.n_ctx_pairs) jb.hist.erase(jb.hist.begin());
        jb.bars.push_back(std::move(y));
        jb.bar += 1;
        if (jb.total >= c.max_output_tokens) jb.bar = jb.j->n_bars;          // etude_decoder.py:352: stop after this bar
        again.push_back(done_jobs[i]);
      }
      ETD_TRY(start_bars(again));
      for (int ji : again) J[ji].n_out_known = 1;
      skip_poll = true;
      continue;                                   // refill, then step without another poll
    }
    int nstep = c.steps_per_poll;
    if (c.force_bar_tokens > 0) {                 // no early EOS possible: run to the nearest bar end in one call
      nstep = 1 << 30;
      for (int i = 0; i < na; ++i) nstep = std::min(nstep, J[active[i]].limit - no[i]);
      nstep = std::max(nstep, 1);
    }
    ETD_TRY(etd_decoder_step(d, slots.data(), na, nstep, stream));
    n_steps += nstep;
  }
  // pack results: per job [n_bars_done, len_0 .. len_{n-1}, tokens of bar 0, tokens of bar 1, ...]
  long long pos = 0;
  for (int i = 0; i < n_jobs; ++i) {
    job_offsets[i] = pos;
    const auto& bars = J[i].bars;
    long long need = 1 + (long long)bars.size();
    for (auto& b : bars) need += (long long)b.size();
    if (pos + need > out_cap) ETD_FAIL(ETD_ENOMEM, "run_jobs: output buffer too small (need > %lld ints)", out_cap);
    out[pos++] = (int32_t)bars.size();
    for (auto& b : bars) out[pos++] = (int32_t)b.size();
    for (auto& b : bars) { memcpy(out + pos, b.data(), b.size() * 4); pos += (long long)b.size(); }
  }
  job_offsets[n_jobs] = pos;
  if (n_steps_out) *n_steps_out = n_steps;
  return ETD_OK;
}

// test hook (no GPU needed): the teacher-forced sequence etd_decoder_score_jobs builds for one cover bar
extern "C" int etd_debug_assemble_scored(const etd_sched_cfg* cfg, int n_hist, const int32_t* const* hx, const int32_t* hxn, const int32_t* const* hy,
                                         const int32_t* hyn, const int32_t* hattrs4, const int32_t* x, int xn, const int32_t* y, int yn,
                                         const int32_t* y_attrs4, int32_t* ids_out, int32_t* cls_out, int32_t* attrs4_out, int32_t* labels_out,
                                         int cap, int* T_out) {
  if (!cfg || n_hist < 0 || !x || !y_attrs4 || !ids_out || !cls_out || !attrs4_out || !labels_out || !T_out) ETD_FAIL(ETD_EINVAL, "assemble_scored: bad arguments");
  if (cfg->struct_bytes != (int)sizeof(etd_sched_cfg)) ETD_FAIL(ETD_EINVAL, "assemble_scored: etd_sched_cfg of %d bytes, expected %d", cfg->struct_bytes, (int)sizeof(etd_sched_cfg));
  ETD_TRY(check_cover_bar(*cfg, y, yn, "assemble_scored", 0, n_hist));
  const int32_t offs[2] = {0, xn};
  etd_job j{x, offs, 1, y_attrs4, nullptr};
  Job jb; jb.j = &j; jb.bar = 0;
  const int first = n_hist > cfg->n_ctx_pairs ? n_hist - cfg->n_ctx_pairs : 0;
  for (int i = first; i < n_hist; ++i) {
    Pair p; p.x = hx[i]; p.xn = hxn[i]; p.y.assign(hy[i], hy[i] + hyn[i]); memcpy(p.a, hattrs4 + 4 * i, 16);
    jb.hist.push_back(std::move(p));
  }
  std::vector<int32_t> ids, cls, at[4], lab;
  const int T = assemble_scored(jb, *cfg, y, yn, ids, cls, at, lab);
  *T_out = T;
  if (T > cap) ETD_FAIL(ETD_ENOMEM, "assemble_scored: need room for %d rows", T);
  if (T > 0) {
    memcpy(ids_out, ids.data(), (size_t)T * 4); memcpy(cls_out, cls.data(), (size_t)T * 4); memcpy(labels_out, lab.data(), (size_t)T * 4);
    for (int k = 0; k < 4; ++k) memcpy(attrs4_out + (size_t)k * cap, at[k].data(), (size_t)T * 4);
  }
  return ETD_OK;
}

// Teacher-forced per-bar scores of many covers (etude_hip.h): every bar of every job becomes one sequence of ONE etd_decoder_score call
extern "C" int etd_decoder_score_jobs(etd_dec* d, const etd_sched_cfg* cfg, const etd_score_job* jobs, int n_jobs, double* bar_logprob, int32_t* bar_tokens,
                                      int32_t* bar_hits, void* stream) {
  if (!d || !cfg || !jobs || n_jobs < 1 || !bar_logprob || !bar_tokens || !bar_hits) ETD_FAIL(ETD_EINVAL, "score_jobs: bad arguments");
  if (cfg->struct_bytes != (int)sizeof(etd_sched_cfg)) ETD_FAIL(ETD_EINVAL, "score_jobs: etd_sched_cfg of %d bytes, this library (ABI %d) expects %d -- caller built against another etude_hip.h", cfg->struct_bytes, ETD_ABI_VERSION, (int)sizeof(etd_sched_cfg));
  const etd_sched_cfg& c = *cfg;
  if (c.n_ctx_pairs < 0 || c.max_bar_token_limit < 1) ETD_FAIL(ETD_EINVAL, "score_jobs: bad scheduler config");
  std::vector<int32_t> ids, cls, at[4], lab, T;
  std::vector<long long> seq_bar;                  // output index of each sequence (bars with nothing to score have none)
  long long nout = 0;
  for (int ji = 0; ji < n_jobs; ++ji) {
    const etd_score_job& s = jobs[ji];
    if (s.n_bars < 0 || s.n_y_bars < 0 || s.n_y_bars > s.n_bars || (s.n_bars > 0 && (!s.x_ids || !s.x_offsets || !s.attrs4)) || (s.n_y_bars > 0 && (!s.y_ids || !s.y_offsets)))
      ETD_FAIL(ETD_EINVAL, "score_jobs: job %d malformed (%d condition bars, %d cover bars)", ji, s.n_bars, s.n_y_bars);
    const etd_job j{s.x_ids, s.x_offsets, s.n_bars, s.attrs4, nullptr};
    Job jb; jb.j = &j;
    for (int b = 0; b < s.n_y_bars; ++b, ++nout) {
      const int32_t* y = s.y_ids + s.y_offsets[b];
      const int yn = s.y_offsets[b + 1] - s.y_offsets[b];
      ETD_TRY(check_cover_bar(c, y, yn, "score_jobs", ji, b));
      bar_logprob[nout] = 0.0; bar_tokens[nout] = 0; bar_hits[nout] = 0;
      jb.bar = b;
      const int t = assemble_scored(jb, c, y, yn, ids, cls, at, lab);
      if (t > 0) { T.push_back(t); seq_bar.push_back(nout); }
      Pair p; p.x = s.x_ids + s.x_offsets[b]; p.xn = s.x_offsets[b + 1] - s.x_offsets[b]; p.y.assign(y, y + yn);
      memcpy(p.a, s.attrs4 + 4 * b, 16);
      jb.hist.push_back(std::move(p));
      if ((int)jb.hist.size() > c.n_ctx_pairs) jb.hist.erase(jb.hist.begin());
    }
  }
  const int n = (int)T.size();
  if (n == 0) return ETD_OK;
  const size_t M = ids.size();
  std::vector<int32_t> a4((size_t)4 * M);
  for (int k = 0; k < 4; ++k) memcpy(a4.data() + (size_t)k * M, at[k].data(), M * 4);
  std::vector<double> lp(n); std::vector<int32_t> tok(n), hit(n);
  ETD_TRY(etd_decoder_score(d, n, T.data(), ids.data(), cls.data(), a4.data(), lab.data(), lp.data(), tok.data(), hit.data(), nullptr, nullptr, nullptr, stream));
  for (int i = 0; i < n; ++i) { bar_logprob[seq_bar[i]] = lp[i]; bar_tokens[seq_bar[i]] = tok[i]; bar_hits[seq_bar[i]] = hit[i]; }
  return ETD_OK;
}
