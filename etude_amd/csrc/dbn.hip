// DBN beat / downbeat tracking on the device: fp64 log-space Viterbi over the beat HMM and one bar HMM per bar length, for a ragged batch of songs.
//
// One workgroup per (song, HMM).  The kernel is a latency chain of T dependent steps, so what it minimises is work and barriers per step:
//   * A state of interval i only ever moves to the next position of its own interval, with probability 1.  The Viterbi vector (LDS, fp64) is therefore never shifted:
//     a physical slot keeps its value and its POSITION advances by one per frame (a per-slot counter in a register); the step adds the frame's density in place,
//     `(v + 0.0) + density`.  Each thread owns its slots for the whole song, so this needs no synchronisation.
//   * The slot whose position wraps to 0 becomes the interval's first state: one thread per (beat, interval) takes the maximum over the last states of the previous
//     beat, `(last + logtrans) + density`, predecessors in increasing order with a strict `>` (lowest index wins ties), and records the winning interval index as a
//     one-byte backpointer [T][beats * intervals].  Last-state values travel through a small double-buffered LDS array, which is what makes ONE barrier per frame enough.
//   * Densities are computed beforehand (k_dbn_prep, parallel over frames, fp64 from the fp32 activations) and staged through LDS 16 frames at a time, prefetched
//     one chunk ahead.
//   * Backtracking jumps from first state to first state (one dependent load per beat), then the per-frame pointers, the runs of "beat" frames, their peaks
//     (`correct`) and the beat numbers are found in parallel and compacted in order.  No atomics: a (song, HMM) is computed by one workgroup from that song alone.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/etude_hip.h"
#include "../../include/etude_hip_debug.h"
#include "common.h"
#include "dbn.h"
#include "host_util.h"
#include "prof.h"

namespace {
constexpr int DBN_CH = 16;          // frames per staged density chunk
constexpr int DBN_SLOTS = 8;        // Viterbi slots per thread at most (8 x 1024 threads = DBN_MAX_STATES)
constexpr int DBN_FIRSTS = 2;       // first states per thread at most (8 beats x 255 intervals <= 2 x 1024)
constexpr int DBN_LT_LDS_MAX = 55;  // intervals up to which the log-transition table lives in LDS (55^2 doubles = 24 KiB)

struct HmmDev {
  int S, NF, n_int, num_beats, K, per_beat;
  double init;
  const int32_t* ivl; const int32_t* first; const double* lt; const int32_t* flo; const int32_t* fhi;
  const uint8_t* ptr; const uint8_t* beatno; const uint16_t* chain;
};

struct DbnRes {          // per (song, HMM), copied to the host
  double logprob;
  int32_t count;         // result pairs found (may exceed the list's capacity: then only `cap` were written)
  int32_t first;         // frames trimmed at the front
  int32_t T_eff;         // frames tracked (0: nothing above the threshold, or all-zero activations)
  int32_t pad;
};

struct DbnJob {
  long long in_row;      // the song's first row in the input [sum T][2]
  int T;                 // its frames
  int hmm;
  int from_res;          // 1: frames / trim offset come from res (written by k_dbn_prep); 0: T frames of supplied densities (debug)
  int out_cap;
  double* dens;          // [T][K]
  uint8_t* bp;           // [T][NF]
  int32_t* seg;          // [T + 1][3]
  uint8_t* rr; uint8_t* bn;   // [T] each
  int32_t* out;          // [out_cap][2]
  int32_t* path;         // [T] states (debug) or null
  DbnRes* res;
};

__device__ __forceinline__ float dbn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// the two activations of a frame as the trackers see them: beat HMM (a, -), bar HMM (max(beat - downbeat, 0), downbeat)
__device__ __forceinline__ void dbn_act(const float* in, long long row, int is_logits, int K, float* a0, float* a1) {
  float b = in[2 * row], d = in[2 * row + 1];
  if (is_logits == ETD_DBN_IN_LOGITS) { b = dbn_sigmoid(b); d = dbn_sigmoid(d); }
  if (K == 2) { *a0 = b; *a1 = 0.f; }
  else if (is_logits == ETD_DBN_IN_COMBINED) { *a0 = b; *a1 = d; }
  else { *a0 = fmaxf(b - d, 0.f); *a1 = d; }
}

// ---- threshold trimming + densities.  One workgroup per (song, HMM).
__global__ __launch_bounds__(256) void k_dbn_prep(const DbnJob* jobs, const HmmDev* hmms, const float* in, int is_logits, float thr, double olambda) {
  __shared__ int s_lo[256], s_hi[256], s_nz[256];
  const DbnJob jb = jobs[blockIdx.x];
  const int K = hmms[jb.hmm].K, T = jb.T, tid = threadIdx.x;
  int lo = T, hi = -1;
  if (thr != 0.f) {
    for (int t = tid; t < T; t += 256) {
      float a0, a1;
      dbn_act(in, jb.in_row + t, is_logits, K, &a0, &a1);
      if (a0 >= thr || (K == 3 && a1 >= thr)) { lo = min(lo, t); hi = max(hi, t); }
    }
  }
  s_lo[tid] = lo; s_hi[tid] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { s_lo[tid] = min(s_lo[tid], s_lo[tid + o]); s_hi[tid] = max(s_hi[tid], s_hi[tid + o]); }
    __syncthreads();
  }
  int first = 0, last = T;
  if (thr != 0.f) {
    if (s_hi[0] > 0) { first = s_lo[0]; last = min(T, s_hi[0] + 1); }      // `idx.any()`: false when the only index is 0
    else { first = 0; last = 0; }
  }
  int nz = 0;
  for (int t = first + tid; t < last; t += 256) {
    float a0, a1;
    dbn_act(in, jb.in_row + t, is_logits, K, &a0, &a1);
    if (a0 != 0.f || a1 != 0.f) nz = 1;
    const double den = olambda - 1.0;
    double* d = jb.dens + (long long)(t - first) * K;
    if (K == 2) {
      d[0] = log((1.0 - (double)a0) / den);
      d[1] = log((double)a0);
    } else {
      const float s = a0 + a1;
      d[0] = log((1.0 - (double)s) / den);
      d[1] = log((double)a0);
      d[2] = log((double)a1);
    }
  }
  s_nz[tid] = nz;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_nz[tid] |= s_nz[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    jb.res->first = first;
    jb.res->T_eff = (last > first && s_nz[0]) ? last - first : 0;
    jb.res->count = 0;
    jb.res->logprob = -INFINITY;
    jb.res->pad = 0;
  }
}

// block-wide ordered compaction step (as in mpe2note_dev.hip): this thread's slot or -1; *base advances by the number of flags
__device__ __forceinline__ int dbn_ordered_slot(bool flag, int* wsum, int* base, int nwaves) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int off = *base, tot = 0;
  for (int w = 0; w < nwaves; ++w) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
  __syncthreads();
  if (threadIdx.x == 0) *base += tot;
  __syncthreads();
  return flag ? off + before : -1;
}

__device__ __forceinline__ double dbn_pick(int p, double d0, double d1, double d2) { return p == 0 ? d0 : (p == 1 ? d1 : d2); }

template <bool LT_LDS>
__global__ __launch_bounds__(1024) void k_dbn_viterbi(const DbnJob* jobs, const HmmDev* hmms, const float* in, int is_logits) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_wsum[16];
  __shared__ int s_base, s_nseg, s_best;
  const DbnJob jb = jobs[blockIdx.x];
  const HmmDev hm = hmms[jb.hmm];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int S = hm.S, NF = hm.NF, n_int = hm.n_int, K = hm.K, B = hm.num_beats;
  const int T = jb.from_res ? jb.res->T_eff : jb.T;
  const int first_frame = jb.from_res ? jb.res->first : 0;
  if (T <= 0) return;                                              // (uniform: nothing to track, k_dbn_prep left count = 0)
  // ---- LDS carve-up (the host sizes it with dbn_lds_bytes)
  double* v = smem;                                                // [S]       the Viterbi vector, by physical slot
  double* last = v + S;                                            // [2][NF]   last-state values of frame t in buffer t & 1
  double* dch = last + 2 * NF;                                     // [2][CH * 3] staged densities
  double* redv = dch + 2 * DBN_CH * 3;                             // [NT]
  double* ltl = redv + NT;                                         // [n_int][n_int] (LT_LDS)
  int* reds = (int*)(ltl + (LT_LDS ? n_int * n_int : 0));          // [NT]
  uint8_t* ptrl = (uint8_t*)(reds + NT);                           // [S]
  for (int s = tid; s < S; s += NT) { v[s] = hm.init; ptrl[s] = hm.ptr[s]; }
  for (int c = tid; c < NF; c += NT) last[NF + c] = hm.init;       // "frame -1" lives in buffer 1
  if (LT_LDS)
    for (int i = tid; i < n_int * n_int; i += NT) ltl[i] = hm.lt[i];
  for (int i = tid; i < DBN_CH * K && i < T * K; i += NT) dch[i] = jb.dens[i];
  // ---- my slots: position counter, interval length, first state of the interval, chain
  int kpos[DBN_SLOTS], klen[DBN_SLOTS], kbase[DBN_SLOTS], kch[DBN_SLOTS];
  int nslot = 0;
#pragma unroll
  for (int j = 0; j < DBN_SLOTS; ++j) {
    const int s = tid + j * NT;
    kpos[j] = klen[j] = kbase[j] = kch[j] = 0;
    if (s < S) {
      const int c = hm.chain[s], iv = c % n_int, b = c / n_int;
      kch[j] = c; klen[j] = hm.ivl[iv]; kbase[j] = b * hm.per_beat + hm.first[iv]; kpos[j] = s - kbase[j];
      nslot = j + 1;
    }
  }
  // ---- my first states
  int fc[DBN_FIRSTS], flen[DBN_FIRSTS], fbase[DBN_FIRSTS], fhead[DBN_FIRSTS], fprev[DBN_FIRSTS], flo[DBN_FIRSTS], fhi[DBN_FIRSTS], fptr[DBN_FIRSTS];
  int nfirst = 0;
#pragma unroll
  for (int q = 0; q < DBN_FIRSTS; ++q) {
    const int c = tid + q * NT;
    fc[q] = flen[q] = fbase[q] = fhead[q] = fprev[q] = flo[q] = fptr[q] = 0; fhi[q] = -1;
    if (c < NF) {
      const int iv = c % n_int, b = c / n_int;
      fc[q] = c; flen[q] = hm.ivl[iv]; fbase[q] = b * hm.per_beat + hm.first[iv]; fhead[q] = flen[q] - 1;
      fprev[q] = ((b + B - 1) % B) * n_int; flo[q] = hm.flo[iv]; fhi[q] = hm.fhi[iv]; fptr[q] = hm.ptr[fbase[q]];
      nfirst = q + 1;
    }
  }
  // ---- T dependent steps, one barrier each
  double pre = 0.0;
  for (int t = 0; t < T; ++t) {
    __syncthreads();
    const double* d = dch + ((t / DBN_CH) & 1) * (DBN_CH * 3) + (t % DBN_CH) * K;
    const double d0 = d[0], d1 = d[1], d2 = K == 3 ? d[2] : 0.0;
    if (t % DBN_CH == 0 && tid < DBN_CH * K) {                     // the next chunk, in flight during this one
      const long long i = (long long)(t + DBN_CH) * K + tid;
      pre = i < (long long)T * K ? jb.dens[i] : 0.0;
    }
    double* lcur = last + (t & 1) * NF;
#pragma unroll
    for (int j = 0; j < DBN_SLOTS; ++j) {
      if (j < nslot) {
        int k = kpos[j] + 1;
        if (k == klen[j]) k = 0;
        kpos[j] = k;
        if (k != 0) {                                              // (position 0 is written by the interval's first-state thread below)
          const int s = tid + j * NT;
          const double nv = (v[s] + 0.0) + dbn_pick(ptrl[kbase[j] + k], d0, d1, d2);
          v[s] = nv;
          if (k == klen[j] - 1) lcur[kch[j]] = nv;
        }
      }
    }
    const double* lprev = last + ((t + 1) & 1) * NF;
#pragma unroll
    for (int q = 0; q < DBN_FIRSTS; ++q) {
      if (q < nfirst) {
        const double* lp = lprev + fprev[q];
        const double* row = (LT_LDS ? ltl : hm.lt) + (fc[q] % n_int) * n_int;
        double best = -INFINITY;
        int arg = flo[q];
        for (int f = flo[q]; f <= fhi[q]; ++f) {
          const double c = lp[f] + row[f];
          if (c > best) { best = c; arg = f; }
        }
        const double nv = best + dbn_pick(fptr[q], d0, d1, d2);
        v[fbase[q] + fhead[q]] = nv;
        jb.bp[(long long)t * NF + fc[q]] = (uint8_t)arg;
        if (flen[q] == 1) lcur[fc[q]] = nv;
        fhead[q] = fhead[q] == 0 ? flen[q] - 1 : fhead[q] - 1;
      }
    }
    if (t % DBN_CH == DBN_CH - 1 && tid < DBN_CH * K) dch[(((t / DBN_CH) + 1) & 1) * (DBN_CH * 3) + tid] = pre;
  }
  __syncthreads();
  // ---- final maximum, lowest state index on ties
  {
    double bv = 0.0;
    int bs = -1;
#pragma unroll
    for (int j = 0; j < DBN_SLOTS; ++j) {
      if (j < nslot) {
        const double x = v[tid + j * NT];
        const int st = kbase[j] + kpos[j];
        if (bs < 0 || x > bv || (x == bv && st < bs)) { bv = x; bs = st; }
      }
    }
    redv[tid] = bv; reds[tid] = bs;
  }
  __syncthreads();
  if (tid == 0) {
    double bv = redv[0];
    int bs = reds[0];
    for (int i = 1; i < NT; ++i) {
      const int st = reds[i];
      if (st < 0) continue;
      const double x = redv[i];
      if (x > bv || (x == bv && st < bs)) { bv = x; bs = st; }
    }
    jb.res->logprob = bv;
    s_best = bs;
    s_nseg = 0;
    // ---- backtrack from first state to first state: (first frame, last frame, state at the first frame) runs, latest first
    if (bv > -INFINITY || jb.path) {
      int c = hm.chain[bs];
      int iv = c % n_int, b = c / n_int;
      int base = b * hm.per_beat + hm.first[iv];
      int k = bs - base, t = T - 1, n = 0;
      while (t >= 0) {
        const int t0 = t - k, ts = t0 > 0 ? t0 : 0;
        jb.seg[3 * n] = ts; jb.seg[3 * n + 1] = t; jb.seg[3 * n + 2] = base + k - (t - ts);
        ++n;
        if (t0 <= 0) break;
        const int f = jb.bp[(long long)t0 * NF + c];
        b = (b + B - 1) % B;
        c = b * n_int + f;
        base = b * hm.per_beat + hm.first[f];
        k = hm.ivl[f] - 1;
        t = t0 - 1;
      }
      s_nseg = n;
    }
  }
  __syncthreads();
  const int nseg = s_nseg;
  if (nseg == 0) return;                                           // log-probability -inf: no beats (count stays 0)
  for (int i = tid; i < nseg; i += NT) {
    const int ts = jb.seg[3 * i], te = jb.seg[3 * i + 1], st = jb.seg[3 * i + 2];
    for (int t = ts; t <= te; ++t) {
      const int s = st + (t - ts);
      jb.rr[t] = ptrl[s];
      jb.bn[t] = hm.beatno[s];
      if (jb.path) jb.path[t] = s;
    }
  }
  if (tid == 0) s_base = 0;
  __syncthreads();
  if (!jb.from_res) return;
  // ---- every run of frames whose state points at a beat density gives one beat at its strongest frame (first maximum)
  for (int t0 = 0; t0 < T; t0 += NT) {
    const int t = t0 + tid;
    bool emit = false;
    int peak = 0;
    if (t < T && jb.rr[t] != 0 && (t == 0 || jb.rr[t - 1] == 0)) {
      emit = true;
      float bestv = 0.f;
      for (int e = t; e < T && jb.rr[e] != 0; ++e) {
        float a0, a1;
        dbn_act(in, jb.in_row + first_frame + e, is_logits, K, &a0, &a1);
        if (e == t || a0 > bestv) { bestv = a0; peak = e; }
        if (K == 3 && a1 > bestv) { bestv = a1; peak = e; }
      }
    }
    const int slot = dbn_ordered_slot(emit, s_wsum, &s_base, (NT + 63) / 64);
    if (slot >= 0 && slot < jb.out_cap) { jb.out[2 * slot] = peak + first_frame; jb.out[2 * slot + 1] = jb.bn[peak]; }
  }
  if (tid == 0) jb.res->count = s_base;
}

size_t dbn_lds_bytes(const DbnHmm& h, int NT, bool lt_lds) {
  size_t n = (size_t)h.S * 8 + (size_t)2 * h.num_beats * h.n_int * 8 + (size_t)2 * DBN_CH * 3 * 8 + (size_t)NT * 8;
  if (lt_lds) n += (size_t)h.n_int * h.n_int * 8;
  n += (size_t)NT * 4 + (size_t)h.S;
  return (n + 15) / 16 * 16;
}
}  // namespace

struct etd_dbn {
  etd_dbn_cfg cfg;
  std::vector<DbnHmm> hm;
  DevPool pool;
  HmmDev* hmms_dev = nullptr;
  int NT = 64;
  bool lt_lds = true;
  size_t lds = 0;
  unsigned char* ws = nullptr; size_t ws_bytes = 0;
  std::vector<DbnJob> jobs;
  std::vector<unsigned char> host;
};

extern "C" void etd_dbn_destroy(etd_dbn* h) {
  if (!h) return;
  (void)hipDeviceSynchronize();
  (void)hipFree(h->ws);
  h->pool.free_all();
  delete h;
}

extern "C" int etd_dbn_create(const etd_dbn_cfg* cfg, etd_dbn** out) {
  if (!out) ETD_FAIL(ETD_EINVAL, "dbn_create: null out");
  std::vector<DbnHmm> hm;
  ETD_TRY(dbn_build(cfg, hm, true));
  etd_dbn* h = new etd_dbn();
  auto fail = [&](int rc) { h->pool.free_all(); delete h; return rc; };
  h->cfg = *cfg;
  h->hm = hm;
  h->lt_lds = hm[0].n_int <= DBN_LT_LDS_MAX;
  std::vector<HmmDev> hd(hm.size());
  for (size_t i = 0; i < hm.size(); ++i) {
    const DbnHmm& m = hm[i];
    HmmDev& d = hd[i];
    d.S = m.S; d.NF = m.num_beats * m.n_int; d.n_int = m.n_int; d.num_beats = m.num_beats; d.K = m.K; d.per_beat = m.per_beat; d.init = m.init;
    int32_t *ivl, *first, *flo, *fhi; double* lt; uint8_t *ptr, *bno; uint16_t* ch;
    ETD_TRY_OR(fail, h->pool.upload(&ivl, m.ivl.data(), m.ivl.size()));
    ETD_TRY_OR(fail, h->pool.upload(&first, m.first.data(), m.first.size()));
    ETD_TRY_OR(fail, h->pool.upload(&flo, m.flo.data(), m.flo.size()));
    ETD_TRY_OR(fail, h->pool.upload(&fhi, m.fhi.data(), m.fhi.size()));
    ETD_TRY_OR(fail, h->pool.upload(&lt, m.lt.data(), m.lt.size()));
    ETD_TRY_OR(fail, h->pool.upload(&ptr, m.ptr.data(), m.ptr.size()));
    ETD_TRY_OR(fail, h->pool.upload(&bno, m.beatno.data(), m.beatno.size()));
    ETD_TRY_OR(fail, h->pool.upload(&ch, m.chain.data(), m.chain.size()));
    d.ivl = ivl; d.first = first; d.flo = flo; d.fhi = fhi; d.lt = lt; d.ptr = ptr; d.beatno = bno; d.chain = ch;
    const int need = std::max((m.S + DBN_SLOTS - 1) / DBN_SLOTS, (d.NF + DBN_FIRSTS - 1) / DBN_FIRSTS);
    h->NT = std::max(h->NT, std::min(1024, (need + 63) / 64 * 64));
  }
  for (const DbnHmm& m : hm) h->lds = std::max(h->lds, dbn_lds_bytes(m, h->NT, h->lt_lds));
  if (h->lds > 160 * 1024) return fail((g_etd_err = "dbn_create: the HMM needs more LDS than a CU has", ETD_EINVAL));
  ETD_TRY_OR(fail, h->pool.upload(&h->hmms_dev, hd.data(), hd.size()));
  if (h->lds > 48 * 1024) {
    if (h->lt_lds) ETD_TRY_OR(fail, ETD_HIP_RC(hipFuncSetAttribute((const void*)k_dbn_viterbi<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds)));
    else ETD_TRY_OR(fail, ETD_HIP_RC(hipFuncSetAttribute((const void*)k_dbn_viterbi<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds)));
  }
  *out = h;
  return ETD_OK;
}

static int dbn_reserve(etd_dbn* h, size_t bytes) {
  if (bytes <= h->ws_bytes) return ETD_OK;
  (void)hipDeviceSynchronize();
  (void)hipFree(h->ws);
  h->ws = nullptr; h->ws_bytes = 0;
  const size_t cap = (bytes + (1u << 20)) / (1u << 20) * (1u << 20);
  HIP_TRY(hipMalloc(&h->ws, cap));
  h->ws_bytes = cap;
  return ETD_OK;
}

static void dbn_launch(etd_dbn* h, const DbnJob* jobs_dev, int n_jobs, const float* in, int is_logits, hipStream_t st) {
  if (h->lt_lds) hipLaunchKernelGGL(k_dbn_viterbi<true>, dim3(n_jobs), dim3(h->NT), h->lds, st, jobs_dev, h->hmms_dev, in, is_logits);
  else hipLaunchKernelGGL(k_dbn_viterbi<false>, dim3(n_jobs), dim3(h->NT), h->lds, st, jobs_dev, h->hmms_dev, in, is_logits);
}

extern "C" int etd_dbn_track(etd_dbn* h, const float* in_dev, int input_kind, int n_seq, const int64_t* T_host,
                             int32_t* beat_frames, long long beat_cap, int64_t* beat_offsets,
                             int32_t* down_frames, int32_t* down_numbers, long long down_cap, int64_t* down_offsets,
                             int32_t* bar_choice, long long* needed, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int is_logits = input_kind;
  if (!h || n_seq < 0 || (n_seq > 0 && (!in_dev || !T_host)) || !beat_offsets || !down_offsets || !needed || beat_cap < 0 || down_cap < 0)
    ETD_FAIL(ETD_EINVAL, "dbn_track: bad args");
  if (is_logits < ETD_DBN_IN_ACTIVATIONS || is_logits > ETD_DBN_IN_COMBINED) ETD_FAIL(ETD_EINVAL, "dbn_track: input kind %d", is_logits);
  needed[0] = needed[1] = 0;
  beat_offsets[0] = down_offsets[0] = 0;
  if (n_seq == 0) return ETD_OK;
  const int n_hmm = (int)h->hm.size(), n_jobs = n_seq * n_hmm;
  // ---- workspace: [jobs][result headers][result lists][per-job blocks]
  size_t off = (size_t)n_jobs * sizeof(DbnJob);
  off = (off + 255) / 256 * 256;
  const size_t o_res = off;
  off += (size_t)n_jobs * sizeof(DbnRes);
  std::vector<size_t> o_out(n_jobs), o_blk(n_jobs);
  for (int s = 0; s < n_seq; ++s) {
    if (T_host[s] < 1 || T_host[s] > 0x3fffffffLL) ETD_FAIL(ETD_EINVAL, "dbn_track: song %d has %lld frames", s, (long long)T_host[s]);
    for (int i = 0; i < n_hmm; ++i) { o_out[s * n_hmm + i] = off; off += (size_t)dbn_ws_layout(h->hm[i], T_host[s]).out_cap * 8; }
  }
  const size_t o_end_out = off;
  off = (off + 255) / 256 * 256;
  for (int s = 0; s < n_seq; ++s)
    for (int i = 0; i < n_hmm; ++i) { o_blk[s * n_hmm + i] = off; off += (size_t)dbn_ws_layout(h->hm[i], T_host[s]).total; }
  ETD_TRY(dbn_reserve(h, off));
  h->jobs.assign(n_jobs, DbnJob());
  long long row = 0;
  for (int s = 0; s < n_seq; ++s) {
    for (int i = 0; i < n_hmm; ++i) {
      const int j = s * n_hmm + i;
      const DbnWs w = dbn_ws_layout(h->hm[i], T_host[s]);
      unsigned char* b = h->ws + o_blk[j];
      DbnJob& jb = h->jobs[j];
      jb.in_row = row; jb.T = (int)T_host[s]; jb.hmm = i; jb.from_res = 1; jb.out_cap = (int)w.out_cap;
      jb.dens = (double*)(b + w.dens); jb.bp = b + w.bp; jb.seg = (int32_t*)(b + w.seg); jb.rr = b + w.rr; jb.bn = b + w.bn;
      jb.out = (int32_t*)(h->ws + o_out[j]); jb.path = nullptr; jb.res = (DbnRes*)(h->ws + o_res) + j;
    }
    row += T_host[s];
  }
  HIP_TRY(hipMemcpyAsync(h->ws, h->jobs.data(), (size_t)n_jobs * sizeof(DbnJob), hipMemcpyHostToDevice, st));
  {
    ProfScope ps("k_dbn_prep", st);
    hipLaunchKernelGGL(k_dbn_prep, dim3(n_jobs), dim3(256), 0, st, (const DbnJob*)h->ws, h->hmms_dev, in_dev, is_logits, (float)h->cfg.threshold, h->cfg.observation_lambda);
    HIP_TRY(hipGetLastError());
  }
  {
    ProfScope ps("k_dbn_viterbi", st);
    dbn_launch(h, (const DbnJob*)h->ws, n_jobs, in_dev, is_logits, st);
    HIP_TRY(hipGetLastError());
  }
  h->host.resize(o_end_out - o_res);
  HIP_TRY(hipMemcpyAsync(h->host.data(), h->ws + o_res, o_end_out - o_res, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const DbnRes* res = (const DbnRes*)h->host.data();
  // ---- per song: the beat HMM's list, and the list of the bar length with the highest log-probability (first wins ties)
  std::vector<int> pick(n_seq, -1);
  long long nb = 0, nd = 0;
  for (int s = 0; s < n_seq; ++s) {
    const DbnRes* r = res + (size_t)s * n_hmm;
    if (r[0].count > h->jobs[s * n_hmm].out_cap) ETD_FAIL(ETD_EHIP, "dbn_track: song %d: %d beats exceed the list of %d", s, r[0].count, h->jobs[s * n_hmm].out_cap);
    nb += r[0].count;
    beat_offsets[s + 1] = nb;
    int best = -1;
    for (int i = 1; i < n_hmm; ++i)
      if (r[i].T_eff > 0 && (best < 0 || r[i].logprob > r[best].logprob)) best = i;
    if (best >= 0 && !(r[best].logprob > -std::numeric_limits<double>::infinity())) best = -1;
    if (best >= 0 && r[best].count > h->jobs[s * n_hmm + best].out_cap) ETD_FAIL(ETD_EHIP, "dbn_track: song %d: %d downbeat rows exceed the list", s, r[best].count);
    pick[s] = best;
    if (best >= 0) nd += r[best].count;
    down_offsets[s + 1] = nd;
    if (bar_choice) bar_choice[s] = best >= 0 ? best - 1 : -1;
  }
  needed[0] = nb; needed[1] = nd;
  if (nb > beat_cap || nd > down_cap || (nb > 0 && !beat_frames) || (nd > 0 && (!down_frames || !down_numbers)))
    ETD_FAIL(ETD_ENOMEM, "dbn_track: need room for %lld beats and %lld downbeat rows", nb, nd);
  for (int s = 0; s < n_seq; ++s) {
    const int32_t* ob = (const int32_t*)(h->host.data() + (o_out[s * n_hmm] - o_res));
    for (long long k = 0, n = beat_offsets[s + 1] - beat_offsets[s]; k < n; ++k) beat_frames[beat_offsets[s] + k] = ob[2 * k];
    if (pick[s] < 0) continue;
    const int32_t* od = (const int32_t*)(h->host.data() + (o_out[s * n_hmm + pick[s]] - o_res));
    for (long long k = 0, n = down_offsets[s + 1] - down_offsets[s]; k < n; ++k) { down_frames[down_offsets[s] + k] = od[2 * k]; down_numbers[down_offsets[s] + k] = od[2 * k + 1]; }
  }
  return ETD_OK;
}

extern "C" int etd_dbn_debug_viterbi(etd_dbn* h, int hmm_index, const double* densities_dev, long long T, int32_t* path_out, double* logprob_out) {
  if (!h || hmm_index < 0 || hmm_index >= (int)h->hm.size() || !densities_dev || T < 1 || T > 0x3fffffffLL || !path_out || !logprob_out)
    ETD_FAIL(ETD_EINVAL, "dbn_debug_viterbi: bad args");
  const DbnWs w = dbn_ws_layout(h->hm[hmm_index], T);
  const size_t o_res = 256, o_path = 512, o_blk = (512 + (size_t)T * 4 + 255) / 256 * 256;
  ETD_TRY(dbn_reserve(h, o_blk + (size_t)w.total));
  unsigned char* b = h->ws + o_blk;
  DbnJob jb = DbnJob();
  jb.in_row = 0; jb.T = (int)T; jb.hmm = hmm_index; jb.from_res = 0; jb.out_cap = 0;
  jb.dens = const_cast<double*>(densities_dev); jb.bp = b + w.bp; jb.seg = (int32_t*)(b + w.seg); jb.rr = b + w.rr; jb.bn = b + w.bn;
  jb.out = nullptr; jb.path = (int32_t*)(h->ws + o_path); jb.res = (DbnRes*)(h->ws + o_res);
  HIP_TRY(hipMemcpy(h->ws, &jb, sizeof(jb), hipMemcpyHostToDevice));
  dbn_launch(h, (const DbnJob*)h->ws, 1, nullptr, 0, nullptr);
  HIP_TRY(hipGetLastError());
  DbnRes r;
  HIP_TRY(hipMemcpy(&r, h->ws + o_res, sizeof(r), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(path_out, h->ws + o_path, (size_t)T * 4, hipMemcpyDeviceToHost));
  *logprob_out = r.logprob;
  return ETD_OK;
}
