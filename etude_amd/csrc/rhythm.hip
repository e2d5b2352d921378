// Rhythm metrics on the GPU: a ragged batch of covers, each a sorted, unique fp64 onset list in seconds -> Rhythmic Grid Consistency (score and inferred tau) and IOI
// Pattern Entropy, the reference's RGCCalculator / IPECalculator (etude/evaluation/metrics/rgc.py, ipe.py) with scikit-learn's KMeans behind the second.  DESIGN.md 4h
// is the contract; tests/rhythm_np.py restates it in fp64 numpy.
//
// ONE launch per batch, one workgroup of 256 threads per cover, everything fp64, the cover's working set in LDS: X [slots] fp64 (the log-IOIs), K [slots] 64-bit (sort
// keys, then the k-means++ distances, then the n-gram keys) and L [slots] labels; `slots` is the power of two above the longest cover of the call, so short covers
// share a CU.  No atomics and no flags: every floating-point sum whose order the contract fixes is added by ONE lane in that order (numpy's pairwise sum, the cumulative
// sum of k-means++, the potentials -- one lane per candidate --, the centre sums -- one lane per cluster --), the rest is integer work (bitonic sorts of 64-bit keys,
// counts, maxima) whose result does not depend on the order, and the entropy's terms are added by position modulo 256 and a fixed tree.  So a cover's numbers depend
// on its onsets alone: bit-identical alone, in any batch, from run to run.
//
// rh_cover also compiles for the host (T = 1: the same arithmetic in the same order except for the entropy's tree), which is how the routine is stepped through in a
// debugger; nothing in the library calls it there.
#include "rhythm.h"
#include "prof.h"
#include "np_sum.h"

#include <cmath>

#pragma clang fp contract(off)      // every product and sum below rounds on its own, on the device and on the host

#if defined(__HIP_DEVICE_COMPILE__)
#define RH_SYNC() __syncthreads()
#else
#define RH_SYNC() ((void)0)
#endif
#define RH_HD __host__ __device__ __forceinline__

struct RhShared {
  unsigned long long red[RH_THREADS];
  double dred[RH_THREADS];
  double top[RH_MAX_TOPK];
  double c[RH_MAX_CLUSTERS], sum[RH_MAX_CLUSTERS], w[RH_MAX_CLUSTERS];
  double cand_pot[4];
  int cand[4];
  double pot, mean, tol;
  int n_top, bad, changed, stop, first, relocated;
};

namespace {

typedef unsigned long long u64;

// ascending bitonic sort of P (a power of two) keys in LDS; the caller has synchronised; synchronised on return
RH_HD void rh_sort(u64* key, int P, int tid, int T) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += T) {
        const int l = i ^ j;
        if (l > i) {
          const u64 a = key[i], b = key[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up && a != b) { key[i] = b; key[l] = a; }
        }
      }
      RH_SYNC();
    }
}

// max / sum of every thread's v over the workgroup (integers: any order gives the same result); synchronised on return, red is free again
RH_HD u64 rh_max(RhShared* s, u64 v, int tid, int T) {
  s->red[tid] = v;
  RH_SYNC();
  for (int h = T >> 1; h > 0; h >>= 1) {
    if (tid < h) { const u64 o = s->red[tid + h]; if (o > s->red[tid]) s->red[tid] = o; }
    RH_SYNC();
  }
  const u64 r = s->red[0];
  RH_SYNC();
  return r;
}
RH_HD u64 rh_add(RhShared* s, u64 v, int tid, int T) {
  s->red[tid] = v;
  RH_SYNC();
  for (int h = T >> 1; h > 0; h >>= 1) {
    if (tid < h) s->red[tid] += s->red[tid + h];
    RH_SYNC();
  }
  const u64 r = s->red[0];
  RH_SYNC();
  return r;
}

RH_HD int rh_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// an order-preserving 64-bit key of a finite double
RH_HD u64 rh_key(double x) {
  const u64 b = (u64)__builtin_bit_cast(long long, x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// scikit-learn's euclidean_distances(squared=True) on one feature, in its order
RH_HD double rh_sqdist(double c, double x) {
  const double d = ((-2.0 * (c * x)) + c * c) + x * x;
  return d > 0.0 ? d : 0.0;
}

// labels = the first minimum of (-2 (x c)) + c c; sets s->changed where a label differs from the one in L.  The caller synchronises around it.
RH_HD void rh_assign(const double* X, unsigned char* L, int m, int k, RhShared* s, int tid, int T) {
  double c[RH_MAX_CLUSTERS], cc[RH_MAX_CLUSTERS];
#pragma unroll
  for (int j = 0; j < RH_MAX_CLUSTERS; ++j) { c[j] = j < k ? s->c[j] : 0.0; cc[j] = c[j] * c[j]; }
  for (int i = tid; i < m; i += T) {
    const double x = X[i];
    int best = 0;
    double bd = (-2.0 * (x * c[0])) + cc[0];
#pragma unroll
    for (int j = 1; j < RH_MAX_CLUSTERS; ++j) {
      const double d = (-2.0 * (x * c[j])) + cc[j];
      if (j < k && d < bd) { bd = d; best = j; }
    }
    if (L[i] != (unsigned char)best) { L[i] = (unsigned char)best; s->changed = 1; }
  }
}

// One cover.  X, K, L: the cover's LDS arrays of `slots` entries (m = n - 1 <= slots); tid / T: this thread and the workgroup's size.
RH_HD void rh_cover(const RhArgs& a, int b, double* X, u64* K, unsigned char* L, RhShared* s, int tid, int T) {
  const long long o0 = a.offsets[b];
  const int n = (int)(a.offsets[b + 1] - o0), m = n - 1;
  const double* t = a.onsets + o0;
  const double nan = __builtin_nan("");
  int rgc = 0, ipe = 0, k = 0, iters = 0;
  double score = nan, tau = nan, H = nan;
  if (tid == 0) { s->bad = 0; s->relocated = 0; }
  RH_SYNC();
  if (n < 2) {
    rgc = 1; ipe = 1;
  } else {
    const int P = rh_pow2(m);
    const u64 idx_mask = (1ULL << RH_IDX_BITS) - 1;
    // ------------------------------------------------------------ RGC: count the rounded IOIs
    for (int i = tid; i < P; i += T) {
      u64 key = ~0ULL;
      if (i < m) {
        const double ioi = t[i + 1] - t[i], q = rint(ioi * a.scale);
        if (!(ioi > 0.0) || !(q < 1125899906842624.0)) { s->bad = 1; key = (u64)i; }      // not sorted and unique, not finite, or past 2^50 once scaled
        else key = ((u64)q << RH_IDX_BITS) | (u64)i;
      }
      K[i] = key;
    }
    RH_SYNC();
    const int bad = s->bad;
    if (bad) {
      rgc = RH_BAD_INPUT; ipe = RH_BAD_INPUT;
    } else {
      if (m < a.top_k) {
        rgc = 2;
      } else {
        rh_sort(K, P, tid, T);
        // a run's head gets (count, first occurrence reversed): the largest is the most common, ties to the earliest in the sequence
        unsigned int* S = (unsigned int*)X;
        for (int i = tid; i < P; i += T) {
          unsigned int v = 0;
          if (i < m) {
            const u64 q = K[i] >> RH_IDX_BITS;
            if (i == 0 || (K[i - 1] >> RH_IDX_BITS) != q) {
              int e = i + 1;
              while (e < m && (K[e] >> RH_IDX_BITS) == q) ++e;
              v = ((unsigned int)(e - i) << RH_IDX_BITS) | (unsigned int)(idx_mask - (K[i] & idx_mask));
            }
          }
          S[i] = v;
        }
        RH_SYNC();
        int n_top = 0;
        for (int r = 0; r < a.top_k; ++r) {
          u64 best = 0;
          for (int i = tid; i < m; i += T) {
            const u64 v = ((u64)S[i] << RH_IDX_BITS) | (u64)i;
            if (v > best) best = v;
          }
          best = rh_max(s, best, tid, T);
          if ((best >> RH_IDX_BITS) == 0) break;            // (uniform: every thread holds the same maximum)
          if (tid == 0) {
            const int pos = (int)(best & idx_mask);
            s->top[r] = (double)(K[pos] >> RH_IDX_BITS) / a.scale;
            S[pos] = 0;
          }
          ++n_top;
          RH_SYNC();
        }
        if (n_top < 2) {
          rgc = 3;
        } else {
          // one lane per candidate tau: the mean of |r - rint(r)| in numpy's order
          for (int c = tid; c < n_top; c += T) {
            const double tc = s->top[c];
            double v = -1.0;                                 // (skipped: below 0.01)
            if (!(tc < 0.01)) {
              const double* top = s->top;
              v = np_sum_leaf(n_top, [&](int j) { const double r = top[j] / tc; return fabs(r - rint(r)); }) / (double)n_top;
            }
            s->dred[c] = v;
          }
          RH_SYNC();
          if (tid == 0) {
            int bi = -1;
            for (int c = 0; c < n_top; ++c)
              if (s->dred[c] >= 0.0 && (bi < 0 || s->dred[c] < s->dred[bi])) bi = c;      // strict <: the first best
            s->first = bi;
          }
          RH_SYNC();
          const int bi = s->first;
          if (bi < 0) rgc = 4;
          else { score = s->dred[bi]; tau = s->top[bi]; }
          RH_SYNC();
        }
      }
      // ------------------------------------------------------------ IPE: clipped log-IOIs, their number of distinct values
      for (int i = tid; i < P; i += T) {
        u64 key = ~0ULL;
        if (i < m) {
          double ioi = t[i + 1] - t[i];
          ioi = ioi < a.min_ioi ? a.min_ioi : ioi;
          ioi = ioi > a.max_ioi ? a.max_ioi : ioi;
          const double x = log(ioi);
          X[i] = x;
          key = rh_key(x);
        }
        K[i] = key;
      }
      RH_SYNC();
      rh_sort(K, P, tid, T);
      u64 heads = 0;
      for (int i = tid; i < m; i += T) heads += (i == 0 || K[i - 1] != K[i]) ? 1 : 0;
      const int n_unique = (int)rh_add(s, heads, tid, T);
      k = n_unique < a.n_clusters ? n_unique : a.n_clusters;
      if (k < 2) {
        ipe = 3;
      } else {
        double* D = (double*)K;                              // the k-means++ distances take the keys' place
        if (tid == 0) s->mean = np_sum_all(m, [&](int i) { return X[i]; }) / (double)m;
        RH_SYNC();
        const double mean = s->mean;
        for (int i = tid; i < m; i += T) {
          const double x = X[i] - mean;
          X[i] = x;
          if (a.tap_x) a.tap_x[o0 + i] = x;
        }
        RH_SYNC();
        if (tid == 0) {
          s->tol = (np_sum_all(m, [&](int i) { return X[i] * X[i]; }) / (double)m) * 1e-4;
          // the first centre: RandomState.choice with uniform p: cdf = cumsum(1 / m) / cdf[-1], searchsorted(side = right)
          const double p = 1.0 / (double)m;
          double last = 0.0;
          for (int i = 0; i < m; ++i) last += p;
          double cs = 0.0;
          int first = m - 1;
          for (int i = 0; i < m; ++i) {
            cs += p;
            if (cs / last > a.rnd[0]) { first = i; break; }
          }
          s->c[0] = X[first];
        }
        RH_SYNC();
        {
          const double c0 = s->c[0];
          for (int i = tid; i < m; i += T) D[i] = rh_sqdist(c0, X[i]);
        }
        RH_SYNC();
        if (tid == 0) {
          double pot = 0.0;
          for (int i = 0; i < m; ++i) pot += D[i];
          s->pot = pot;
        }
        RH_SYNC();
        const int trials = 2 + (k >= 8 ? 2 : (k >= 3 ? 1 : 0));            // 2 + int(log k), k <= 8
        int rpos = 1;
        for (int c = 1; c < k; ++c) {
          if (tid == 0) {
            // the candidates: the first i whose sequential cumulative sum reaches rnd * pot, clipped to m - 1
            double v[4];
            int found = 0;
            for (int q = 0; q < 4; ++q) { v[q] = q < trials ? a.rnd[rpos + q] * s->pot : 0.0; s->cand[q] = m - 1; }
            double cs = 0.0;
            for (int i = 0; i < m && found != (1 << trials) - 1; ++i) {
              cs += D[i];
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (q < trials && !((found >> q) & 1) && cs >= v[q]) { found |= 1 << q; s->cand[q] = i; }
            }
          }
          rpos += trials;
          RH_SYNC();
          for (int q = tid; q < trials; q += T) {             // one lane per candidate: its potential, added in sample order
            const double xc = X[s->cand[q]];
            double pot = 0.0;
            for (int i = 0; i < m; ++i) {
              const double d = rh_sqdist(xc, X[i]), e = D[i];
              pot += d < e ? d : e;
            }
            s->cand_pot[q] = pot;
          }
          RH_SYNC();
          if (tid == 0) {
            int bq = 0;
            for (int q = 1; q < trials; ++q)
              if (s->cand_pot[q] < s->cand_pot[bq]) bq = q;   // the first minimum
            s->pot = s->cand_pot[bq];
            s->c[c] = X[s->cand[bq]];
          }
          RH_SYNC();
          {
            const double xc = s->c[c];
            for (int i = tid; i < m; i += T) {
              const double d = rh_sqdist(xc, X[i]), e = D[i];
              D[i] = d < e ? d : e;
            }
          }
          RH_SYNC();
        }
        // ---------------------------------------------------------- Lloyd
        for (int i = tid; i < m; i += T) L[i] = 255;
        bool strict = false;
        for (iters = 1; iters <= RH_MAX_ITER; ++iters) {
          if (tid == 0) s->changed = 0;
          RH_SYNC();
          rh_assign(X, L, m, k, s, tid, T);
          RH_SYNC();
          for (int j = tid; j < k; j += T) {                 // one lane per cluster: its sum and count in sample order
            double sum = 0.0, w = 0.0;
            for (int i = 0; i < m; ++i)
              if (L[i] == j) { sum += X[i]; w += 1.0; }
            s->sum[j] = sum; s->w[j] = w;
          }
          RH_SYNC();
          if (tid == 0) {
            int empty[RH_MAX_CLUSTERS], n_empty = 0;
            for (int j = 0; j < k; ++j)
              if (s->w[j] == 0.0) empty[n_empty++] = j;
            if (n_empty) {
              // _relocate_empty_clusters_dense: the samples farthest from their own centre move, distance descending, then the lowest index (the project's rule)
              s->relocated = 1;
              int far[RH_MAX_CLUSTERS];
              bool any = true;
              for (int e = 0; e < n_empty && any; ++e) {
                int bi = -1;
                double bd = -1.0;
                for (int i = 0; i < m; ++i) {
                  bool taken = false;
                  for (int f = 0; f < e; ++f) taken |= far[f] == i;
                  const double df = X[i] - s->c[L[i]], d = df * df;
                  if (!taken && d > bd) { bd = d; bi = i; }
                }
                if (e == 0 && bd == 0.0) any = false;         // more clusters than distinct samples: nothing moves
                far[e] = bi;
              }
              if (any)
                for (int e = 0; e < n_empty; ++e) {
                  const int j = empty[e], i = far[e], o = L[i];
                  s->sum[o] -= X[i] * 1.0;
                  s->sum[j] = X[i] * 1.0;
                  s->w[j] = 1.0;
                  s->w[o] -= 1.0;
                }
            }
            int heavy = 0;
            for (int j = 1; j < k; ++j)
              if (s->w[j] > s->w[heavy]) heavy = j;
            for (int j = 0; j < k; ++j) {                     // in place and in ascending j, as _average_centers
              if (s->w[j] > 0.0) s->sum[j] *= 1.0 / s->w[j];
              else s->sum[j] = s->sum[heavy];
            }
            double sh[RH_MAX_CLUSTERS];
            for (int j = 0; j < RH_MAX_CLUSTERS; ++j) {
              double v = 0.0;
              if (j < k) { const double d = s->sum[j] - s->c[j], r = sqrt(d * d); v = r * r; s->c[j] = s->sum[j]; }
              sh[j] = v;
            }
            const double tot = k < 8 ? ((((((sh[0] + sh[1]) + sh[2]) + sh[3]) + sh[4]) + sh[5]) + sh[6])
                                     : ((sh[0] + sh[1]) + (sh[2] + sh[3])) + ((sh[4] + sh[5]) + (sh[6] + sh[7]));
            s->stop = !s->changed ? 1 : (tot <= s->tol ? 2 : 0);
          }
          RH_SYNC();
          const int stop = s->stop;
          if (stop == 1) strict = true;
          if (stop) break;
        }
        if (iters > RH_MAX_ITER) iters = RH_MAX_ITER;
        if (!strict) {
          RH_SYNC();
          rh_assign(X, L, m, k, s, tid, T);
        }
        RH_SYNC();
        if (a.tap_lab)
          for (int i = tid; i < m; i += T) a.tap_lab[o0 + i] = (signed char)L[i];
        if (a.tap_c)
          for (int j = tid; j < RH_MAX_CLUSTERS; j += T) a.tap_c[(long long)b * RH_MAX_CLUSTERS + j] = j < k ? s->c[j] : nan;
        // ---------------------------------------------------------- the n-grams' entropy
        const int mg = m - a.n_gram + 1;
        if (mg < 1) {
          H = 0.0;
        } else {
          const int P2 = rh_pow2(mg);
          for (int i = tid; i < P2; i += T) {
            u64 key = ~0ULL;
            if (i < mg) {
              key = 0;
              for (int g = 0; g < a.n_gram; ++g) key = (key << 3) | (u64)L[i + g];
            }
            K[i] = key;
          }
          RH_SYNC();
          rh_sort(K, P2, tid, T);
          double acc = 0.0;
          for (int i = tid; i < mg; i += T) {
            if (i == 0 || K[i - 1] != K[i]) {
              int e = i + 1;
              while (e < mg && K[e] == K[i]) ++e;
              const double p = (double)(e - i) / (double)mg;
              acc += p * log2(p);
            }
          }
          s->dred[tid] = acc;
          RH_SYNC();
          for (int h = T >> 1; h > 0; h >>= 1) {
            if (tid < h) s->dred[tid] += s->dred[tid + h];
            RH_SYNC();
          }
          H = -s->dred[0];
        }
      }
    }
  }
  if (tid == 0) {
    a.out[3LL * b + 0] = score; a.out[3LL * b + 1] = tau; a.out[3LL * b + 2] = ipe == 0 ? H : nan;
    a.status[b] = rgc | (ipe << 4) | (s->relocated << 8) | (k << 12) | (iters << 16);
  }
}

__global__ __launch_bounds__(RH_THREADS) void k_rhythm(const RhArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rh_lds[];
  __shared__ RhShared sh;
  double* X = (double*)rh_lds;
  u64* K = (u64*)(rh_lds + (size_t)8 * a.slots);
  unsigned char* L = rh_lds + (size_t)16 * a.slots;
  rh_cover(a, (int)blockIdx.x, X, K, L, &sh, (int)threadIdx.x, RH_THREADS);
}

}  // namespace

struct etd_rhythm {
  etd_rhythm_cfg cfg;
  double rnd[RH_N_RANDOM];
  double scale;
  bool attr_set = false;
  double* tap_x = nullptr; signed char* tap_lab = nullptr; double* tap_c = nullptr;
};

extern "C" int etd_rhythm_limits(int* max_onsets, int* max_covers, int* max_top_k, int* max_n_gram) {
  if (max_onsets) *max_onsets = RH_MAX_ONSETS;
  if (max_covers) *max_covers = RH_MAX_COVERS;
  if (max_top_k) *max_top_k = RH_MAX_TOPK;
  if (max_n_gram) *max_n_gram = RH_MAX_NGRAM;
  return ETD_OK;
}

extern "C" int etd_rhythm_create(const etd_rhythm_cfg* cfg, etd_rhythm** out) {
  if (!cfg || !out) ETD_FAIL(ETD_EINVAL, "rhythm_create: null argument");
  ETD_CHECK_CFG(cfg, etd_rhythm_cfg, "rhythm_create");
  if (cfg->top_k < 1 || cfg->top_k > RH_MAX_TOPK) ETD_FAIL(ETD_EINVAL, "rhythm_create: top_k = %d (need 1 .. %d)", cfg->top_k, RH_MAX_TOPK);
  if (cfg->precision_digits < 0 || cfg->precision_digits > RH_MAX_DIGITS) ETD_FAIL(ETD_EINVAL, "rhythm_create: precision_digits = %d (need 0 .. %d)", cfg->precision_digits, RH_MAX_DIGITS);
  if (cfg->n_gram < 1 || cfg->n_gram > RH_MAX_NGRAM) ETD_FAIL(ETD_EINVAL, "rhythm_create: n_gram = %d (need 1 .. %d)", cfg->n_gram, RH_MAX_NGRAM);
  if (cfg->n_clusters < 1 || cfg->n_clusters > RH_MAX_CLUSTERS) ETD_FAIL(ETD_EINVAL, "rhythm_create: n_clusters = %d (need 1 .. %d: a symbol takes 3 bits)", cfg->n_clusters, RH_MAX_CLUSTERS);
  if (!(cfg->min_ioi > 0.0) || !(cfg->max_ioi >= cfg->min_ioi) || !std::isfinite(cfg->max_ioi))
    ETD_FAIL(ETD_EINVAL, "rhythm_create: need 0 < min_ioi <= max_ioi < inf (got %g, %g)", cfg->min_ioi, cfg->max_ioi);
  if (cfg->n_random != RH_N_RANDOM || !cfg->random_host) ETD_FAIL(ETD_EINVAL, "rhythm_create: random_host must hold %d doubles (got %d)", RH_N_RANDOM, cfg->n_random);
  for (int i = 0; i < RH_N_RANDOM; ++i)
    if (!(cfg->random_host[i] >= 0.0 && cfg->random_host[i] < 1.0)) ETD_FAIL(ETD_EINVAL, "rhythm_create: random_host[%d] = %g is outside [0, 1)", i, cfg->random_host[i]);
  etd_rhythm* h = new etd_rhythm();
  h->cfg = *cfg;
  h->cfg.random_host = nullptr;
  for (int i = 0; i < RH_N_RANDOM; ++i) h->rnd[i] = cfg->random_host[i];
  h->scale = 1.0;
  for (int i = 0; i < cfg->precision_digits; ++i) h->scale *= 10.0;      // (exact: 10^9 < 2^53)
  *out = h;
  return ETD_OK;
}

extern "C" void etd_rhythm_destroy(etd_rhythm* h) {
  if (!h) return;
  if (h->attr_set) (void)hipDeviceSynchronize();      // kernels of this handle may still be in flight
  delete h;
}

extern "C" int etd_rhythm_debug_logioi(etd_rhythm* h, double* logioi_dev, signed char* labels_dev, double* centres_dev) {
  if (!h) ETD_FAIL(ETD_EINVAL, "rhythm_debug_logioi: null handle");
  if ((logioi_dev || labels_dev || centres_dev) && !(logioi_dev && labels_dev && centres_dev))
    ETD_FAIL(ETD_EINVAL, "rhythm_debug_logioi: give all three buffers, or none to turn the tap off");
  h->tap_x = logioi_dev; h->tap_lab = labels_dev; h->tap_c = centres_dev;
  return ETD_OK;
}

extern "C" int etd_rhythm_check(const etd_rhythm* h, const int64_t* offsets_host, int n_covers) {
  if (!h || !offsets_host) ETD_FAIL(ETD_EINVAL, "rhythm: null argument");
  if (n_covers < 1 || n_covers > RH_MAX_COVERS) ETD_FAIL(ETD_EINVAL, "rhythm: %d covers in one call (need 1 .. %d)", n_covers, RH_MAX_COVERS);
  if (offsets_host[0] != 0) ETD_FAIL(ETD_EINVAL, "rhythm: offsets_host[0] = %lld (need 0)", (long long)offsets_host[0]);
  for (int b = 0; b < n_covers; ++b) {
    const long long n = offsets_host[b + 1] - offsets_host[b];
    if (n < 0) ETD_FAIL(ETD_EINVAL, "rhythm: offsets_host decreases at cover %d", b);
    if (n > RH_MAX_ONSETS) ETD_FAIL(ETD_EINVAL, "rhythm: cover %d has %lld onsets (> %d, what a cover's working set in LDS holds)", b, n, RH_MAX_ONSETS);
  }
  return ETD_OK;
}

extern "C" int etd_rhythm_run(etd_rhythm* h, const double* onsets_dev, const int64_t* offsets_dev, const int64_t* offsets_host, int n_covers, double* out_dev,
                              int32_t* status_dev, void* stream) {
  if (!h || !offsets_dev || !offsets_host) ETD_FAIL(ETD_EINVAL, "rhythm_run: null argument");
  if (!out_dev || !status_dev) ETD_FAIL(ETD_EINVAL, "rhythm_run: null output (out_dev and status_dev are both written)");
  ETD_TRY(etd_rhythm_check(h, offsets_host, n_covers));
  long long longest = 0;
  for (int b = 0; b < n_covers; ++b) {
    const long long n = offsets_host[b + 1] - offsets_host[b];
    if (n > longest) longest = n;
  }
  if (offsets_host[n_covers] > 0 && !onsets_dev) ETD_FAIL(ETD_EINVAL, "rhythm_run: null onsets_dev");
  hipStream_t st = (hipStream_t)stream;
  if (!h->attr_set) {
    // more dynamic LDS than the 64 KB a launch gets without saying so
    HIP_TRY(hipFuncSetAttribute((const void*)k_rhythm, hipFuncAttributeMaxDynamicSharedMemorySize, RH_LDS_PER_SLOT * RH_MAX_ONSETS));
    h->attr_set = true;
  }
  RhArgs a;
  memset(&a, 0, sizeof(a));
  a.onsets = onsets_dev; a.offsets = offsets_dev; a.n_covers = n_covers; a.out = out_dev; a.status = status_dev;
  a.top_k = h->cfg.top_k; a.n_gram = h->cfg.n_gram; a.n_clusters = h->cfg.n_clusters;
  a.slots = 8;
  while (a.slots < longest - 1) a.slots <<= 1;
  a.scale = h->scale; a.min_ioi = h->cfg.min_ioi; a.max_ioi = h->cfg.max_ioi;
  for (int i = 0; i < RH_N_RANDOM; ++i) a.rnd[i] = h->rnd[i];
  a.tap_x = h->tap_x; a.tap_lab = h->tap_lab; a.tap_c = h->tap_c;
  {
    ProfScope ps("k_rhythm", st, 0, (double)offsets_host[n_covers] * 8.0);
    hipLaunchKernelGGL(k_rhythm, dim3((unsigned)n_covers), dim3(RH_THREADS), (size_t)RH_LDS_PER_SLOT * a.slots, st, a);
  }
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
