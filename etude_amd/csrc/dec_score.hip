// Teacher-forced scoring kernels of the EtudeDecoder (dec_score.h).  Both are small next to the forward pass that feeds them:
// a row is V logits (154 shipped, 3000 the config default) read once; a sequence is a few hundred floats.
// No atomics: every sum runs in a fixed order, so the results are bitwise reproducible and independent of the launch layout.
#include "dec_score.h"
#include "prof.h"

// ================================================================================================
// log-softmax of one row at its label + argmax        F.cross_entropy / torch.argmax (etude_decoder.py:196-198, :333)
// ================================================================================================
__global__ __launch_bounds__(64) void k_row_logprob(const float* __restrict__ logits, int ldl, int V, int n, const int* __restrict__ out_row,
                                                    const int* __restrict__ labels, float* __restrict__ lp, float* __restrict__ lse, int* __restrict__ amax) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= n) return;                                  // (grid == n; the whole wave leaves together)
  const float* lg = logits + (long long)j * ldl;
  // max + argmax, lowest index on ties: the comparisons of wave_argmax (dec_kernels.hip), so the greedy hit of a row is what k_dargmax would pick
  float best = -INFINITY; int bi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float x = lg[v];
    if (x > best || (x == best && v < bi)) { best = x; bi = v; }
  }
#define ETD_AMAX_STAGE(O) { const float ob = lane_xor<O>(best); const int oi = lane_xor<O>(bi); \
    const bool take = (ob > best) | ((ob == best) & (oi < bi)); best = take ? ob : best; bi = take ? oi : bi; }
  ETD_AMAX_STAGE(32) ETD_AMAX_STAGE(16) ETD_AMAX_STAGE(8) ETD_AMAX_STAGE(4) ETD_AMAX_STAGE(2) ETD_AMAX_STAGE(1)
#undef ETD_AMAX_STAGE
  // sum exp(l - max): each lane over its own stride, then a butterfly -- both partners of a stage add the same two values, so every
  // lane ends with the same bits
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(lg[v] - best);
  s += lane_xor<32>(s); s += lane_xor<16>(s); s += lane_xor<8>(s); s += lane_xor<4>(s); s += lane_xor<2>(s); s += lane_xor<1>(s);
  if (lane == 0) {
    const int r = out_row[j];
    const int lab = labels[r];
    const float z = best + logf(s);
    lp[r] = (lab >= 0 && lab < V) ? lg[lab] - z : 0.f;
    lse[r] = z;
    amax[r] = bi;
  }
}

int launch_row_logprob(const float* logits, int ldl, int V, int n, const int* out_row, const int* labels, float* lp, float* lse, int* amax, hipStream_t st) {
  if (n <= 0) return ETD_OK;
  if (V < 1 || ldl < V) ETD_FAIL(ETD_EINVAL, "row_logprob: bad shape V=%d ldl=%d", V, ldl);
  ProfScope ps("k_row_logprob", st, 3.0 * n * V, 4.0 * n * V);
  hipLaunchKernelGGL(k_row_logprob, dim3(n), dim3(64), 0, st, logits, ldl, V, n, out_row, labels, lp, lse, amax);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ================================================================================================
// per-sequence sums: log-likelihood (double), scored tokens, greedy hits
// ================================================================================================
__global__ __launch_bounds__(64) void k_seq_reduce(const int* __restrict__ row0, const int* __restrict__ len, int n_seq, const int* __restrict__ labels,
                                                   const float* __restrict__ lp, const int* __restrict__ amax, double* __restrict__ seq_lp,
                                                   int* __restrict__ seq_tokens, int* __restrict__ seq_hits) {
  __shared__ double ps[64];
  __shared__ int pt[64], ph[64];
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= n_seq) return;
  const int r0 = row0[s], n = len[s];
  double acc = 0.0; int tok = 0, hit = 0;
  for (int t = lane; t < n; t += 64) {
    const int r = r0 + t, lab = labels[r];
    if (lab != ETD_IGNORE_LABEL) { acc += (double)lp[r]; ++tok; hit += amax[r] == lab; }
  }
  ps[lane] = acc; pt[lane] = tok; ph[lane] = hit;
  __syncthreads();
  if (lane == 0) {
    double a = 0.0; int tk = 0, hh = 0;
    for (int i = 0; i < 64; ++i) { a += ps[i]; tk += pt[i]; hh += ph[i]; }     // lane order: the same sum for the same rows, whatever the launch
    seq_lp[s] = a; seq_tokens[s] = tk; seq_hits[s] = hh;
  }
}

int launch_seq_reduce(const int* row0, const int* len, int n_seq, const int* labels, const float* lp, const int* amax,
                      double* seq_lp, int* seq_tokens, int* seq_hits, hipStream_t st) {
  if (n_seq <= 0) return ETD_OK;
  ProfScope ps("k_seq_reduce", st, 0, 0);
  hipLaunchKernelGGL(k_seq_reduce, dim3(n_seq), dim3(64), 0, st, row0, len, n_seq, labels, lp, amax, seq_lp, seq_tokens, seq_hits);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
