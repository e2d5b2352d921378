// Training engine of the EtudeDecoder: forward with saved activations, backward of F.cross_entropy for every parameter, gradient accumulation, global-norm
// clipping and AdamW (dec_train.h).  The model is the reference's (etude/models/etude_decoder.py:148-206 over HF GPT-NeoX) in its fp32 arithmetic;
// dropout is 0 in the reference's configuration, so train mode computes what eval mode computes.
//
// This file holds what is the decoder's own: attention, rotary embedding, the parallel residual, the embedding kernels, the cross-entropy and the engine.  The
// linear layers' products, LayerNorm, GELU, the column reductions, the norm and AdamW are train_kernels.hip's; the parameter store is train_store.h.
// Arithmetic: fp32 operands and fp32 accumulation everywhere.  The attention kernels keep one query (or key) row per lane and use fmaf chains.
// Order: no floating-point atomics.  Every sum -- an attention row, an embedding row's gradient -- runs in an order fixed by the shapes of the call, so the
// same call on the same inputs gives the same bits.
#include "dec_train.h"

#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "etude_hip.h"
#include "etude_hip_debug.h"
#include "train_store.h"

#define ETD_IGNORE_LABEL (-100)

// ================================================================================================
// attention: one row per lane, the other side's tile in LDS (every lane reads the same LDS address: a broadcast)
// ================================================================================================
// loads rows [t0, t0 + 64) x 64 floats of one head's slice (row stride ld floats) into tile[64][16] float4; rows at or past `len` read as 0
__device__ __forceinline__ void tile_load(f32x4 (*tile)[16], const float* __restrict__ base, long long ld, int t0, int len, int lane) {
  for (int e = lane; e < 64 * 16; e += 64) {
    const int r = e >> 4, c = e & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t0 + r < len) v = *(const f32x4*)(base + (long long)(t0 + r) * ld + 4 * c);
    tile[r][c] = v;
  }
}
__device__ __forceinline__ float dot64(const float (&a)[64], const f32x4* __restrict__ row) {
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 k4 = row[c];
    d = fmaf(a[4 * c], k4[0], d); d = fmaf(a[4 * c + 1], k4[1], d); d = fmaf(a[4 * c + 2], k4[2], d); d = fmaf(a[4 * c + 3], k4[3], d);
  }
  return d;
}
__device__ __forceinline__ void axpy64(float (&acc)[64], float s, const f32x4* __restrict__ row) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v4 = row[c];
    acc[4 * c] = fmaf(s, v4[0], acc[4 * c]); acc[4 * c + 1] = fmaf(s, v4[1], acc[4 * c + 1]);
    acc[4 * c + 2] = fmaf(s, v4[2], acc[4 * c + 2]); acc[4 * c + 3] = fmaf(s, v4[3], acc[4 * c + 3]);
  }
}
__device__ __forceinline__ void row_load(float (&a)[64], const float* __restrict__ p) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v = *(const f32x4*)(p + 4 * c);
    a[4 * c] = v[0]; a[4 * c + 1] = v[1]; a[4 * c + 2] = v[2]; a[4 * c + 3] = v[3];
  }
}
__device__ __forceinline__ void row_store(float* __restrict__ p, const float (&a)[64], float s) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v = {a[4 * c] * s, a[4 * c + 1] * s, a[4 * c + 2] * s, a[4 * c + 3] * s};
    *(f32x4*)(p + 4 * c) = v;
  }
}

// grid (query tiles, heads, sequences), 64 threads: lane = query row
__global__ __launch_bounds__(64) void k_tattn_fwd(const float* __restrict__ qkv, int nh, const int* __restrict__ row0, const int* __restrict__ lens,
                                                  float* __restrict__ O, float* __restrict__ lse) {
  __shared__ f32x4 Ks[64][16], Vs[64][16];
  const int qt = blockIdx.x, h = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  const int len = lens[s];
  if (qt * 64 >= len) return;                          // (uniform)
  const long long ld = 3LL * nh * 64;
  const float* base = qkv + (long long)row0[s] * ld + (long long)h * 192;
  const int qi = qt * 64 + lane;
  const bool valid = qi < len;
  float q[64], o[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) { q[d] = 0.f; o[d] = 0.f; }
  if (valid) row_load(q, base + (long long)qi * ld);
  float m = -INFINITY, lsum = 0.f;
  for (int kt = 0; kt <= qt; ++kt) {
    __syncthreads();
    tile_load(Ks, base + 64, ld, kt * 64, len, lane);
    tile_load(Vs, base + 128, ld, kt * 64, len, lane);
    __syncthreads();
    if (!valid) continue;
    const int kbase = kt * 64;
    for (int c = 0; c < 64; c += 16) {
      if (kbase + c > qi) break;
      float sc[16], cm = m;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float d = dot64(q, Ks[c + j]) * 0.125f;
        sc[j] = (kbase + c + j <= qi) ? d : -INFINITY;
        cm = fmaxf(cm, sc[j]);
      }
      const float alpha = expf(m - cm);              // (m = -inf on the first chunk: exp(-inf) = 0, and key 0 is never masked, so cm is finite)
      lsum *= alpha;
#pragma unroll
      for (int d = 0; d < 64; ++d) o[d] *= alpha;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float p = expf(sc[j] - cm);
        lsum += p;
        axpy64(o, p, Vs[c + j]);
      }
      m = cm;
    }
  }
  if (valid) {
    const long long r = row0[s] + qi;
    row_store(O + r * nh * 64 + h * 64, o, 1.f / lsum);
    lse[r * nh + h] = m + logf(lsum);
  }
}

// dQ and D: grid (query tiles, heads, sequences), lane = query row.  dq is written in the rotated space of q.
__global__ __launch_bounds__(64) void k_tattn_dq(const float* __restrict__ qkv, const float* __restrict__ O, const float* __restrict__ lse,
                                                 const float* __restrict__ dO, int nh, const int* __restrict__ row0, const int* __restrict__ lens,
                                                 float* __restrict__ Dbuf, float* __restrict__ dqkv) {
  __shared__ f32x4 Ks[64][16], Vs[64][16];
  const int qt = blockIdx.x, h = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  const int len = lens[s];
  if (qt * 64 >= len) return;
  const long long ld = 3LL * nh * 64;
  const float* base = qkv + (long long)row0[s] * ld + (long long)h * 192;
  const int qi = qt * 64 + lane;
  const bool valid = qi < len;
  const long long r = (long long)row0[s] + (valid ? qi : 0);
  float q[64], go[64], dq[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) { q[d] = 0.f; go[d] = 0.f; dq[d] = 0.f; }
  float D = 0.f, L = 0.f;
  if (valid) {
    row_load(q, base + (long long)qi * ld);
    row_load(go, dO + r * nh * 64 + h * 64);
    const float* orow = O + r * nh * 64 + h * 64;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const f32x4 v = *(const f32x4*)(orow + 4 * c);
      D = fmaf(go[4 * c], v[0], D); D = fmaf(go[4 * c + 1], v[1], D); D = fmaf(go[4 * c + 2], v[2], D); D = fmaf(go[4 * c + 3], v[3], D);
    }
    L = lse[r * nh + h];
    Dbuf[r * nh + h] = D;
  }
  for (int kt = 0; kt <= qt; ++kt) {
    __syncthreads();
    tile_load(Ks, base + 64, ld, kt * 64, len, lane);
    tile_load(Vs, base + 128, ld, kt * 64, len, lane);
    __syncthreads();
    if (!valid) continue;
    const int kbase = kt * 64;
    const int jn = min(64, qi - kbase + 1);           // keys kbase .. qi
    for (int j = 0; j < jn; ++j) {
      const float p = expf(dot64(q, Ks[j]) * 0.125f - L);
      const float dp = dot64(go, Vs[j]);
      axpy64(dq, p * (dp - D), Ks[j]);
    }
  }
  if (valid) row_store(dqkv + r * ld + (long long)h * 192, dq, 0.125f);
}

// dK and dV: grid (key tiles, heads, sequences), lane = key row; queries ascending
__global__ __launch_bounds__(64) void k_tattn_dkv(const float* __restrict__ qkv, const float* __restrict__ lse, const float* __restrict__ dO,
                                                  const float* __restrict__ Dbuf, int nh, const int* __restrict__ row0, const int* __restrict__ lens,
                                                  float* __restrict__ dqkv) {
  __shared__ f32x4 Qs[64][16], Gs[64][16];
  __shared__ float Ls[64], Ds[64];
  const int kt = blockIdx.x, h = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  const int len = lens[s];
  if (kt * 64 >= len) return;
  const long long ld = 3LL * nh * 64, r0 = row0[s];
  const float* base = qkv + r0 * ld + (long long)h * 192;
  const float* gbase = dO + r0 * nh * 64 + h * 64;
  const int kj = kt * 64 + lane;
  const bool valid = kj < len;
  float k[64], v[64], dk[64], dv[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) { k[d] = 0.f; v[d] = 0.f; dk[d] = 0.f; dv[d] = 0.f; }
  if (valid) { row_load(k, base + (long long)kj * ld + 64); row_load(v, base + (long long)kj * ld + 128); }
  const int n_tiles = (len + 63) / 64;
  for (int qt = kt; qt < n_tiles; ++qt) {
    __syncthreads();
    tile_load(Qs, base, ld, qt * 64, len, lane);
    tile_load(Gs, gbase, (long long)nh * 64, qt * 64, len, lane);
    {
      const int qi = qt * 64 + lane;
      Ls[lane] = qi < len ? lse[(r0 + qi) * nh + h] : 0.f;
      Ds[lane] = qi < len ? Dbuf[(r0 + qi) * nh + h] : 0.f;
    }
    __syncthreads();
    if (!valid) continue;
    const int in = min(64, len - qt * 64);
    const int i_first = max(0, kj - qt * 64);          // queries at or after this key
    for (int i = i_first; i < in; ++i) {
      const float p = expf(dot64(k, Qs[i]) * 0.125f - Ls[i]);
      axpy64(dv, p, Gs[i]);
      const float dp = dot64(v, Gs[i]);
      axpy64(dk, p * (dp - Ds[i]), Qs[i]);
    }
  }
  if (valid) {
    row_store(dqkv + (r0 + kj) * ld + (long long)h * 192 + 64, dk, 0.125f);
    row_store(dqkv + (r0 + kj) * ld + (long long)h * 192 + 128, dv, 1.f);
  }
}

static int attn_grid(int nh, int n_seq, int max_len, dim3* g) {
  if (nh < 1 || n_seq < 1 || max_len < 1) ETD_FAIL(ETD_EINVAL, "train attention: bad shape heads=%d sequences=%d length=%d", nh, n_seq, max_len);
  if (n_seq > 65535 || nh > 65535) ETD_FAIL(ETD_EINVAL, "train attention: more than 65535 sequences or heads in one call");
  *g = dim3((max_len + 63) / 64, nh, n_seq);
  return ETD_OK;
}
int launch_tattn_fwd(const float* qkv, int nh, const int* row0, const int* len, int n_seq, int max_len, float* O, float* lse, hipStream_t st) {
  dim3 g;
  ETD_TRY(attn_grid(nh, n_seq, max_len, &g));
  hipLaunchKernelGGL(k_tattn_fwd, g, dim3(64), 0, st, qkv, nh, row0, len, O, lse);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_tattn_bwd(const float* qkv, const float* O, const float* lse, const float* dO, int nh, const int* row0, const int* len, int n_seq, int max_len,
                     float* Dbuf, float* dqkv, hipStream_t st) {
  dim3 g;
  ETD_TRY(attn_grid(nh, n_seq, max_len, &g));
  hipLaunchKernelGGL(k_tattn_dq, g, dim3(64), 0, st, qkv, O, lse, dO, nh, row0, len, Dbuf, dqkv);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_tattn_dkv, g, dim3(64), 0, st, qkv, lse, dO, Dbuf, nh, row0, len, dqkv);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ================================================================================================
// row and elementwise kernels
// ================================================================================================
// rotate-half RoPE on the first 16 dims of q and k of every head, in place; sign = +1 forward, -1 the inverse rotation (backward).  tab [max_pos][16] = cos | sin
__global__ void k_trope(float* __restrict__ qkv, int nh, int M, const int* __restrict__ pos, const float* __restrict__ tab, float sign) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // (row, head, q|k, i < 8)
  if (e >= (long long)M * nh * 16) return;
  const int i = (int)(e & 7), which = (int)((e >> 3) & 1), h = (int)((e >> 4) % nh);
  const long long r = (e >> 4) / nh;
  float* p = qkv + r * 3LL * nh * 64 + (long long)h * 192 + which * 64;
  const float c = tab[pos[r] * 16 + i], sn = sign * tab[pos[r] * 16 + 8 + i];
  const float x1 = p[i], x2 = p[i + 8];
  p[i] = x1 * c - x2 * sn;
  p[i + 8] = x2 * c + x1 * sn;
}

// h_next = (mlp + attn) + h: the order of HF's parallel residual
__global__ void k_tadd3(const float* __restrict__ m, const float* __restrict__ a, const float* __restrict__ h, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (m[i] + a[i]) + h[i];
}
// the four attribute embeddings side by side: A[r][k * E + e] = table_k[attr_k[r]][e]
__global__ void k_tembed_gather(const int* __restrict__ attrs4, int M, int E, const float* t0, const float* t1, const float* t2, const float* t3,
                                float* __restrict__ A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * 4 * E) return;
  const int c = (int)(i % (4 * E)), k = c / E, e = c % E;
  const long long r = i / (4 * E);
  const float* t = k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3;
  A[i] = t[(long long)attrs4[(long long)k * M + r] * E + e];
}
// h = (word + class) + projected attributes (already in h)
__global__ void k_tembed_sum(const int* __restrict__ ids, const int* __restrict__ cls, const float* __restrict__ word, const float* __restrict__ cemb, int H,
                             float* __restrict__ h, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long r = i / H;
  const int c = (int)(i % H);
  h[i] = (word[(long long)ids[r] * H + c] + cemb[(long long)cls[r] * H + c]) + h[i];
}

// cross-entropy of one row, in place: logits -> (softmax - onehot) * scale, or zeros where the label is -100; row_loss = lse - logit[label] (0 where ignored)
__global__ __launch_bounds__(64) void k_tce(float* __restrict__ logits, int V, const int* __restrict__ labels, float scale, float* __restrict__ row_loss) {
  const int r = blockIdx.x, lane = threadIdx.x;
  float* lg = logits + (long long)r * V;
  const int lab = labels[r];
  if (lab == ETD_IGNORE_LABEL) {                       // (uniform)
    for (int v = lane; v < V; v += 64) lg[v] = 0.f;
    if (lane == 0) row_loss[r] = 0.f;
    return;
  }
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lg[v]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(lg[v] - mx);
  s = wave_sum(s);
  const float at = lg[lab];
  for (int v = lane; v < V; v += 64) {
    const float p = expf(lg[v] - mx) / s;
    lg[v] = (p - (v == lab ? 1.f : 0.f)) * scale;
  }
  if (lane == 0) row_loss[r] = (mx + logf(s)) - at;
}

// Embedding gradients.  The batch rows are grouped by table row on the host (a stable counting sort): segment g = rows order[start[g] .. start[g] + count[g]) ascending,
// all with index seg_id[g]; the padding row has no segment.  grid (segments, column blocks of 64), 4 row slices, summed as in k_tcolred.
__global__ __launch_bounds__(256) void k_tembed_grad(const float* __restrict__ src, int ld, int col0, int width, const int* __restrict__ order,
                                                     const int* __restrict__ seg_id, const int* __restrict__ seg_start, const int* __restrict__ seg_count,
                                                     float* __restrict__ grad) {
  __shared__ float part[4][64];
  const int g = blockIdx.x, t = threadIdx.x, c = blockIdx.y * 64 + (t & 63), s = t >> 6;
  const int st = seg_start[g], n = seg_count[g];
  float a = 0.f;
  if (c < width)
    for (int k = s; k < n; k += 4) a += src[(long long)order[st + k] * ld + col0 + c];
  part[s][t & 63] = a;
  __syncthreads();
  if (s == 0 && c < width) grad[(long long)seg_id[g] * width + c] += ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

// ================================================================================================
// launchers: each kernel above with its grid and block, called by the engine and by the stage taps at the end of this file
// ================================================================================================
static void launch_trope(float* qkv, int nh, int M, const int* pos, const float* tab, float sign, hipStream_t st) {
  hipLaunchKernelGGL(k_trope, ew_grid((long long)M * nh * 16), dim3(256), 0, st, qkv, nh, M, pos, tab, sign);
}
static void launch_tadd3(const float* m, const float* a, const float* h, float* out, long long n, hipStream_t st) {
  hipLaunchKernelGGL(k_tadd3, ew_grid(n), dim3(256), 0, st, m, a, h, out, n);
}
static void launch_tembed_gather(const int* attrs4, int M, int E, const float* t0, const float* t1, const float* t2, const float* t3, float* A, hipStream_t st) {
  hipLaunchKernelGGL(k_tembed_gather, ew_grid((long long)M * 4 * E), dim3(256), 0, st, attrs4, M, E, t0, t1, t2, t3, A);
}
static void launch_tembed_sum(const int* ids, const int* cls, const float* word, const float* cemb, int M, int H, float* h, hipStream_t st) {
  const long long n = (long long)M * H;
  hipLaunchKernelGGL(k_tembed_sum, ew_grid(n), dim3(256), 0, st, ids, cls, word, cemb, H, h, n);
}
static void launch_tce(float* logits, int M, int V, const int* labels, float scale, float* row_loss, hipStream_t st) {
  hipLaunchKernelGGL(k_tce, dim3(M), dim3(64), 0, st, logits, V, labels, scale, row_loss);
}
// grad [.][width] += the rows of src [.][ld] at columns [col0, col0 + width), by segment; a table none of whose rows has a segment is not launched
static void launch_tembed_grad(const float* src, int ld, int col0, int width, const int* order, const int* seg_id, const int* seg_start, const int* seg_count,
                               int n_seg, float* grad, hipStream_t st) {
  if (n_seg > 0) hipLaunchKernelGGL(k_tembed_grad, dim3(n_seg, (width + 63) / 64), dim3(256), 0, st, src, ld, col0, width, order, seg_id, seg_start, seg_count, grad);
}

// ================================================================================================
// the engine
// ================================================================================================
struct TLayer { size_t ln1_w, ln1_b, ln2_w, ln2_b, qkv_w, qkv_b, d_w, d_b, f1_w, f1_b, f2_w, f2_b; };

struct etd_dtrain {
  etd_dec_cfg cfg;
  int pad_token = 0, pad_class = 0, pad_attr = 0, max_rows = 0;
  int V = 0, H = 0, I = 0, L = 0, nh = 0, E = 0, NB = 0, NC = 0;
  TrainStore ps;                                      // the first n_train floats are trained; transformer.embed_in.weight sits behind them
  size_t word = 0, cemb = 0, attr[4] = {0, 0, 0, 0}, proj_w = 0, proj_b = 0, lnf_w = 0, lnf_b = 0, head = 0;
  std::vector<TLayer> layers;
  // saved activations
  float *A4 = nullptr, *dA4 = nullptr, *hs = nullptr, *mean = nullptr, *rstd = nullptr, *qkv = nullptr, *lse = nullptr, *att = nullptr, *pre = nullptr, *hf = nullptr;
  // workspace
  float *logits = nullptr, *wI = nullptr, *wH1 = nullptr, *wH2 = nullptr, *wH3 = nullptr, *dqkv = nullptr, *Dbuf = nullptr, *row_loss = nullptr, *rope = nullptr;
  int* ints = nullptr;
  size_t n_ints = 0;
  std::vector<float> h_row_loss;
  std::vector<int> h_ints;
  size_t workspace_bytes = 0;
  DevPool pool;
};

static int dtrain_check_cfg(const etd_dec_cfg* c, int max_rows) {
  if (!c) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: null config");
  if (c->struct_bytes != (int)sizeof(etd_dec_cfg)) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: etd_dec_cfg of %d bytes, this library's has %d", c->struct_bytes, (int)sizeof(etd_dec_cfg));
  if (c->vocab_size < 1 || c->hidden_size < 1 || c->num_hidden_layers < 0 || c->num_attention_heads < 1 || c->intermediate_size < 1 || c->num_classes < 1 ||
      c->attribute_emb_dim < 1 || c->num_attribute_bins < 1 || c->max_position_embeddings < 1)
    ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: a dimension is not positive");
  if (c->hidden_size != 64 * c->num_attention_heads) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: head_dim must be 64 (hidden %d, heads %d)", c->hidden_size, c->num_attention_heads);
  if ((int)(64 * c->rotary_pct) != 16) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: 16 rotary dims only (rotary_pct %g)", c->rotary_pct);
  if (c->hidden_size % 256) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: hidden_size %d is not a multiple of 256", c->hidden_size);
  if (c->intermediate_size % 128) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: intermediate_size %d is not a multiple of 128", c->intermediate_size);
  if (max_rows < 1 || max_rows > (1 << 22)) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: max_rows %d outside 1 .. 2^22", max_rows);
  return ETD_OK;
}

extern "C" long long etd_dtrain_workspace_bytes(const etd_dec_cfg* c, int max_rows) {
  if (dtrain_check_cfg(c, max_rows) != ETD_OK) return ETD_EINVAL;
  const long long H = c->hidden_size, I = c->intermediate_size, L = c->num_hidden_layers, nh = c->num_attention_heads, V = c->vocab_size, E = c->attribute_emb_dim;
  const long long saved = 8 * E + (L + 1) * H + L * (2 + 3 * H + nh + H + I) + 2 + H;      // floats per row kept from forward to backward
  const long long work = V + I + 3 * H + 3 * H + nh + 1;                                     // floats per row of scratch
  return 4 * (saved + work) * (long long)max_rows;
}

extern "C" int etd_dtrain_create(const etd_dec_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n,
                                 int pad_token_id, int pad_class_id, int attribute_pad_id, int max_rows, etd_dtrain** out) {
  if (!out) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: null out");
  *out = nullptr;
  ETD_TRY(dtrain_check_cfg(cfg, max_rows));
  const etd_dec_cfg& c = *cfg;
  if (pad_token_id < 0 || pad_token_id >= c.vocab_size || pad_class_id < 0 || pad_class_id >= c.num_classes || attribute_pad_id < 0 || attribute_pad_id >= c.num_attribute_bins)
    ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: a padding index lies outside its table");
  if (!names || !host_ptrs || !numels || n < 1) ETD_FAIL(ETD_EINVAL, "etd_dtrain_create: no weights");
  etd_dtrain* d = new etd_dtrain();
  auto fail = [&](int rc) { d->pool.free_all(); delete d; return rc; };
  d->cfg = c; d->pad_token = pad_token_id; d->pad_class = pad_class_id; d->pad_attr = attribute_pad_id; d->max_rows = max_rows;
  d->V = c.vocab_size; d->H = c.hidden_size; d->I = c.intermediate_size; d->L = c.num_hidden_layers; d->nh = c.num_attention_heads;
  d->E = c.attribute_emb_dim; d->NB = c.num_attribute_bins; d->NC = c.num_classes;
  const size_t V = d->V, H = d->H, I = d->I, E = d->E;
  TrainStore& ps = d->ps;
  d->word = ps.add("word_embeddings.weight", V * H);
  d->cemb = ps.add("class_embeddings.weight", (size_t)d->NC * H);
  static const char* attr_names[4] = {"pitch_overlap", "polyphony", "note_sustain", "rhythm_intensity"};      // the concat order of etude_decoder.py:171-176
  for (int k = 0; k < 4; ++k) d->attr[k] = ps.add(std::string(attr_names[k]) + "_embeddings.weight", (size_t)d->NB * E);
  d->proj_w = ps.add("attribute_projection.weight", H * 4 * E);
  d->proj_b = ps.add("attribute_projection.bias", H);
  for (int i = 0; i < d->L; ++i) {
    const std::string p = "transformer.layers." + std::to_string(i) + ".";
    TLayer y;
    y.ln1_w = ps.add(p + "input_layernorm.weight", H); y.ln1_b = ps.add(p + "input_layernorm.bias", H);
    y.ln2_w = ps.add(p + "post_attention_layernorm.weight", H); y.ln2_b = ps.add(p + "post_attention_layernorm.bias", H);
    y.qkv_w = ps.add(p + "attention.query_key_value.weight", 3 * H * H); y.qkv_b = ps.add(p + "attention.query_key_value.bias", 3 * H);
    y.d_w = ps.add(p + "attention.dense.weight", H * H); y.d_b = ps.add(p + "attention.dense.bias", H);
    y.f1_w = ps.add(p + "mlp.dense_h_to_4h.weight", I * H); y.f1_b = ps.add(p + "mlp.dense_h_to_4h.bias", I);
    y.f2_w = ps.add(p + "mlp.dense_4h_to_h.weight", H * I); y.f2_b = ps.add(p + "mlp.dense_4h_to_h.bias", H);
    d->layers.push_back(y);
  }
  d->lnf_w = ps.add("transformer.final_layer_norm.weight", H);
  d->lnf_b = ps.add("transformer.final_layer_norm.bias", H);
  d->head = ps.add("lm_head.weight", V * H);
  ps.n_train = ps.n_total;
  // GPTNeoXModel's own token table: part of the state dict, never read (the model is fed inputs_embeds), so autograd gives it no gradient and
  // torch.optim.AdamW leaves it alone, weight decay included.  It is kept, saved and never changed.
  ps.add("transformer.embed_in.weight", V * H);
  // host image of the parameters, checked before the device is touched
  WeightTable wt(names, host_ptrs, numels, n);
  std::vector<float> host(ps.n_total, 0.f);
  ETD_TRY_OR(fail, ps.fill(wt, host.data()));
  std::vector<float> rope((size_t)c.max_position_embeddings * 16);
  for (int pos = 0; pos < c.max_position_embeddings; ++pos)
    for (int i = 0; i < 8; ++i) {                      // modeling_gpt_neox.py:72-109 in fp32: inv_freq, pos * inv_freq, then cos / sin of that fp32 angle
      const float inv = 1.0f / powf(c.rope_theta, (float)(2 * i) / 16.0f);
      const float fr = (float)pos * inv;
      rope[(size_t)pos * 16 + i] = (float)cos((double)fr);
      rope[(size_t)pos * 16 + 8 + i] = (float)sin((double)fr);
    }
  // ---- device
  DevPool& pl = d->pool;
  ETD_TRY_OR(fail, ps.upload(pl, host.data(), ps.n_total));
  ETD_TRY_OR(fail, (pl.upload<float, float>(&d->rope, rope.data(), rope.size())));
  const size_t R = (size_t)max_rows, Lz = (size_t)d->L, nh = (size_t)d->nh;
  const size_t before = pl.mark();
  ETD_TRY_OR(fail, pl.alloc(&d->A4, R * 4 * E));
  ETD_TRY_OR(fail, pl.alloc(&d->dA4, R * 4 * E));
  ETD_TRY_OR(fail, pl.alloc(&d->hs, (Lz + 1) * R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->mean, (Lz + 1) * R));
  ETD_TRY_OR(fail, pl.alloc(&d->rstd, (Lz + 1) * R));
  ETD_TRY_OR(fail, pl.alloc(&d->qkv, std::max<size_t>(Lz, 1) * R * 3 * H));
  ETD_TRY_OR(fail, pl.alloc(&d->lse, std::max<size_t>(Lz, 1) * R * nh));
  ETD_TRY_OR(fail, pl.alloc(&d->att, std::max<size_t>(Lz, 1) * R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->pre, std::max<size_t>(Lz, 1) * R * I));
  ETD_TRY_OR(fail, pl.alloc(&d->hf, R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->logits, R * V));
  ETD_TRY_OR(fail, pl.alloc(&d->wI, R * I));
  ETD_TRY_OR(fail, pl.alloc(&d->wH1, R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->wH2, R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->wH3, R * H));
  ETD_TRY_OR(fail, pl.alloc(&d->dqkv, R * 3 * H));
  ETD_TRY_OR(fail, pl.alloc(&d->Dbuf, R * nh));
  ETD_TRY_OR(fail, pl.alloc(&d->row_loss, R));
  ETD_TRY_OR(fail, pl.alloc(&ps.partial, (size_t)TN_BLOCKS));
  // ints: ids, cls, attrs4 [4], labels, pos (8 R) | row0, len (2 R) | six sort orders (6 R) | segments: id, start, count of at most V + NC + 4 NB table rows
  d->n_ints = 16 * R + 3 * (V + (size_t)d->NC + 4 * (size_t)d->NB);
  ETD_TRY_OR(fail, pl.alloc(&d->ints, d->n_ints));
  for (size_t i = before; i < pl.bytes.size(); ++i) d->workspace_bytes += pl.bytes[i];
  d->h_row_loss.resize(R);
  *out = d;
  return ETD_OK;
}

extern "C" void etd_dtrain_destroy(etd_dtrain* d) {
  if (!d) return;
  d->pool.free_all();
  delete d;
}

extern "C" long long etd_dtrain_bytes(const etd_dtrain* d, int what) {
  if (!d) return ETD_EINVAL;
  return what == 0 ? (long long)d->workspace_bytes : (long long)(4 * d->ps.n_total * sizeof(float));      // 0: activations + scratch; 1: weights, gradients, two moments
}

// stable grouping of M rows by table index: order / segments appended to `ints` at (o_order, o_seg ..); returns the number of segments (the padding row has none)
static int group_rows(const int32_t* idx, int M, int n_rows, int pad, int* order, int* seg_id, int* seg_start, int* seg_count) {
  std::vector<int> cnt(n_rows + 1, 0);
  for (int r = 0; r < M; ++r) ++cnt[idx[r] + 1];
  for (int i = 0; i < n_rows; ++i) cnt[i + 1] += cnt[i];
  std::vector<int> at(cnt.begin(), cnt.end() - 1);
  for (int r = 0; r < M; ++r) order[at[idx[r]]++] = r;
  int ns = 0;
  for (int i = 0; i < n_rows; ++i) {
    const int c = cnt[i + 1] - cnt[i];
    if (c == 0 || i == pad) continue;
    seg_id[ns] = i; seg_start[ns] = cnt[i]; seg_count[ns] = c; ++ns;
  }
  return ns;
}

extern "C" int etd_dtrain_forward_backward(etd_dtrain* d, int n, const int32_t* T, const int32_t* ids, const int32_t* cls, const int32_t* attrs4,
                                           const int32_t* labels, float loss_scale, float* loss_out, int32_t* n_scored_out, void* stream) {
  if (!d || !T || !ids || !cls || !attrs4 || !labels || !loss_out || !n_scored_out) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: null argument");
  if (n < 1 || n > 65535) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: %d sequences (1 .. 65535)", n);
  long long Ml = 0;
  int max_len = 0;
  for (int s = 0; s < n; ++s) {
    if (T[s] < 1 || T[s] > d->cfg.max_position_embeddings) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: sequence %d has %d rows (1 .. max_position_embeddings = %d)", s, T[s], d->cfg.max_position_embeddings);
    Ml += T[s];
    max_len = std::max(max_len, (int)T[s]);
  }
  if (Ml > d->max_rows) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: %lld rows, the workspace was sized for %d", Ml, d->max_rows);
  const int M = (int)Ml;
  int scored = 0;
  for (int r = 0; r < M; ++r) {
    if (ids[r] < 0 || ids[r] >= d->V) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: token id %d out of range [0, %d) at row %d", ids[r], d->V, r);
    if (cls[r] < 0 || cls[r] >= d->NC) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: class id %d out of range [0, %d) at row %d", cls[r], d->NC, r);
    for (int k = 0; k < 4; ++k)
      if (attrs4[(size_t)k * M + r] < 0 || attrs4[(size_t)k * M + r] >= d->NB)
        ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: attribute bin %d out of range [0, %d) at row %d", attrs4[(size_t)k * M + r], d->NB, r);
    if (labels[r] != ETD_IGNORE_LABEL && (labels[r] < 0 || labels[r] >= d->V)) ETD_FAIL(ETD_EINVAL, "etd_dtrain_forward_backward: label %d out of range at row %d", labels[r], r);
    scored += labels[r] != ETD_IGNORE_LABEL;
  }
  *n_scored_out = scored;
  if (scored == 0) {                                   // F.cross_entropy gives nan; train.py:169 skips the batch.  Nothing is launched: the gradients keep every bit.
    *loss_out = NAN;
    return ETD_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  const int H = d->H, I = d->I, V = d->V, E = d->E, nh = d->nh, L = d->L;
  const size_t R = (size_t)d->max_rows;
  // ---- the call's integers, one upload
  std::vector<int>& hi = d->h_ints;
  hi.assign(d->n_ints, 0);
  int* h_ids = hi.data(); int* h_cls = h_ids + R; int* h_at = h_cls + R; int* h_lab = h_at + 4 * R; int* h_pos = h_lab + R;
  int* h_row0 = h_pos + R; int* h_len = h_row0 + R; int* h_ord = h_len + R; int* h_seg = h_ord + 6 * R;
  memcpy(h_ids, ids, sizeof(int) * M); memcpy(h_cls, cls, sizeof(int) * M); memcpy(h_lab, labels, sizeof(int) * M);
  for (int k = 0; k < 4; ++k) memcpy(h_at + (size_t)k * M, attrs4 + (size_t)k * M, sizeof(int) * M);
  for (int s = 0, r = 0; s < n; ++s) {
    h_row0[s] = r; h_len[s] = T[s];
    for (int t = 0; t < T[s]; ++t) h_pos[r++] = t;
  }
  const size_t seg_cap = (size_t)V + d->NC + 4 * (size_t)d->NB;
  int* h_sid = h_seg; int* h_sst = h_seg + seg_cap; int* h_scn = h_seg + 2 * seg_cap;
  int seg0[7];
  seg0[0] = 0;
  seg0[1] = group_rows(ids, M, V, d->pad_token, h_ord, h_sid, h_sst, h_scn);
  seg0[2] = seg0[1] + group_rows(cls, M, d->NC, d->pad_class, h_ord + R, h_sid + seg0[1], h_sst + seg0[1], h_scn + seg0[1]);
  for (int k = 0; k < 4; ++k)
    seg0[3 + k] = seg0[2 + k] + group_rows(attrs4 + (size_t)k * M, M, d->NB, d->pad_attr, h_ord + (2 + k) * R, h_sid + seg0[2 + k], h_sst + seg0[2 + k], h_scn + seg0[2 + k]);
  HIP_TRY(hipMemcpyAsync(d->ints, hi.data(), sizeof(int) * d->n_ints, hipMemcpyHostToDevice, st));
  const int* ii = d->ints;
  const int *d_ids = ii, *d_cls = ii + R, *d_at = ii + 2 * R, *d_lab = ii + 6 * R, *d_pos = ii + 7 * R, *d_row0 = ii + 8 * R, *d_len = ii + 9 * R, *d_ord = ii + 10 * R;
  const int *d_sid = ii + 16 * R, *d_sst = d_sid + seg_cap, *d_scn = d_sid + 2 * seg_cap;
  float* P = d->ps.P;
  float* G = d->ps.G;
  const long long MH = (long long)M * H, MI = (long long)M * I;
  const float eps = d->cfg.layer_norm_eps;
  // ================================================================ forward
  {
    ProfScope ps("dtrain_forward", st);
    launch_tembed_gather(d_at, M, E, P + d->attr[0], P + d->attr[1], P + d->attr[2], P + d->attr[3], d->A4, st);
    ETD_TRY(launch_tgemm(ETD_TG_NT, M, H, 4 * E, d->A4, 4 * E, P + d->proj_w, 4 * E, P + d->proj_b, d->hs, H, false, st));
    launch_tembed_sum(d_ids, d_cls, P + d->word, P + d->cemb, M, H, d->hs, st);
    for (int l = 0; l < L; ++l) {
      const TLayer& y = d->layers[l];
      float* h = d->hs + (size_t)l * R * H;
      float* qkv = d->qkv + (size_t)l * R * 3 * H;
      float* att = d->att + (size_t)l * R * H;
      float* pre = d->pre + (size_t)l * R * I;
      launch_tln_fwd(h, M, H, eps, d->mean + (size_t)l * R, d->rstd + (size_t)l * R, P + y.ln1_w, P + y.ln1_b, d->wH1, P + y.ln2_w, P + y.ln2_b, d->wH2, st);
      ETD_TRY(launch_tgemm(ETD_TG_NT, M, 3 * H, H, d->wH1, H, P + y.qkv_w, H, P + y.qkv_b, qkv, 3 * H, false, st));
      launch_trope(qkv, nh, M, d_pos, d->rope, 1.f, st);
      ETD_TRY(launch_tattn_fwd(qkv, nh, d_row0, d_len, n, max_len, att, d->lse + (size_t)l * R * nh, st));
      ETD_TRY(launch_tgemm(ETD_TG_NT, M, H, H, att, H, P + y.d_w, H, P + y.d_b, d->wH1, H, false, st));          // wH1: attention branch
      ETD_TRY(launch_tgemm(ETD_TG_NT, M, I, H, d->wH2, H, P + y.f1_w, H, P + y.f1_b, pre, I, false, st));
      launch_tgelu(pre, d->wI, MI, st);
      ETD_TRY(launch_tgemm(ETD_TG_NT, M, H, I, d->wI, I, P + y.f2_w, I, P + y.f2_b, d->wH3, H, false, st));       // wH3: MLP branch
      launch_tadd3(d->wH3, d->wH1, h, h + R * H, MH, st);
    }
    launch_tln_fwd(d->hs + (size_t)L * R * H, M, H, eps, d->mean + (size_t)L * R, d->rstd + (size_t)L * R, P + d->lnf_w, P + d->lnf_b, d->hf, nullptr, nullptr,
                   nullptr, st);
    ETD_TRY(launch_tgemm(ETD_TG_NT, M, V, H, d->hf, H, P + d->head, H, nullptr, d->logits, V, false, st));
    launch_tce(d->logits, M, V, d_lab, loss_scale / (float)scored, d->row_loss, st);
    HIP_TRY(hipGetLastError());
  }
  // ================================================================ backward
  {
    ProfScope ps("dtrain_backward", st);
    float* dh = d->wH1;                                // gradient of the residual stream
    float* tx = d->wH2;                                // a recomputed LayerNorm output
    float* dxn = d->wH3;                               // gradient of a LayerNorm output / of the attention output
    ETD_TRY(launch_tgemm(ETD_TG_TN, V, H, M, d->logits, V, d->hf, H, nullptr, G + d->head, H, true, st));
    ETD_TRY(launch_tgemm(ETD_TG_NN, M, H, V, d->logits, V, P + d->head, H, nullptr, dxn, H, false, st));
    launch_tcolred(1, dxn, H, M, H, d->hs + (size_t)L * R * H, d->mean + (size_t)L * R, d->rstd + (size_t)L * R, G + d->lnf_b, G + d->lnf_w, st);
    HIP_TRY(hipMemsetAsync(dh, 0, sizeof(float) * MH, st));
    launch_tln_bwd(dxn, d->hs + (size_t)L * R * H, d->mean + (size_t)L * R, d->rstd + (size_t)L * R, P + d->lnf_w, M, H, dh, st);
    for (int l = L - 1; l >= 0; --l) {
      const TLayer& y = d->layers[l];
      const float* h = d->hs + (size_t)l * R * H;
      const float* mean = d->mean + (size_t)l * R;
      const float* rstd = d->rstd + (size_t)l * R;
      const float* qkv = d->qkv + (size_t)l * R * 3 * H;
      const float* att = d->att + (size_t)l * R * H;
      const float* pre = d->pre + (size_t)l * R * I;
      // dh is d loss / d (mlp + attn + h): the gradient of both branch outputs, and (kept) of h through the residual
      // ---- MLP branch
      launch_tgelu(pre, d->wI, MI, st);
      ETD_TRY(launch_tgemm(ETD_TG_TN, H, I, M, dh, H, d->wI, I, nullptr, G + y.f2_w, I, true, st));
      launch_tcolred(0, dh, H, M, H, nullptr, nullptr, nullptr, G + y.f2_b, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_NN, M, I, H, dh, H, P + y.f2_w, I, nullptr, d->wI, I, false, st));
      launch_tgelu_bwd(pre, d->wI, MI, st);
      launch_tln_fwd(h, M, H, eps, nullptr, nullptr, P + y.ln2_w, P + y.ln2_b, tx, nullptr, nullptr, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_TN, I, H, M, d->wI, I, tx, H, nullptr, G + y.f1_w, H, true, st));
      launch_tcolred(0, d->wI, I, M, I, nullptr, nullptr, nullptr, G + y.f1_b, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_NN, M, H, I, d->wI, I, P + y.f1_w, H, nullptr, dxn, H, false, st));
      launch_tcolred(1, dxn, H, M, H, h, mean, rstd, G + y.ln2_b, G + y.ln2_w, st);
      // ---- attention branch (before dh takes the LayerNorm terms: both branches read the incoming dh)
      ETD_TRY(launch_tgemm(ETD_TG_TN, H, H, M, dh, H, att, H, nullptr, G + y.d_w, H, true, st));
      launch_tcolred(0, dh, H, M, H, nullptr, nullptr, nullptr, G + y.d_b, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_NN, M, H, H, dh, H, P + y.d_w, H, nullptr, tx, H, false, st));                 // tx: d loss / d attention output
      launch_tln_bwd(dxn, h, mean, rstd, P + y.ln2_w, M, H, dh, st);                                              // (the MLP branch's LayerNorm, now that dh has been read)
      ETD_TRY(launch_tattn_bwd(qkv, att, d->lse + (size_t)l * R * nh, tx, nh, d_row0, d_len, n, max_len, d->Dbuf, d->dqkv, st));
      launch_trope(d->dqkv, nh, M, d_pos, d->rope, -1.f, st);
      launch_tln_fwd(h, M, H, eps, nullptr, nullptr, P + y.ln1_w, P + y.ln1_b, tx, nullptr, nullptr, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_TN, 3 * H, H, M, d->dqkv, 3 * H, tx, H, nullptr, G + y.qkv_w, H, true, st));
      launch_tcolred(0, d->dqkv, 3 * H, M, 3 * H, nullptr, nullptr, nullptr, G + y.qkv_b, nullptr, st);
      ETD_TRY(launch_tgemm(ETD_TG_NN, M, H, 3 * H, d->dqkv, 3 * H, P + y.qkv_w, H, nullptr, dxn, H, false, st));
      launch_tcolred(1, dxn, H, M, H, h, mean, rstd, G + y.ln1_b, G + y.ln1_w, st);
      launch_tln_bwd(dxn, h, mean, rstd, P + y.ln1_w, M, H, dh, st);
    }
    // ---- embeddings: dh is d loss / d inputs_embeds
    ETD_TRY(launch_tgemm(ETD_TG_TN, H, 4 * E, M, dh, H, d->A4, 4 * E, nullptr, G + d->proj_w, 4 * E, true, st));
    launch_tcolred(0, dh, H, M, H, nullptr, nullptr, nullptr, G + d->proj_b, nullptr, st);
    ETD_TRY(launch_tgemm(ETD_TG_NN, M, 4 * E, H, dh, H, P + d->proj_w, 4 * E, nullptr, d->dA4, 4 * E, false, st));
    launch_tembed_grad(dh, H, 0, H, d_ord, d_sid, d_sst, d_scn, seg0[1], G + d->word, st);
    launch_tembed_grad(dh, H, 0, H, d_ord + R, d_sid + seg0[1], d_sst + seg0[1], d_scn + seg0[1], seg0[2] - seg0[1], G + d->cemb, st);
    for (int k = 0; k < 4; ++k)
      launch_tembed_grad(d->dA4, 4 * E, k * E, E, d_ord + (2 + k) * R, d_sid + seg0[2 + k], d_sst + seg0[2 + k], d_scn + seg0[2 + k], seg0[3 + k] - seg0[2 + k],
                         G + d->attr[k], st);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(d->h_row_loss.data(), d->row_loss, sizeof(float) * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double tot = 0.0;
  for (int r = 0; r < M; ++r) tot += (double)d->h_row_loss[r];      // row order; rows that are not scored hold 0
  *loss_out = (float)(tot / (double)scored);
  return ETD_OK;
}

extern "C" int etd_dtrain_zero_grad(etd_dtrain* d, void* stream) {
  if (!d) ETD_FAIL(ETD_EINVAL, "etd_dtrain_zero_grad: null handle");
  return d->ps.zero_grad(d->ps.n_total, (hipStream_t)stream);
}

extern "C" int etd_dtrain_grad_norm(etd_dtrain* d, double* norm, void* stream) {
  if (!d || !norm) ETD_FAIL(ETD_EINVAL, "etd_dtrain_grad_norm: null argument");
  return d->ps.grad_norm(d->ps.n_train, (hipStream_t)stream, norm);
}

extern "C" int etd_dtrain_clip_and_step(etd_dtrain* d, double max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, double* norm_out,
                                        void* stream) {
  if (!d) ETD_FAIL(ETD_EINVAL, "etd_dtrain_clip_and_step: null handle");
  return adamw_step(d->ps, d->ps.n_train, "etd_dtrain_clip_and_step", "dtrain_optimizer", max_norm, lr, beta1, beta2, eps, weight_decay, norm_out, (hipStream_t)stream);
}

extern "C" int etd_dtrain_set_step(etd_dtrain* d, long long step) {
  if (!d || step < 0) ETD_FAIL(ETD_EINVAL, "etd_dtrain_set_step: null handle or negative step");
  d->ps.step = step;
  return ETD_OK;
}
extern "C" long long etd_dtrain_get_step(const etd_dtrain* d) { return d ? d->ps.step : ETD_EINVAL; }

static TrainStore* dstore(etd_dtrain* d) { return d ? &d->ps : nullptr; }      // (train_io refuses a null handle with its other null arguments)
extern "C" int etd_dtrain_read_param(etd_dtrain* d, const char* name, float* out_host, long long numel, void* stream) {
  return train_io(dstore(d), "etd_dtrain", name, 0, out_host, nullptr, numel, (hipStream_t)stream);
}
extern "C" int etd_dtrain_read_grad(etd_dtrain* d, const char* name, float* out_host, long long numel, void* stream) {
  return train_io(dstore(d), "etd_dtrain", name, 1, out_host, nullptr, numel, (hipStream_t)stream);
}
extern "C" int etd_dtrain_read_moment(etd_dtrain* d, const char* name, int second, float* out_host, long long numel, void* stream) {
  return train_io(dstore(d), "etd_dtrain", name, second ? 3 : 2, out_host, nullptr, numel, (hipStream_t)stream);
}
extern "C" int etd_dtrain_write_moment(etd_dtrain* d, const char* name, int second, const float* in_host, long long numel, void* stream) {
  return train_io(dstore(d), "etd_dtrain", name, second ? 3 : 2, nullptr, in_host, numel, (hipStream_t)stream);
}

// ================================================================================================
// debug entries (include/etude_hip_debug.h): the two kernels with tile edges, on their own inputs
// ================================================================================================
extern "C" int etd_debug_dtrain_gemm(int form, int M, int N, int K, const float* A_dev, int lda, const float* B_dev, int ldb, const float* bias_dev, float* C_dev,
                                     int ldc, int accumulate, void* stream) {
  return launch_tgemm(form, M, N, K, A_dev, lda, B_dev, ldb, bias_dev, C_dev, ldc, accumulate != 0, (hipStream_t)stream);
}

extern "C" int etd_debug_dtrain_attn(int n_seq, const int32_t* T_host, int n_heads, const float* qkv_dev, const float* dO_dev, float* O_dev, float* lse_dev,
                                     float* dqkv_dev, void* stream) {
  if (n_seq < 1 || n_seq > 65535 || !T_host || n_heads < 1 || !qkv_dev || !dO_dev || !O_dev || !lse_dev || !dqkv_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_attn: bad argument");
  std::vector<int> h(2 * (size_t)n_seq);
  long long M = 0;
  int max_len = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (T_host[s] < 1) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_attn: empty sequence %d", s);
    h[s] = (int)M; h[n_seq + s] = T_host[s];
    M += T_host[s];
    max_len = std::max(max_len, (int)T_host[s]);
  }
  if (M > (1 << 22)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_attn: %lld rows", M);
  hipStream_t st = (hipStream_t)stream;
  DevPool pl;
  int* di = nullptr;
  float* Dbuf = nullptr;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(st); pl.free_all(); return rc; };
  ETD_TRY_OR(fail, pl.alloc(&di, h.size()));
  ETD_TRY_OR(fail, pl.alloc(&Dbuf, (size_t)M * n_heads));
  ETD_TRY_OR(fail, ETD_HIP_RC(hipMemcpyAsync(di, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st)));
  ETD_TRY_OR(fail, launch_tattn_fwd(qkv_dev, n_heads, di, di + n_seq, n_seq, max_len, O_dev, lse_dev, st));
  ETD_TRY_OR(fail, launch_tattn_bwd(qkv_dev, O_dev, lse_dev, dO_dev, n_heads, di, di + n_seq, n_seq, max_len, Dbuf, dqkv_dev, st));
  return fail(ETD_HIP_RC(hipStreamSynchronize(st)));
}

// ================================================================================================
// stage taps (include/etude_hip_debug.h): every row and elementwise kernel on a caller's input, through the launcher the engine calls
// ================================================================================================
#define TAP_MAX_ROWS (1 << 22)          // etd_dtrain_create's limit of max_rows
#define TAP_MAX_ELEMS (1LL << 36)       // elementwise taps: the grid of ew_grid stays below 2^31 workgroups

extern "C" int etd_debug_dtrain_ln(const float* x_dev, int M, int H, float eps, float* mean_dev, float* rstd_dev, const float* g1_dev, const float* b1_dev,
                                   float* y1_dev, const float* g2_dev, const float* b2_dev, float* y2_dev, const float* dy_dev, float* dx_dev, void* stream) {
  if (!x_dev || !g1_dev || !b1_dev || !y1_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: x, the first gain and bias and y1 are required");
  if (M < 1 || M > TAP_MAX_ROWS || H < 1 || !(eps >= 0.f)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: bad shape M=%d H=%d eps=%g", M, H, (double)eps);
  if ((mean_dev == nullptr) != (rstd_dev == nullptr)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: mean and rstd go together");
  if ((y2_dev != nullptr) != (g2_dev != nullptr) || (y2_dev != nullptr) != (b2_dev != nullptr)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: y2, g2 and b2 go together");
  if ((dy_dev != nullptr) != (dx_dev != nullptr)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: dy and dx go together");
  if (dy_dev && !mean_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ln: the backward pass reads the saved mean and rstd");
  hipStream_t st = (hipStream_t)stream;
  launch_tln_fwd(x_dev, M, H, eps, mean_dev, rstd_dev, g1_dev, b1_dev, y1_dev, g2_dev, b2_dev, y2_dev, st);
  if (dy_dev) launch_tln_bwd(dy_dev, x_dev, mean_dev, rstd_dev, g1_dev, M, H, dx_dev, st);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_gelu(const float* x_dev, long long n, float* y_dev, float* dy_dev, void* stream) {
  if (!x_dev || !y_dev || n < 1 || n > TAP_MAX_ELEMS) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_gelu: null buffer or n=%lld outside 1 .. 2^36", n);
  launch_tgelu(x_dev, y_dev, n, (hipStream_t)stream);
  if (dy_dev) launch_tgelu_bwd(x_dev, dy_dev, n, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_add3(const float* m_dev, const float* a_dev, const float* h_dev, long long n, float* out_dev, void* stream) {
  if (!m_dev || !a_dev || !h_dev || !out_dev || n < 1 || n > TAP_MAX_ELEMS) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_add3: null buffer or n=%lld outside 1 .. 2^36", n);
  launch_tadd3(m_dev, a_dev, h_dev, out_dev, n, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_rope(etd_dtrain* d, float* qkv_dev, int n_heads, int M, const int32_t* pos_dev, int sign, void* stream) {
  if (!d || !qkv_dev || !pos_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_rope: null argument");
  if (n_heads < 1 || n_heads > 65535 || M < 1 || M > TAP_MAX_ROWS || (sign != 1 && sign != -1))
    ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_rope: bad shape heads=%d M=%d sign=%d", n_heads, M, sign);
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> pos((size_t)M);                 // read back: a position past the handle's table must not reach the kernel
  HIP_TRY(hipMemcpyAsync(pos.data(), pos_dev, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int r = 0; r < M; ++r)
    if (pos[r] < 0 || pos[r] >= d->cfg.max_position_embeddings)
      ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_rope: position %d at row %d outside [0, %d)", pos[r], r, d->cfg.max_position_embeddings);
  launch_trope(qkv_dev, n_heads, M, pos_dev, d->rope, (float)sign, st);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// `n` host ints on the device for the length of one tap
static int tap_upload(DevPool& pl, const std::vector<int>& h, int** out, hipStream_t st) {
  ETD_TRY(pl.alloc(out, h.size()));
  HIP_TRY(hipMemcpyAsync(*out, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st));
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_embed(int M, int H, int E, int V, int NC, int NB, const int32_t* ids_host, const int32_t* cls_host, const int32_t* attrs4_host,
                                      const float* word_dev, const float* cemb_dev, const float* attr0_dev, const float* attr1_dev, const float* attr2_dev,
                                      const float* attr3_dev, const float* h_in_dev, float* A4_dev, float* h_dev, void* stream) {
  if (!ids_host || !cls_host || !attrs4_host || !word_dev || !cemb_dev || !attr0_dev || !attr1_dev || !attr2_dev || !attr3_dev || !h_in_dev || !A4_dev || !h_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed: null argument");
  if (M < 1 || M > TAP_MAX_ROWS || H < 1 || E < 1 || V < 1 || NC < 1 || NB < 1 || (long long)M * 4 * E > TAP_MAX_ELEMS || (long long)M * H > TAP_MAX_ELEMS)
    ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed: bad shape M=%d H=%d E=%d V=%d NC=%d NB=%d", M, H, E, V, NC, NB);
  std::vector<int> h(6 * (size_t)M);                    // ids | cls | attrs4 [4][M]
  for (int r = 0; r < M; ++r) {
    if (ids_host[r] < 0 || ids_host[r] >= V || cls_host[r] < 0 || cls_host[r] >= NC) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed: token or class id out of range at row %d", r);
    h[r] = ids_host[r]; h[(size_t)M + r] = cls_host[r];
    for (int k = 0; k < 4; ++k) {
      const int a = attrs4_host[(size_t)k * M + r];
      if (a < 0 || a >= NB) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed: attribute bin %d out of range [0, %d) at row %d", a, NB, r);
      h[(2 + (size_t)k) * M + r] = a;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  DevPool pl;
  int* di = nullptr;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(st); pl.free_all(); return rc; };
  ETD_TRY_OR(fail, tap_upload(pl, h, &di, st));
  launch_tembed_gather(di + 2 * (size_t)M, M, E, attr0_dev, attr1_dev, attr2_dev, attr3_dev, A4_dev, st);
  if (h_dev != h_in_dev) ETD_TRY_OR(fail, ETD_HIP_RC(hipMemcpyAsync(h_dev, h_in_dev, sizeof(float) * (size_t)M * H, hipMemcpyDeviceToDevice, st)));
  launch_tembed_sum(di, di + M, word_dev, cemb_dev, M, H, h_dev, st);
  ETD_TRY_OR(fail, ETD_HIP_RC(hipGetLastError()));
  return fail(ETD_HIP_RC(hipStreamSynchronize(st)));
}

extern "C" int etd_debug_dtrain_ce(float* logits_dev, int M, int V, const int32_t* labels_host, float scale, float* row_loss_dev, void* stream) {
  if (!logits_dev || !labels_host || !row_loss_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ce: null argument");
  if (M < 1 || M > TAP_MAX_ROWS || V < 1) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ce: bad shape M=%d V=%d", M, V);
  std::vector<int> h((size_t)M);
  for (int r = 0; r < M; ++r) {
    if (labels_host[r] != ETD_IGNORE_LABEL && (labels_host[r] < 0 || labels_host[r] >= V)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_ce: label %d out of range at row %d", labels_host[r], r);
    h[r] = labels_host[r];
  }
  hipStream_t st = (hipStream_t)stream;
  DevPool pl;
  int* di = nullptr;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(st); pl.free_all(); return rc; };
  ETD_TRY_OR(fail, tap_upload(pl, h, &di, st));
  launch_tce(logits_dev, M, V, di, scale, row_loss_dev, st);
  ETD_TRY_OR(fail, ETD_HIP_RC(hipGetLastError()));
  return fail(ETD_HIP_RC(hipStreamSynchronize(st)));
}

extern "C" int etd_debug_dtrain_colred(int mode, const float* dy_dev, int ld, int M, int N, const float* x_dev, const float* mean_dev, const float* rstd_dev,
                                       float* g0_dev, float* g1_dev, void* stream) {
  if (mode != 0 && mode != 1) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_colred: unknown mode %d", mode);
  if (!dy_dev || !g0_dev || (mode == 1 && (!x_dev || !mean_dev || !rstd_dev || !g1_dev))) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_colred: null argument");
  if (M < 1 || M > TAP_MAX_ROWS || N < 1 || ld < N) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_colred: bad shape M=%d N=%d ld=%d", M, N, ld);
  launch_tcolred(mode, dy_dev, ld, M, N, x_dev, mean_dev, rstd_dev, g0_dev, g1_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_embed_grad(const float* src_dev, int ld, int col0, int width, int M, const int32_t* idx_host, int n_rows, int pad_row,
                                           float* grad_dev, void* stream) {
  if (!src_dev || !idx_host || !grad_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed_grad: null argument");
  if (M < 1 || M > TAP_MAX_ROWS || n_rows < 1 || n_rows > TAP_MAX_ROWS || width < 1 || width > (1 << 20) || col0 < 0 || (long long)col0 + width > ld || pad_row < 0 || pad_row >= n_rows)
    ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed_grad: bad shape M=%d rows=%d width=%d col0=%d ld=%d pad=%d", M, n_rows, width, col0, ld, pad_row);
  for (int r = 0; r < M; ++r)
    if (idx_host[r] < 0 || idx_host[r] >= n_rows) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_embed_grad: index %d out of range [0, %d) at row %d", idx_host[r], n_rows, r);
  std::vector<int> h((size_t)M + 3 * (size_t)n_rows, 0);      // order | segment id, start, count
  int* h_seg = h.data() + M;
  const int n_seg = group_rows(idx_host, M, n_rows, pad_row, h.data(), h_seg, h_seg + n_rows, h_seg + 2 * (size_t)n_rows);
  hipStream_t st = (hipStream_t)stream;
  DevPool pl;
  int* di = nullptr;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(st); pl.free_all(); return rc; };
  ETD_TRY_OR(fail, tap_upload(pl, h, &di, st));
  const int* seg = di + M;
  launch_tembed_grad(src_dev, ld, col0, width, di, seg, seg + n_rows, seg + 2 * (size_t)n_rows, n_seg, grad_dev, st);
  ETD_TRY_OR(fail, ETD_HIP_RC(hipGetLastError()));
  return fail(ETD_HIP_RC(hipStreamSynchronize(st)));
}

extern "C" int etd_debug_dtrain_adamw(float* p_dev, float* g_dev, float* m_dev, float* v_dev, long long n, double max_norm, double norm, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, long long step, void* stream) {
  if (!p_dev || !g_dev || !m_dev || !v_dev || n < 1 || n > TAP_MAX_ELEMS) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_adamw: null buffer or n=%lld outside 1 .. 2^36", n);
  if (step < 1 || !(norm >= 0.0)) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_adamw: step %lld (1-based) or norm %g", step, norm);
  ETD_TRY(adamw_check("etd_debug_dtrain_adamw", lr, beta1, beta2, eps, weight_decay));
  launch_tadamw(p_dev, g_dev, m_dev, v_dev, n, adamw_args(max_norm, norm, lr, beta1, beta2, eps, weight_decay, step), (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

extern "C" int etd_debug_dtrain_sumsq(const float* g_dev, long long n, double* norm, void* stream) {
  if (!g_dev || !norm || n < 1 || n > TAP_MAX_ELEMS) ETD_FAIL(ETD_EINVAL, "etd_debug_dtrain_sumsq: null argument or n=%lld outside 1 .. 2^36", n);
  hipStream_t st = (hipStream_t)stream;
  DevPool pl;
  double* partial = nullptr;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(st); pl.free_all(); return rc; };
  ETD_TRY_OR(fail, pl.alloc(&partial, (size_t)TN_BLOCKS));
  return fail(grad_norm(g_dev, n, partial, st, norm));
}
