// C-ABI glue for the Decode stage: EtudeDecoder weights -> device layout, per-stream KV cache and
// generation state kept on the device, prefill / decode-step launch sequences.
// Reference: etude/models/etude_decoder.py:148-206 (forward), :291-343 (token loop);
// etude/utils/model_loader.py:12-60 (checkpoint contract).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/etude_hip_debug.h"
#include "dec_kernels.h"
#include "gemm3.h"
#include "ext_kernels.h"
#include "dec_score.h"
#include "prof.h"

namespace {

// fp32 -> the decoder's 16-bit operand type (dec_kernels.h: IEEE half by default, bf16 under -DETD_DEC_BF16), round to nearest even
inline uint16_t f2bf_h(float f) { return ETD_DEC_IS_F16 ? f32_to_f16_bits(f) : f32_to_bf16_bits(f); }

struct Lin { void* W = nullptr; float* b = nullptr; int N = 0, Npad = 0, K = 0;
             void* Wf = nullptr;      // d16 weights: a second copy in MFMA-fragment order for k_linear (the batched prefill); W stays row-major for the step kernels
             G3Lin g3; };             // fp32 weights: again as hi / lo f16 planes for k_gemm3 (csrc/gemm3.h; W stays fp32 for the weight-streaming kernels below 513 rows); b = g3.b
struct Layer { float *ln1g, *ln1b, *ln2g, *ln2b; Lin qkv, dense, up, down;
               void* dense_hw = nullptr;   // d16 [heads][H][64]: attention.dense regrouped per head for k_dstep_attn_down
               Lin cat;      // decode step: [dense_4h_to_h | attention.dense] along K, so mlp + attn come out of ONE GEMM
               void* mlp_frag = nullptr;   // batched prefill: up | (down | dense) as k_dmlp_fused's weight stream (H 512, I 2048)
               // fp32 mode on the f16 matrix cores: log2 of the plane scales of the attention operands, from provable bounds (etd_decoder_create; the GEMM inputs': g3.x_log2)
               int q_log2 = 0, k_log2 = 0, v_log2 = 0; };

}  // namespace

#define ETD_STAMP_WORDS (ETD_STAMP_HDR + 2 * ETD_STAMP_LOGCAP)      // u64 words of the device-side span accumulator + launch log of the attention launches (layout: dec_kernels.h)
struct etd_dec {
  etd_dec_cfg cfg;
  DevPool pool;                                  // (its byte counts: etd_debug_decoder_checksum)
  bool bf16w = false;
  int H, I, V, L, nh, S, ctx, Mmax, Mcap, out_cap;
  float *word = nullptr, *cls_emb = nullptr, *attr_tab = nullptr;
  std::vector<Layer> layers;
  float *lnfg = nullptr, *lnfb = nullptr;
  Lin head;
  float *X1f = nullptr, *X2f = nullptr;          // fp32 mode, >= G3_MIN_ROWS rows: the two LayerNorm branches as fp32 rows
  float *t_q = nullptr, *t_ao = nullptr, *t_do = nullptr, *t_m1 = nullptr;   // fp32 mode: the last layer's tail on the prompts' last rows only ([S][H], [S][I])
  void* head_frag = nullptr;                     // lm_head in MFMA-fragment order for k_dstep_head: [tile][k-step][lane][8] (d16 weights, H == 512)
  float *rope_cos = nullptr, *rope_sin = nullptr;
  void *Kc = nullptr, *Vc = nullptr;             // [layer][slot][head][ctx][64]
  long long slot_stride = 0, layer_stride = 0;   // elements
  // workspaces
  float *h = nullptr, *h2 = nullptr, *Q = nullptr, *AO = nullptr, *DO = nullptr, *M1 = nullptr, *logits = nullptr;
  int *row_slot = nullptr, *row_pos = nullptr, *row_active = nullptr, *row_sp = nullptr, *ids = nullptr, *slots_dev = nullptr;
  // stream state
  int *cur_tok = nullptr, *len = nullptr, *done = nullptr, *n_out = nullptr, *eos = nullptr, *limit = nullptr, *tgt_attrs = nullptr, *out_tok = nullptr;
  float* tgt_proj = nullptr;                     // [slot][H]: attribute projection of the slot's target attributes (k_slot_proj)
  std::vector<int> last_slots;                   // host copy of what slots_dev holds
  float* qkv_raw = nullptr;                      // [3H] scratch row of the M == 1 QKV path
  d16 *X1b = nullptr, *X2b = nullptr, *AOb = nullptr, *M1b = nullptr;   // d16 activations of the d16 pipeline (M > 1)
  d16* Qb = nullptr;                            // batched prefill: RoPE'd queries [M][H] of the MFMA attention (k_pattn reads K / V from the cache)
  float* hlast = nullptr;                        // [S][H] gathered last rows of a batched prefill
  DSampleCfg* samp_dev = nullptr;                // sampling parameters (device-resident: captured graphs follow set_sampling)
  unsigned long long* rng_key = nullptr;         // [S] per-stream draw keys
  std::vector<unsigned long long> host_key; bool keys_dirty = true; bool sampling = false;
  float* Pk = nullptr;                           // [5][512][H] split-K partials of the decode-step (down | dense) projection
  // diagnostic (etd_debug_decoder_trace_*): per-row hashes of every decode-step kernel's outputs, one record per step
  unsigned* trace = nullptr; int* trace_step = nullptr; int trace_cap = 0; float* trace_pk = nullptr; float* trace_q = nullptr; float* trace_dbg = nullptr;   // trace_pk: layer 0's slabs of the LAST traced step
  int* row_cnt = nullptr;                        // [L][512] arrival counters of the in-launch row finish (DRowFin); zero between launches
  d16* Xcat = nullptr;                          // [512][I + H] d16: GELU(up) | attention output, the K-concatenated input of that GEMM
  std::vector<int> stage;                        // host staging of a prefill batch (fallback when the pinned buffer is absent)
  // pinned host memory (hipHostMalloc): copies to / from it are true async DMAs -- a pageable source or destination costs a
  // staging pass and ~100 us per call at these sizes, all of it with this engine's queue empty (bar boundaries)
  int* pin_stage = nullptr; size_t pin_stage_ints = 0; hipEvent_t pin_stage_evt = nullptr;   // prefill upload; the event = "the last upload has left the buffer"
  int* pin_rb = nullptr;                         // read-back: [done S][n_out S][tokens S * out_cap]
  std::vector<int> host_n_out; bool host_n_out_valid = false;   // n_out as of the last poll; valid until the next step / begin_bars
  std::map<int, hipGraphExec_t> graphs;          // captured decode step per (n_active, paired rows, rows_identity): key 4 * n_active + 2 * pair + identity
  bool rows_identity = false;                    // the step's slot list is 0, 1, ..., n_active - 1
  std::vector<int> host_len;                     // host-side estimate of each slot's KV length (profiler byte counts only)
  double attn_bytes_hint = 0;
  bool step_pair = false;                        // this call's decode steps pair the rows of a head in the attention launch (etd_decoder_step decides)
  // counters of the decode steps issued on this handle since the last etd_decoder_stats_reset (host-side, exact: etd_decoder_stats)
  double stat_steps = 0, stat_row_steps = 0, stat_kv_bytes = 0, stat_attn_launches = 0, stat_stamp_bytes = 0;
  int force_pair = -1;                           // test hook (etd_debug_decoder_force_pair): -1 = the rule above, 0 / 1 = one-row / paired-rows attention form
  unsigned long long* stamp_dev = nullptr;       // device-side span accumulator of k_dstep_attn_down (etd_decoder_stamp); its own allocation
  bool stamp_on = false, stamp_armed = false; long long stamp_skip = 0;      // armed: requested; on: this call's steps are stamped (after `stamp_skip` more steps)
  int bar_logit_rows = 0;                        // test hook (etd_debug_decoder_bar_logits): rows of d->logits the latest begin_bars left
  float* logits_dbg = nullptr; bool logits_dbg_on = false, last_step_fused = false;   // test hook: the fused step's logits [S][V] (etd_debug_decoder_step_logits)
  // teacher-forced scoring (etd_decoder_score): own buffers, allocated by the first score call and freed with the handle (the generate path never touches them).
  // sc_i = [labels Mcap][row list Mcap + score_hb][seq row0 S][seq len S] (uploaded per chunk) then [argmax Mcap][seq tokens S][seq hits S];
  // sc_f = [lp Mcap][lse Mcap]; sc_d = [seq log-likelihood S]; sc_x = [score_hb][H] gathered hidden rows of one head block
  int* sc_i = nullptr; float* sc_f = nullptr; double* sc_d = nullptr; float* sc_x = nullptr; int score_hb = 0;
  // weight sharing (etd_decoder_clone): a clone reads the owner's weight buffers and has its own KV cache, workspaces and
  // stream state.  `pool` of an owner = weights first (n_weight_allocs of them), then its workspaces; a clone's = workspaces only.
  etd_debug_dec_taps taps = {}; bool taps_on = false;      // test hook (etd_debug_decoder_stage_taps): device destinations of the 16-bit sequences' stage outputs
  etd_dec* weights_owner = nullptr;              // null: this handle owns its weights
  size_t n_weight_allocs = 0;
  int n_clones = 0; bool zombie = false;         // owner destroyed while clones are alive: weights freed with the last clone
};

namespace {

// weight [N][K] (+ bias [N] or null) -> device, rows padded with zeros to a multiple of 128
int load_lin(etd_dec* d, const WeightTable& L, const std::string& pfx, int N, int K, bool has_bias, Lin* w) {
  const float* W = L.get(pfx + ".weight", (int64_t)N * K);
  if (!W) return ETD_EINVAL;
  const float* b = nullptr;
  if (has_bias) { b = L.get(pfx + ".bias", N); if (!b) return ETD_EINVAL; }
  const int Npad = ((N + 127) / 128) * 128;
  w->N = N; w->Npad = Npad; w->K = K;
  DevPool& P = d->pool;
  if (d->bf16w) {
    std::vector<uint16_t> hb((size_t)Npad * K, 0);
    for (size_t i = 0; i < (size_t)N * K; ++i) hb[i] = f2bf_h(W[i]);
    uint16_t* p; ETD_TRY(P.upload(&p, hb.data(), hb.size()));
    w->W = p;
    if (K % 16 == 0) {
      std::vector<uint16_t> hp(hb.size());
      pack_wfrag_host(hb.data(), Npad, K, hp.data());
      uint16_t* pf; ETD_TRY(P.upload(&pf, hp.data(), hp.size()));
      w->Wf = pf;
    }
  } else {
    std::vector<float> hf((size_t)Npad * K, 0.f);
    memcpy(hf.data(), W, (size_t)N * K * 4);
    float* p; ETD_TRY(P.upload(&p, hf.data(), hf.size()));
    w->W = p;
    if (K % 32 == 0) {
      ETD_TRY(g3_lin_upload(P, W, b, N, K, 0.f, &w->g3));      // planes, then the padded bias; g3.x_log2: set by etd_decoder_create once the layer's bounds are known
      w->b = w->g3.b;
      return ETD_OK;
    }
  }
  std::vector<float> hb2(Npad, 0.f);
  if (b) memcpy(hb2.data(), b, (size_t)N * 4);
  return P.upload(&w->b, hb2.data(), hb2.size());
}

int load_vec(etd_dec* d, const WeightTable& L, const std::string& name, int n, float** dst) {
  const float* p = L.get(name, n);
  if (!p) return ETD_EINVAL;
  return d->pool.upload(dst, p, n);
}

// ---- one forward pass over M rows.  `rows` describes each row (slot, position, active); the embeddings are in d->h.  One function per kernel sequence
// below (forward_x3 / _plain / _skinny16 / _prefill16); forward_rows picks one per call and returns (in *hfinal) the buffer that holds the last layer's output.
struct PrefillInfo { int n; const int* seq_row0; const int* seq_len; int max_len; double attn_flops; };
// ---- step trace (diagnostic): hash of every row of a buffer -> trace[step % cap][off + slab * M + row]
__global__ __launch_bounds__(64) void k_trace_rows(const unsigned* buf, long long row_stride, int words, long long slab_stride, int M,
                                                   unsigned* trace, const int* step, int cap, long long wps, int off) {
  const int row = blockIdx.x, slab = blockIdx.y, lane = threadIdx.x;
  const unsigned* p = buf + (long long)slab * slab_stride + (long long)row * row_stride;
  unsigned acc = 0;
  for (int i = lane; i < words; i += 64) acc += p[i] * (2654435761u * (unsigned)(i + 1) | 1u);
  for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) trace[(long long)(*step % cap) * wps + off + slab * M + row] = acc;
}
// K / V cache of (row, head) as the step's attention will read it: hash of the row appended by this step, and of rows 0 .. pos
__global__ __launch_bounds__(64) void k_trace_kv(const unsigned* Kc, const unsigned* Vc, long long slot_stride_w, int max_ctx, const int* row_slot, const int* row_pos, int M,
                                                 unsigned* trace, const int* step, int cap, long long wps, int off) {
  const int row = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;
  const int slot = row_slot[row], pos = row_pos[row] < max_ctx ? row_pos[row] : max_ctx - 1;
  unsigned* out = trace + (long long)(*step % cap) * wps + off;
  for (int which = 0; which < 2; ++which) {
    const unsigned* base = (which ? Vc : Kc) + (long long)slot * slot_stride_w + (long long)head * max_ctx * 32;      // 64 d16 = 32 words per position
    unsigned a_new = 0, a_all = 0;
    for (long long i = lane; i < (long long)(pos + 1) * 32; i += 64) {
      const unsigned w = base[i] * (2654435761u * (unsigned)(i + 1) | 1u);
      a_all += w;
      if (i >= (long long)pos * 32) a_new += w;
    }
    for (int o = 32; o; o >>= 1) { a_new += __shfl_xor(a_new, o); a_all += __shfl_xor(a_all, o); }
    if (lane == 0) { out[(which * 8 + head) * M + row] = a_new; out[(16 + which * 8 + head) * M + row] = a_all; }
  }
}
__global__ void k_trace_next(int* step) { *step += 1; }
#define ETD_TRACE_LAYER 49     // records per row and layer: Q, gelu(up), 12 slabs, h_out, ln1, ln2, then per head K[pos], V[pos], K[0..pos], V[0..pos]
static inline long long trace_wps(const etd_dec* d, int M) { return (long long)(ETD_TRACE_LAYER * d->L + 2) * M; }
static int trace_rows(etd_dec* d, const void* buf, long long row_stride, int words, int nslab, long long slab_stride, int M, int off, hipStream_t st) {
  hipLaunchKernelGGL(k_trace_rows, dim3(M, nslab), dim3(64), 0, st, (const unsigned*)buf, row_stride, words, slab_stride, M, d->trace, d->trace_step,
                     d->trace_cap, trace_wps(d, M), off);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ---- stage taps (etd_debug_decoder_stage_taps): every copy below follows the launch that produced its source, on the same stream.  With taps off
// tap_slice is -1 and nothing is enqueued.
// slice of layer l in the caller's buffers, -1 when the layer is not tapped; tail: the slice behind the layers', the last-rows tail of a batched prefill
static inline int tap_slice(const etd_dec* d, int l, bool tail = false) {
  if (!d->taps_on || !((d->taps.layer_mask >> l) & 1u)) return -1;
  return tail ? __builtin_popcount(d->taps.layer_mask) : __builtin_popcount(d->taps.layer_mask & ((1u << l) - 1u));
}
static int tap_copy(void* dst, int slice, size_t slice_bytes, const void* src, size_t bytes, hipStream_t st) {
  if (slice < 0 || !dst) return ETD_OK;
  HIP_TRY(hipMemcpyAsync((char*)dst + (size_t)slice * slice_bytes, src, bytes, hipMemcpyDeviceToDevice, st));
  return ETD_OK;
}
// M rows of `width` elements of `esz` bytes into slice `s` of a [slices][taps.rows][width] buffer
static int tap_rows(const etd_dec* d, void* dst, int s, const void* src, int M, int width, int esz, hipStream_t st) {
  return tap_copy(dst, s, (size_t)d->taps.rows * width * esz, src, (size_t)M * width * esz, st);
}
static int tap_layer_in(const etd_dec* d, int s, const float* hin, int M, hipStream_t st) {      // residual stream and LayerNorm rows entering a layer
  if (s < 0) return ETD_OK;
  ETD_TRY(tap_rows(d, d->taps.hin, s, hin, M, d->H, 4, st));
  ETD_TRY(tap_rows(d, d->taps.ln1, s, d->X1b, M, d->H, 2, st));
  return tap_rows(d, d->taps.ln2, s, d->X2b, M, d->H, 2, st);
}
static int tap_xcat(const etd_dec* d, int s, int M, hipStream_t st) { return tap_rows(d, d->taps.xcat, s, d->Xcat, M, d->I + d->H, 2, st); }
static int tap_slabs(const etd_dec* d, int s, int nslab, int M, hipStream_t st) {
  return tap_copy(d->taps.slabs, s, (size_t)d->taps.slab_cap * d->taps.rows * d->H * 4, d->Pk, (size_t)nslab * M * d->H * 4, st);
}
// the caller's stated sizes against a call of M rows whose split-K launches write nslab slabs: checked before the call launches anything
static int taps_fit(const etd_dec* d, int M, int nslab, bool tail = false /* the call may run the last-rows tail of a batched prefill */) {
  if (!d->taps_on) return ETD_OK;
  const int need = __builtin_popcount(d->taps.layer_mask) + (tail && ((d->taps.layer_mask >> (d->L - 1)) & 1u) ? 1 : 0);
  if (need > d->taps.slices) ETD_FAIL(ETD_EINVAL, "stage taps: the call writes %d slices, the tap buffers hold %d", need, d->taps.slices);
  if (M > d->taps.rows) ETD_FAIL(ETD_EINVAL, "stage taps: a call of %d rows, the tap buffers hold %d", M, d->taps.rows);
  if (d->taps.slabs && (long long)nslab * M > (long long)d->taps.slab_cap * d->taps.rows) ETD_FAIL(ETD_EINVAL, "stage taps: %d slabs of %d rows exceed slab_cap %d x rows %d", nslab, M, d->taps.slab_cap, d->taps.rows);
  return ETD_OK;
}

static inline bool fused_pmlp_on() { const char* e = getenv("ETD_FUSED_PMLP"); return !e || atoi(e) > 0; }
// "Only each prompt's last position is needed" (begin_bars): the last layer then runs its attention, MLP and residual for
// those n rows only -- on the decode-step kernels -- after the big QKV GEMM has put every position's K/V into the cache.
struct LastOnly { int n; const int* idx; DecRows rows; };
constexpr int DS_K_SPLITS = 5;      // the (down | dense) GEMM of the skinny sequence and of the last-rows tail splits K over this many workgroups, each over a multiple of 64 * 8 columns
static inline bool ksplit_fits(const etd_dec* d) { return (d->I + d->H) % (DS_K_SPLITS * 64 * 8) == 0; }
// ... and the fused step kernels (k_dstep_qkv_up, k_dstep_head) are built for hidden 512: the shape test of the fused decode step and of the last-rows tail
static inline bool step_shape(const etd_dec* d) { return ksplit_fits(d) && d->H == 512; }
#ifdef ETD_EXPERIMENTS
static inline bool rowfin_on() { static const bool on = getenv("ETD_ROWFIN") && atoi(getenv("ETD_ROWFIN")) > 0; return on; }     // the in-launch row finish (skinny_attn_down): read once per process
#else
static inline bool rowfin_on() { return false; }          // (measured dead end: built with -DETD_EXPERIMENTS only)
#endif

// ---- argument builders: what every launch of a kind shares; the call sites add the fields of their epilogue
// Y = epi(X W^T + b) over M rows of X.  fp32 weights: W = the fp32 rows of the weight-streaming kernels, Wp = the planes of k_gemm3; 16-bit: W row-major, Wf in fragment order
static DGemmArgs lin_args(const Lin& w, const float* X, int ldx, int M) {
  DGemmArgs a = {};
  a.X = X; a.ldx = ldx; a.M = M; a.W = w.W; a.Wf = w.Wf; a.bias = w.b; a.N = w.N; a.Npad = w.Npad; a.K = w.K; a.Wp = w.g3.Wp; a.w_log2 = w.g3.w_log2; a.x_log2 = w.g3.x_log2;
  return a;
}
static inline void* kv_layer(const etd_dec* d, void* cache, int l) { return (char*)cache + (size_t)l * d->layer_stride * (d->bf16w ? 2 : 4); }
static DGemmArgs qkv_args(const etd_dec* d, int l, const float* X, const DecRows& rows, int M) {      // fused QKV of layer l + RoPE + KV append
  DGemmArgs q = lin_args(d->layers[l].qkv, X, d->H, M);
  q.rows = rows; q.rope_cos = d->rope_cos; q.rope_sin = d->rope_sin; q.rot_half = 8; q.Q = d->Q;
  q.Kc = kv_layer(d, d->Kc, l); q.Vc = kv_layer(d, d->Vc, l); q.slot_stride = d->slot_stride; q.max_ctx = d->ctx; q.n_heads = d->nh;
  return q;
}
static DAttnArgs attn_args(const etd_dec* d, int l, const DecRows& rows, int M) {      // causal attention of `rows` against layer l's KV cache
  DAttnArgs at = {};
  at.Q = d->Q; at.Kc = kv_layer(d, d->Kc, l); at.Vc = kv_layer(d, d->Vc, l); at.slot_stride = d->slot_stride; at.max_ctx = d->ctx; at.n_heads = d->nh;
  at.rows = rows; at.M = M; at.scale = 0.125f; at.bytes_hint = d->attn_bytes_hint;
  return at;
}
static inline void attn_step_pairs(const etd_dec* d, DAttnArgs* at) { at->row_sp = d->row_sp; at->identity = d->rows_identity ? 1 : 0; }     // decode step: the step's (slot, pos) pairs
static inline void attn_stamp(const etd_dec* d, int l, DAttnArgs* at) { at->stamp = d->stamp_on ? d->stamp_dev : nullptr; at->stamp_par = l & 1; }
// LayerNorm parameters and destinations of layer l + 1 (the last kernel of a 16-bit layer also writes the next layer's LayerNorm rows), or nulls after the last layer
struct NextLn { const float *g1, *b1, *g2, *b2; d16 *x1, *x2; };
static NextLn next_ln(const etd_dec* d, int l) {
  const Layer* nx = l + 1 < d->L ? &d->layers[l + 1] : nullptr;
  return nx ? NextLn{nx->ln1g, nx->ln1b, nx->ln2g, nx->ln2b, d->X1b, d->X2b} : NextLn{};
}
// ---- launches that several 16-bit sequences share
static int ln_rows16(etd_dec* d, int l, const float* h, int M, hipStream_t st) {
  const Layer& w = d->layers[l];      // both LayerNorms of layer l -> X1b / X2b
  return launch_ln_rows(h, M, d->H, w.ln1g, w.ln1b, w.ln2g, w.ln2b, d->cfg.layer_norm_eps, d->X1b, d->X2b, st);
}
// k_dattn per (row, head): fp32 rows to AO, 16-bit rows to Ob (row stride ldob, 0 = hidden; null: none)
static int layer_dattn(etd_dec* d, int l, const DecRows& rows, int M, d16* Ob, int ldob, hipStream_t st) {
  DAttnArgs at = attn_args(d, l, rows, M); at.O = d->AO; at.Ob = Ob; at.ldob = ldob;
  if (rows.slot == d->row_slot) { attn_step_pairs(d, &at); attn_stamp(d, l, &at); }
  return launch_dattn(at, d->bf16w, st);
}
// QKV (+RoPE, KV append) and MLP up (+GELU -> Xcat) of the LayerNorm rows in X1b / X2b share one launch
static int step_qkv_up(etd_dec* d, int l, const float* X, const DecRows& rows, int M, hipStream_t st) {
  DGemmArgs q = qkv_args(d, l, X, rows, M); q.Xb = d->X1b; q.Y = d->qkv_raw; q.ldy = 3 * d->H;
  DGemmArgs up = lin_args(d->layers[l].up, X, d->H, M); up.Xb = d->X2b; up.Y = d->M1; up.Yb = d->Xcat; up.ldy = d->I + d->H;
  return launch_dstep_qkv_up(q, up, st);
}
// the row kernel: hout = sum of nslab split-K slabs + (b2 + bd) + hin, and the next layer's two LayerNorms
static int resid_ln(etd_dec* d, int l, int nslab, const float* hin, float* hout, int M, const NextLn& nx, hipStream_t st) {
  return launch_resid_ln_rows(d->Pk, nslab, d->layers[l].cat.b, nullptr, hin, hout, M, d->H, nx.g1, nx.b1, nx.g2, nx.b2, d->cfg.layer_norm_eps, nx.x1, nx.x2, st);
}
// (down | dense) projection with K split over workgroups, then ONE row kernel: partial sums + bias + residual and the
// next layer's two LayerNorms.  (Folding that row kernel into the GEMM's last-arriving workgroup was measured: the
// serial read of 5 slabs x 32 rows costs 3x the kernel boundary it saves.)
static int down_splitk(etd_dec* d, int l, const float* hin, float* hout, int M, const NextLn& nx, hipStream_t st, int ts = -1 /* tap slice */) {
  DGemmArgs dn = lin_args(d->layers[l].cat, d->M1, d->I + d->H, M); dn.Xb = d->Xcat; dn.hin = hin; dn.hout = hout; dn.k_splits = DS_K_SPLITS; dn.Y = d->Pk; dn.ldy = d->H;
  ETD_TRY(launch_dgemm(dn, DEPI_PARTIAL, true, st));
  ETD_TRY(tap_slabs(d, ts, DS_K_SPLITS, M, st));
  ETD_TRY(resid_ln(d, l, DS_K_SPLITS, hin, hout, M, nx, st));
  return tap_rows(d, d->taps.hout, ts, hout, M, d->H, 4, st);
}
// k_linear's decoder modes: M 16-bit rows X [M][w.K] against w in fragment order; `dec` carries what the epilogue reads
static int linear16(const Lin& w, const d16* X, int M, const DGemmArgs& dec, int epi, hipStream_t st) {
  LinArgs a = {};
  a.X = (const e16*)X; a.ldx = w.K; a.W = (const e16*)w.Wf;     /* (LinArgs carries the extractor's element type; the decoder modes of k_linear read these as d16) */
  a.bias = w.b; a.M = M; a.N = w.N; a.K = w.K; a.vt_block = -1; a.dec = dec;
  return launch_linear_dec(a, epi, st);
}

// ---- fp32 mode, >= G3_MIN_ROWS rows: the layer as LayerNorm rows -> QKV (+RoPE, KV append) -> attention -> dense -> up + GELU -> down + residual with every
// contraction on the f16 matrix cores at fp32 grade (csrc/gemm3.h).  Prefill: ragged causal attention over the prompts straight from the fp32 cache rows the QKV
// epilogue has just written, and the last layer's tail only for each prompt's last position; decode step: k_dattn<float> per (row, head).
static int gemm3_auto(const DGemmArgs& a, int epi, hipStream_t st) { return gemm3_s_takes(a, epi) ? launch_gemm3_s(a, epi, st) : launch_gemm3(a, epi, st); }
// last layer: every position's K / V is in the cache now; attention, MLP and residual are needed for the prompts' last rows only (on the weight-streaming kernels).
// gather rows -> attention -> dense -> up + GELU -> down + residual: hout rows 0 .. n-1 = the prompts' last positions, in prompt order
static int x3_last_rows(etd_dec* d, const LastOnly& lo, const float* hin, float* hout, hipStream_t st) {
  const int n = lo.n, l = d->L - 1, H = d->H; const Layer& w = d->layers[l];
  ETD_TRY(launch_gather_rows(hin, lo.idx, n, H, d->hlast, st)); ETD_TRY(launch_gather_rows(d->Q, lo.idx, n, H, d->t_q, st));
  DAttnArgs at = attn_args(d, l, lo.rows, n); at.Q = d->t_q; at.O = d->t_ao; at.bytes_hint = 0;
  ETD_TRY(launch_dattn(at, false, st));
  DGemmArgs de = lin_args(w.dense, d->t_ao, H, n); de.Y = d->t_do; de.ldy = H;
  ETD_TRY(launch_dgemm(de, DEPI_BIAS, false, st));
  DGemmArgs up = lin_args(w.up, d->hlast, H, n); up.Y = d->t_m1; up.ldy = d->I; up.ln_g = w.ln2g; up.ln_b = w.ln2b; up.ln_eps = d->cfg.layer_norm_eps;
  ETD_TRY(launch_dgemm(up, DEPI_GELU, false, st));
  DGemmArgs dn = lin_args(w.down, d->t_m1, d->I, n); dn.add = d->t_do; dn.hin = d->hlast; dn.hout = hout;
  return launch_dgemm(dn, DEPI_RESID, false, st);
}
// every other layer, after its QKV: attention (prefill: ragged causal attn3; decode step: k_dattn) -> dense -> up + GELU -> down + residual
static int x3_layer_rest(etd_dec* d, int l, const DecRows& rows, int M, const PrefillInfo* pf, const float* hin, float* hout, hipStream_t st) {
  const Layer& w = d->layers[l]; const int H = d->H;
  if (pf) {
    Attn3Args t = {};
    t.Q = d->Q; t.ldq = H; t.K = (const float*)kv_layer(d, d->Kc, l); t.V = (const float*)kv_layer(d, d->Vc, l); t.O = d->AO; t.ldo = H; t.n_seq = pf->n; t.n_heads = d->nh;
    t.seq_row0 = pf->seq_row0; t.seq_len = pf->seq_len; t.row_slot = rows.slot; t.slot_stride = d->slot_stride; t.max_ctx = d->ctx; t.max_len = pf->max_len;
    t.scale = 0.125f; t.q_log2 = w.q_log2; t.k_log2 = w.k_log2; t.v_log2 = w.v_log2; t.flops_hint = pf->attn_flops;
    ETD_TRY(launch_attn3(t, st));
  } else {
    DAttnArgs at = attn_args(d, l, rows, M);
    at.O = d->AO; attn_stamp(d, l, &at);
    if (rows.slot == d->row_slot) attn_step_pairs(d, &at);
    ETD_TRY(launch_dattn(at, false, st));
  }
  DGemmArgs de = lin_args(w.dense, d->AO, H, M); de.Y = d->DO; de.ldy = H;      // (attention output: a convex combination of V rows)
  ETD_TRY(gemm3_auto(de, DEPI_BIAS, st));
  DGemmArgs up = lin_args(w.up, d->X2f, H, M); up.Y = d->M1; up.ldy = d->I;
  ETD_TRY(gemm3_auto(up, DEPI_GELU, st));
  DGemmArgs dn = lin_args(w.down, d->M1, d->I, M); dn.add = d->DO; dn.hin = hin; dn.hout = hout;
  return gemm3_auto(dn, DEPI_RESID, st);
}
static int forward_x3(etd_dec* d, int M, const DecRows& rows, const PrefillInfo* pf, const LastOnly* lo, hipStream_t st, float** hfinal, bool* compact) {
  const bool tail = lo && pf && lo->n >= 1 && lo->n < G3_MIN_ROWS && lo->n <= d->S;
  float* hin = d->h; float* hout = d->h2;
  for (int l = 0; l < d->L; ++l) {
    const Layer& w = d->layers[l];
    ETD_TRY(launch_ln_rows_f32(hin, M, d->H, w.ln1g, w.ln1b, w.ln2g, w.ln2b, d->cfg.layer_norm_eps, d->X1f, d->X2f, st));
    ETD_TRY(gemm3_auto(qkv_args(d, l, d->X1f, rows, M), DEPI_QKV, st));
    ETD_TRY(tail && l == d->L - 1 ? x3_last_rows(d, *lo, hin, hout, st) : x3_layer_rest(d, l, rows, M, pf, hin, hout, st));
    std::swap(hin, hout);
  }
  *hfinal = hin; if (tail) *compact = true;
  return ETD_OK;
}

// ---- plain sequence (fp32 weights below G3_MIN_ROWS rows, one row outside the fused step, 16-bit geometries the two 16-bit sequences below do not take):
// QKV -> attention -> dense -> up + GELU -> down + residual, one launch_dgemm each.  act16 (16-bit weights, M > 1): k_ln_rows first and 16-bit activations between
// the GEMMs; otherwise fp32 activations with the LayerNorms fused into the GEMM prologues (k_dgemm / k_dgemm_s / k_dgemv)
static int forward_plain(etd_dec* d, int M, const DecRows& rows, bool act16, hipStream_t st, float** hfinal) {
  float* hin = d->h; float* hout = d->h2; const float eps = d->cfg.layer_norm_eps;
  for (int l = 0; l < d->L; ++l) {
    const Layer& w = d->layers[l];
    if (act16) ETD_TRY(ln_rows16(d, l, hin, M, st));
    DGemmArgs q = qkv_args(d, l, hin, rows, M); q.Y = d->qkv_raw; q.ldy = 3 * d->H;
    if (act16) q.Xb = d->X1b; else { q.ln_g = w.ln1g; q.ln_b = w.ln1b; q.ln_eps = eps; }
    ETD_TRY(launch_dgemm(q, DEPI_QKV, d->bf16w, st));
    ETD_TRY(layer_dattn(d, l, rows, M, act16 ? d->AOb : nullptr, 0, st));
    DGemmArgs de = lin_args(w.dense, d->AO, d->H, M); de.Y = d->DO; de.ldy = d->H; if (act16) de.Xb = d->AOb;
    ETD_TRY(launch_dgemm(de, DEPI_BIAS, d->bf16w, st));
    DGemmArgs up = lin_args(w.up, hin, d->H, M); up.Y = d->M1; up.ldy = d->I;
    if (act16) { up.Xb = d->X2b; up.Yb = d->M1b; } else { up.ln_g = w.ln2g; up.ln_b = w.ln2b; up.ln_eps = eps; }
    ETD_TRY(launch_dgemm(up, DEPI_GELU, d->bf16w, st));
    DGemmArgs dn = lin_args(w.down, d->M1, d->I, M); dn.add = d->DO; dn.hin = hin; dn.hout = hout; if (act16) dn.Xb = d->M1b;      // parallel residual: h = (mlp + attn) + h   (modeling_gpt_neox.py:272)
    ETD_TRY(launch_dgemm(dn, DEPI_RESID, d->bf16w, st));
    std::swap(hin, hout);
  }
  *hfinal = hin;
  return ETD_OK;
}

// ---- 16-bit skinny sequence (a decode step of any row count, a prefill of <= DS_MAX_ROWS rows): QKV | up in one launch, attention.dense folded into the down projection
// ([W2 | Wd] [gelu(..) ; attn] + (b2 + bd): one GEMM and no fp32 round trip of the dense output) as split-K slabs, then the row kernel.
// Step trace after the QKV | up launch of layer l: Q, GELU(up) and the K / V rows (record layout: ETD_TRACE_LAYER)
static int trace_qkv_up(etd_dec* d, int l, int M, hipStream_t st) {
  if (!d->trace) return ETD_OK;
  ETD_TRY(trace_rows(d, d->Q, d->H, d->H, 1, 0, M, l * ETD_TRACE_LAYER * M, st));
  if (l == 0) HIP_TRY(hipMemcpyAsync(d->trace_q, d->Q, (size_t)M * d->H * 4, hipMemcpyDeviceToDevice, st));
  ETD_TRY(trace_rows(d, d->Xcat, (d->I + d->H) / 2, d->I / 2, 1, 0, M, l * ETD_TRACE_LAYER * M + M, st));
  if (d->nh == 8) {
    hipLaunchKernelGGL(k_trace_kv, dim3(M, 8), dim3(64), 0, st, (const unsigned*)kv_layer(d, d->Kc, l), (const unsigned*)kv_layer(d, d->Vc, l), d->slot_stride / 2, d->ctx,
                       d->row_slot, d->row_pos, M, d->trace, d->trace_step, d->trace_cap, trace_wps(d, M), l * ETD_TRACE_LAYER * M + 17 * M);
    HIP_TRY(hipGetLastError());
  }
  return ETD_OK;
}
// decode step: attention (+ its share of attention.dense) and the MLP down projection in ONE launch, then the row kernel
static int skinny_attn_down(etd_dec* d, int l, const DecRows& rows, int M, const float* hin, float* hout, hipStream_t st, int ts) {
  const Layer& w = d->layers[l]; const NextLn nx = next_ln(d, l);
  const int ksd = d->I / 512;      // slabs of the down projection; one more per head from the attention workgroups
  DAttnArgs at = attn_args(d, l, rows, M);
  attn_step_pairs(d, &at); attn_stamp(d, l, &at); at.pair = d->step_pair ? 1 : 0;
  at.dense_w = (const d16*)w.dense_hw; at.dense_out = d->Pk + (size_t)ksd * M * d->H; at.dbg = (d->trace && l == 0) ? d->trace_dbg : nullptr;
  DGemmArgs dn = lin_args(w.cat, nullptr, d->I + d->H, M); dn.Xb = d->Xcat; dn.k_splits = ksd; dn.Y = d->Pk; dn.ldy = d->H;
  // ETD_ROWFIN=1: the row kernel (split-K sum + bias + residual + next LayerNorms) rides in the attention launch -- the last
  // contributor of a row finishes it (DRowFin; 17 launches per step instead of 25, bit-identical results).  Measured round 2
  // ((history: 4ac2f57) tools/runs/r2_run21/24/27.sh): a step of one engine 0.197 -> 0.185 ms, four engines stepping 9.9 -> 10.1 engine-steps/ms,
  // but the JOB 569-575 -> 567 audio-s/s (the attention workgroups live 19 instead of 15.5 us and hold 128 registers per
  // wave while the other engines' prefill GEMMs want the same CUs).  Off by default.
  if (rowfin_on() && ksd + d->nh == 12 && M <= DS_STEP_MAX_ROWS) {
    DRowFin fin = {};
    fin.cnt = d->row_cnt + (size_t)l * DS_STEP_MAX_ROWS; fin.target = d->nh + 16 * ksd; fin.P = d->Pk; fin.nslab = 12;
    fin.bias = w.cat.b; fin.hin = hin; fin.hout = hout; fin.eps = d->cfg.layer_norm_eps;
    fin.g1 = nx.g1; fin.b1 = nx.b1; fin.g2 = nx.g2; fin.b2 = nx.b2; fin.x1 = nx.x1; fin.x2 = nx.x2;
    return launch_dstep_attn_down(at, dn, &fin, st);
  }
  ETD_TRY(launch_dstep_attn_down(at, dn, nullptr, st));
  ETD_TRY(tap_xcat(d, ts, M, st));
  ETD_TRY(tap_slabs(d, ts, ksd + d->nh, M, st));
  if (d->trace && ksd + d->nh == 12) ETD_TRY(trace_rows(d, d->Pk, d->H, d->H, 12, (long long)M * d->H, M, l * ETD_TRACE_LAYER * M + 2 * M, st));
  if (d->trace && l == 0 && ksd + d->nh == 12) HIP_TRY(hipMemcpyAsync(d->trace_pk, d->Pk, (size_t)12 * M * d->H * 4, hipMemcpyDeviceToDevice, st));
  ETD_TRY(resid_ln(d, l, ksd + d->nh, hin, hout, M, nx, st));
  ETD_TRY(tap_rows(d, d->taps.hout, ts, hout, M, d->H, 4, st));
  if (d->trace) {
    ETD_TRY(trace_rows(d, hout, d->H, d->H, 1, 0, M, l * ETD_TRACE_LAYER * M + 14 * M, st));
    if (nx.x1) {
      ETD_TRY(trace_rows(d, d->X1b, d->H / 2, d->H / 2, 1, 0, M, l * ETD_TRACE_LAYER * M + 15 * M, st));
      ETD_TRY(trace_rows(d, d->X2b, d->H / 2, d->H / 2, 1, 0, M, l * ETD_TRACE_LAYER * M + 16 * M, st));
    }
  }
  return ETD_OK;
}
// ln0_done: X1b / X2b already hold layer 0's LayerNorm rows (the fused step: written by the previous step's head kernel)
static int forward_skinny16(etd_dec* d, int M, const DecRows& rows, bool ln0_done, hipStream_t st, float** hfinal) {
  const bool attn_down = rows.slot == d->row_slot && d->H == 512 && d->nh == 8 && d->I % 512 == 0 && d->I / 512 + d->nh <= 12 && d->layers[0].dense_hw &&
                         d->ctx >= 256 && !getenv("ETD_NO_ATTN_DOWN");
  float* hin = d->h; float* hout = d->h2;
  if (!ln0_done) ETD_TRY(ln_rows16(d, 0, hin, M, st));
  for (int l = 0; l < d->L; ++l) {
    const int ts = tap_slice(d, l);
    ETD_TRY(tap_layer_in(d, ts, hin, M, st));
    ETD_TRY(step_qkv_up(d, l, hin, rows, M, st));
    ETD_TRY(tap_rows(d, d->taps.q, ts, d->Q, M, d->H, 4, st));
    ETD_TRY(trace_qkv_up(d, l, M, st));
    if (attn_down) ETD_TRY(skinny_attn_down(d, l, rows, M, hin, hout, st, ts));
    else {
      ETD_TRY(layer_dattn(d, l, rows, M, d->Xcat + d->I, d->I + d->H, st));
      ETD_TRY(tap_xcat(d, ts, M, st));
      ETD_TRY(down_splitk(d, l, hin, hout, M, next_ln(d, l), st, ts));
    }
    std::swap(hin, hout);
  }
  *hfinal = hin;
  return ETD_OK;
}

// ---- 16-bit big prefill sequence (more than DS_MAX_ROWS rows): k_ln_rows -> QKV on the big-tile MFMA GEMM (k_linear decoder modes) or k_pqkv -> ragged MFMA flash
// attention (pf; without it k_dattn per row) -> the fused MLP kernel, or up + GELU and (down | dense) + residual as two k_linear launches
static int prefill16_qkv(etd_dec* d, int l, const float* hin, const DecRows& rows, int M, bool mfma_attn, hipStream_t st) {
  const Layer& w = d->layers[l];
  DGemmArgs q = qkv_args(d, l, hin, rows, M); q.Xb = d->X1b; q.Y = d->qkv_raw; q.ldy = 3 * d->H;
  if (mfma_attn) q.Qb = d->Qb;       // (K / V: the attention reads the cache rows this epilogue writes)
  static const bool pqkv_on = !getenv("ETD_NO_PQKV");
  if (!(mfma_attn && pqkv_on && M >= 49152 && d->H == 512 && d->nh == 8 && w.qkv.N == 1536)) return linear16(w.qkv, d->X1b, M, q, DEPI_QKV, st);
  // QKV with the token block stationary in registers and the weights streamed through LDS (csrc/dec_prefill.hip): 256-token workgroups that walk all 48 weight
  // tiles -- from ~192 workgroups up (below that k_linear's 128 x 256 tiles fill the chip better: 6 466 rows 24 us against 86)
  PQkvArgs pa = {};
  pa.X = d->X1b; pa.ldx = d->H; pa.Wf = (const d16*)w.qkv.Wf; pa.bias = w.qkv.b; pa.M = M; pa.N = w.qkv.N; pa.rows = rows;
  pa.rope_cos = d->rope_cos; pa.rope_sin = d->rope_sin; pa.Qb = d->Qb; pa.Kc = (d16*)q.Kc; pa.Vc = (d16*)q.Vc; pa.slot_stride = d->slot_stride; pa.max_ctx = d->ctx; pa.n_heads = d->nh;
  return launch_pqkv(pa, st);
}
// every other layer, after its QKV: attention into the block of Xcat behind GELU(up), then the MLP with attention.dense folded in, and the residual
static int prefill16_layer_rest(etd_dec* d, int l, const DecRows& rows, int M, const PrefillInfo* pf, bool fmlp, const float* hin, float* hout, hipStream_t st) {
  const Layer& w = d->layers[l]; const int ts = tap_slice(d, l);
  if (pf) {
    // ragged causal MFMA flash attention over the prompts of all streams at once, K / V straight from the cache rows (csrc/dec_prefill.hip)
    PAttnArgs t = {};
    t.Q = d->Qb; t.ldq = d->H; t.Kc = (const d16*)kv_layer(d, d->Kc, l); t.Vc = (const d16*)kv_layer(d, d->Vc, l); t.slot_stride = d->slot_stride; t.max_ctx = d->ctx; t.n_heads = d->nh;
    t.O = d->Xcat + d->I; t.ldo = d->I + d->H; t.seq_row0 = pf->seq_row0; t.seq_len = pf->seq_len; t.row_slot = rows.slot;
    t.n_seq = pf->n; t.max_len = pf->max_len; t.scale_log2e = 0.125f * 1.4426950408889634f; t.flops_hint = pf->attn_flops;
    ETD_TRY(launch_pattn(t, st));
  } else ETD_TRY(layer_dattn(d, l, rows, M, d->Xcat + d->I, d->I + d->H, st));
  if (fmlp) {
    // up + GELU, (down | dense), residual and the next layer's LayerNorms: one launch, the hidden layer never leaves the CU
    const NextLn nx = next_ln(d, l); DMlpArgs ma = {};
    ma.X2 = d->X2b; ma.AO = d->Xcat + d->I; ma.ldao = d->I + d->H; ma.hin = hin; ma.hout = hout; ma.Wm = (const d16*)w.mlp_frag;
    ma.b_up = w.up.b; ma.b_cat = w.cat.b; ma.eps = d->cfg.layer_norm_eps; ma.M = M;
    ma.g1 = nx.g1; ma.b1 = nx.b1; ma.g2 = nx.g2; ma.b2 = nx.b2; ma.nx1 = nx.x1; ma.nx2 = nx.x2;
    ETD_TRY(tap_xcat(d, ts, M, st));
    ETD_TRY(launch_dmlp_fused(ma, st));
    return tap_rows(d, d->taps.hout, ts, hout, M, d->H, 4, st);
  }
  DGemmArgs up = {}; up.Yb = d->Xcat; up.ldy = d->I + d->H;      // (what k_linear's GELU and RESID epilogues read of `dec`)
  ETD_TRY(linear16(w.up, d->X2b, M, up, DEPI_GELU, st));
  ETD_TRY(tap_xcat(d, ts, M, st));
  DGemmArgs dn = {}; dn.N = d->H; dn.hin = hin; dn.hout = hout;
  ETD_TRY(linear16(w.cat, d->Xcat, M, dn, DEPI_RESID, st));
  return tap_rows(d, d->taps.hout, ts, hout, M, d->H, 4, st);
}
// last layer, last positions only: every position's K/V is in the cache now; what remains of the layer is needed for
// n rows, not M (attention, MLP up, (down | dense), residual = 9 % of the prefill's FLOPs at 8 layers) and runs on the skinny sequence's kernels.
// gather rows -> k_ln_rows -> QKV | up -> attention -> split-K (down | dense) -> row kernel: hout rows 0 .. n-1 = the prompts' last positions, in prompt order
static int prefill16_last_rows(etd_dec* d, const LastOnly& lo, const float* hin, float* hout, hipStream_t st) {
  const int n = lo.n, l = d->L - 1, ts = tap_slice(d, l, true);
  ETD_TRY(launch_gather_rows(hin, lo.idx, n, d->H, d->hlast, st));
  ETD_TRY(ln_rows16(d, l, d->hlast, n, st));
  ETD_TRY(tap_layer_in(d, ts, d->hlast, n, st));
  ETD_TRY(step_qkv_up(d, l, d->hlast, lo.rows, n, st));
  ETD_TRY(tap_rows(d, d->taps.q, ts, d->Q, n, d->H, 4, st));
  DAttnArgs at = attn_args(d, l, lo.rows, n); at.O = d->AO; at.Ob = d->Xcat + d->I; at.ldob = d->I + d->H; at.bytes_hint = 0;
  ETD_TRY(launch_dattn(at, d->bf16w, st));
  ETD_TRY(tap_xcat(d, ts, n, st));
  return down_splitk(d, l, d->hlast, hout, n, NextLn{}, st, ts);
}
static int forward_prefill16(etd_dec* d, int M, const DecRows& rows, const PrefillInfo* pf, const LastOnly* lo, hipStream_t st, float** hfinal, bool* compact) {
  // batched prefill on the fused MLP kernel: it also writes the NEXT layer's LayerNorm rows, so only layer 0 needs the row kernel
  // ON by default, ETD_FUSED_PMLP=0 turns it off (read at create time for the packed stream, and per call so that the A/B test can toggle it): measured round 2
  // ((history: 4ac2f57) tools/runs/r2_run47.sh) at 195 us per launch against 166 + 16 us for the launches it replaces, +1.3 % in the job -- csrc/dec_fused.hip
  const bool fmlp = d->layers[0].mlp_frag && d->H == 512 && d->I == 2048 && fused_pmlp_on();
  const bool tail = lo && pf && lo->n > 1 && lo->n <= DS_STEP_MAX_ROWS && step_shape(d) && !getenv("ETD_NO_LAST_ONLY");
  float* hin = d->h; float* hout = d->h2;
  for (int l = 0; l < d->L; ++l) {
    if (l == 0 || !fmlp) ETD_TRY(ln_rows16(d, l, hin, M, st));
    const int ts = tap_slice(d, l);
    ETD_TRY(tap_layer_in(d, ts, hin, M, st));
    ETD_TRY(prefill16_qkv(d, l, hin, rows, M, pf != nullptr, st));
    ETD_TRY(pf ? tap_rows(d, d->taps.qb, ts, d->Qb, M, d->H, 2, st) : tap_rows(d, d->taps.q, ts, d->Q, M, d->H, 4, st));
    ETD_TRY(tail && l == d->L - 1 ? prefill16_last_rows(d, *lo, hin, hout, st) : prefill16_layer_rest(d, l, rows, M, pf, fmlp, hin, hout, st));
    std::swap(hin, hout);
  }
  *hfinal = hin; if (tail) *compact = true;
  return ETD_OK;
}

// ---- picks the sequence, once per call.  *hfinal = the buffer that holds the last layer's output (before the final LayerNorm); lo (with compact): the last layer may run for the prompts' last rows alone, *compact says whether it did
static int forward_rows(etd_dec* d, int M, const DecRows& rows, const PrefillInfo* pf, const LastOnly* lo, hipStream_t st, float** hfinal, bool* compact) {
  if (compact) *compact = false; else lo = nullptr;
  const Layer& w0 = d->layers[0];
  if (!d->bf16w && M >= G3_MIN_ROWS && d->X1f && w0.qkv.g3.Wp && w0.down.g3.Wp) return forward_x3(d, M, rows, pf, lo, st, hfinal, compact);
  const bool act16 = d->bf16w && M > 1;
  if (act16 && M > DS_MAX_ROWS && w0.qkv.Wf && w0.up.Wf && w0.cat.Wf) return forward_prefill16(d, M, rows, pf, lo, st, hfinal, compact);
  if (act16 && ksplit_fits(d)) return forward_skinny16(d, M, rows, false, st, hfinal);
  return forward_plain(d, M, rows, act16, st, hfinal);
}

// final LayerNorm + lm_head for `n` rows of X (fp32 [n][H]) -> logits [n][V]
int head_logits(etd_dec* d, const float* X, int n, float* logits, hipStream_t st) {
  const bool g3 = !d->bf16w && n >= G3_MIN_ROWS && d->X1f && d->head.g3.Wp;
  if (g3) ETD_TRY(launch_ln_rows_f32(X, n, d->H, d->lnfg, d->lnfb, nullptr, nullptr, d->cfg.layer_norm_eps, d->X1f, nullptr, st));
  DGemmArgs lm = lin_args(d->head, g3 ? d->X1f : X, d->H, n);
  lm.bias = nullptr; lm.Y = logits; lm.ldy = d->V;
  if (g3) return launch_gemm3(lm, DEPI_LOGITS, st);
  lm.ln_g = d->lnfg; lm.ln_b = d->lnfb; lm.ln_eps = d->cfg.layer_norm_eps;
  return launch_dgemm(lm, DEPI_LOGITS, d->bf16w, st);
}

int check_slot(etd_dec* d, int slot) {
  if (!d || slot < 0 || slot >= d->S) ETD_FAIL(ETD_EINVAL, "decoder: bad slot %d", slot);
  return ETD_OK;
}

__global__ void k_init_slots(const int* __restrict__ init, int n, int* tgt_attrs, int* cur_tok, int* len, int* done, int* n_out, int* eos, int* limit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int* p = init + i * 7;
  const int s = p[0];
  tgt_attrs[4 * s] = p[1]; tgt_attrs[4 * s + 1] = p[2]; tgt_attrs[4 * s + 2] = p[3]; tgt_attrs[4 * s + 3] = p[4];
  cur_tok[s] = 0; len[s] = 0; done[s] = 0; n_out[s] = 0; eos[s] = p[5]; limit[s] = p[6];
}

// The attribute projection of a slot's TARGET attributes, ((t0 + t1) + t2) + t3 exactly as k_dembed / k_dstep_head add it
// (etude_decoder.py:171-176): fixed for the whole bar, so it is formed once here and every decode step reads one row
// instead of four.
__global__ __launch_bounds__(128) void k_slot_proj(const int* __restrict__ init, const float* __restrict__ attr_tab, int n_bins, int H, float* proj) {
  const int* p = init + blockIdx.x * 7;
  const int s = p[0];
  for (int k = threadIdx.x * 4; k < H; k += 128 * 4) {
    f32x4 t[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) t[a] = *reinterpret_cast<const f32x4*>(attr_tab + (long long)(a * n_bins + p[1 + a]) * H + k);
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = ((t[0][c] + t[1][c]) + t[2][c]) + t[3][c];
    *reinterpret_cast<f32x4*>(proj + (long long)s * H + k) = o;
  }
}

// Stage a batch of n prompts (concatenated) on the device, embed them, run the model.  On return *hfinal holds
// the hidden states of all Mtot rows; the staged row metadata lives in d->ids (layout below).
struct Staged { int Mtot; const int *ids, *cls, *attrs, *row_slot, *row_pos, *row_active, *last_idx, *last_slot, *last_pos, *last_active, *init, *row_seq, *seq_row0, *seq_len; };

int stage_and_forward(etd_dec* d, int n, const int32_t* slots, const int32_t* T, const int32_t* ids, const int32_t* cls,
                      const int32_t* attrs4, const int32_t* init7 /* [n][7] or null */, Staged* sg, float** hfinal, hipStream_t st, bool* last_only = nullptr) {
  if (!d || n < 1 || n > d->S || !slots || !T || !ids || !cls || !attrs4) ETD_FAIL(ETD_EINVAL, "prefill: bad arguments");
  long long Mtot = 0;
  std::vector<char> seen((size_t)d->S, 0);
  for (int i = 0; i < n; ++i) {
    ETD_TRY(check_slot(d, slots[i]));
    if (T[i] <= 0 || T[i] > d->ctx) ETD_FAIL(ETD_EINVAL, "prefill: prompt %d has T=%d (max_ctx=%d)", i, T[i], d->ctx);
    if (seen[slots[i]]) ETD_FAIL(ETD_EINVAL, "prefill: slot %d listed twice", slots[i]);
    seen[slots[i]] = 1;
    Mtot += T[i];
  }
  if (Mtot > d->Mcap) ETD_FAIL(ETD_EINVAL, "prefill: %lld prompt rows exceed max_prefill_rows=%d", Mtot, d->Mcap);
  const int M = (int)Mtot;
  ETD_TRY(taps_fit(d, M, DS_K_SPLITS, n > 1 && M > DS_MAX_ROWS));      // (a superset of forward_prefill16's `tail`)
  for (int i = 0; i < M; ++i) {
    if (ids[i] < 0 || ids[i] >= d->V || cls[i] < 0 || cls[i] >= d->cfg.num_classes) ETD_FAIL(ETD_EINVAL, "prefill: token/class id out of range at row %d", i);
    for (int k = 0; k < 4; ++k) if (attrs4[(size_t)k * M + i] < 0 || attrs4[(size_t)k * M + i] >= d->cfg.num_attribute_bins) ETD_FAIL(ETD_EINVAL, "prefill: attribute bin out of range at row %d", i);
  }
  // staging layout: [ids M][cls M][attrs 4M][row_slot M][row_pos M][row_active M][last_idx n][last_slot n][last_pos n][last_active n][init 7n]
  //                 [row_seq M][seq_row0 n][seq_len n]
  const size_t sv_ints = (size_t)10 * M + 13 * n;
  int* svp;
  const bool pinned = d->pin_stage && sv_ints <= d->pin_stage_ints;
  if (pinned) {
    HIP_TRY(hipEventSynchronize(d->pin_stage_evt));            // the previous upload (if any) has been read out of the buffer
    svp = d->pin_stage;                                         // (every word of the layout is written below: no memset of ~40 bytes per prompt row)
  } else {
    d->stage.resize(sv_ints);
    svp = d->stage.data();
  }
  memcpy(svp, ids, (size_t)M * 4);
  memcpy(svp + M, cls, (size_t)M * 4);
  memcpy(svp + 2 * (size_t)M, attrs4, (size_t)4 * M * 4);
  int* rs = svp + 6 * (size_t)M; int* rp = rs + M; int* ra = rp + M;
  int* li = ra + M; int* ls = li + n; int* lp = ls + n; int* la = lp + n; int* in7 = la + n;
  int* rq = in7 + 7 * n; int* sr0 = rq + M; int* sln = sr0 + n;
  int row = 0, max_len = 0; double kvb = 0, aflops = 0;
  for (int i = 0; i < n; ++i) {
    sr0[i] = row; sln[i] = T[i]; if (T[i] > max_len) max_len = T[i];
    aflops += 0.5 * 256.0 * d->nh * (double)T[i] * T[i];
    for (int t = 0; t < T[i]; ++t, ++row) { rs[row] = slots[i]; rp[row] = t; ra[row] = 1; rq[row] = i; }
    li[i] = row - 1; ls[i] = slots[i]; lp[i] = T[i] - 1; la[i] = 1;
    d->host_len[slots[i]] = T[i];
    kvb += (double)T[i] * d->nh * 64 * (2.0 * (d->bf16w ? 2 : 4) + 4 + 4);   // prefill: Q, K, V read once, O written once (K/V re-reads are L2 hits)
  }
  if (init7) memcpy(in7, init7, (size_t)7 * n * 4); else memset(in7, 0, (size_t)7 * n * 4);
  d->attn_bytes_hint = kvb;
  HIP_TRY(hipMemcpyAsync(d->ids, svp, sv_ints * 4, hipMemcpyHostToDevice, st));   // pinned: an async DMA; pageable fallback: returns after staging
  if (pinned) HIP_TRY(hipEventRecord(d->pin_stage_evt, st));
  d->host_n_out_valid = false;
  const int* b = d->ids;
  *sg = Staged{M, b, b + M, b + 2 * (size_t)M, b + 6 * (size_t)M, b + 7 * (size_t)M, b + 8 * (size_t)M, b + 9 * (size_t)M, b + 9 * (size_t)M + n,
               b + 9 * (size_t)M + 2 * n, b + 9 * (size_t)M + 3 * n, b + 9 * (size_t)M + 4 * n,
               b + 9 * (size_t)M + 11 * n, b + 10 * (size_t)M + 11 * n, b + 10 * (size_t)M + 12 * n};
  if (init7) {
    hipLaunchKernelGGL(k_init_slots, dim3((n + 63) / 64), dim3(64), 0, st, sg->init, n, d->tgt_attrs, d->cur_tok, d->len, d->done, d->n_out, d->eos, d->limit);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_slot_proj, dim3(n), dim3(128), 0, st, sg->init, d->attr_tab, d->cfg.num_attribute_bins, d->H, d->tgt_proj);
    HIP_TRY(hipGetLastError());
  }
  DEmbedArgs e = {};
  e.ids = sg->ids; e.cls = sg->cls; e.attrs = sg->attrs; e.M = M; e.H = d->H; e.n_bins = d->cfg.num_attribute_bins;
  e.word = d->word; e.cls_emb = d->cls_emb; e.attr_tab = d->attr_tab; e.h = d->h;
  e.rows = DecRows{sg->row_slot, sg->row_pos, sg->row_active, sg->row_seq};
  ETD_TRY(launch_dembed(e, st));
  PrefillInfo pf{n, sg->seq_row0, sg->seq_len, max_len, aflops};
  const bool can_mfma_attn = (d->bf16w ? d->Qb != nullptr : d->X1f != nullptr);
  LastOnly lo{n, sg->last_idx, DecRows{sg->last_slot, sg->last_pos, sg->last_active}};
  return forward_rows(d, M, e.rows, can_mfma_attn ? &pf : nullptr, &lo, st, hfinal, last_only);
}

// KV cache, activation workspaces and stream state of one handle (everything that is not a weight)
int alloc_workspaces(etd_dec* d) {
  const int H = d->H;
  DevPool& P = d->pool;
  d->slot_stride = (long long)d->nh * d->ctx * 64;
  d->layer_stride = d->slot_stride * d->S;
  const size_t kv_elems = (size_t)d->layer_stride * d->L;
  if (d->bf16w) { uint16_t *k, *v; ETD_TRY(P.alloc(&k, kv_elems, true)); ETD_TRY(P.alloc(&v, kv_elems, true)); d->Kc = k; d->Vc = v; }
  else { float *k, *v; ETD_TRY(P.alloc(&k, kv_elems, true)); ETD_TRY(P.alloc(&v, kv_elems, true)); d->Kc = k; d->Vc = v; }
  const size_t M = d->Mcap;
  const size_t Mf = d->bf16w ? (size_t)(d->S > 1 ? d->S : 1) : M;     // rows that can take the fp32-activation path
  ETD_TRY(P.alloc(&d->h, M * H)); ETD_TRY(P.alloc(&d->h2, M * H));
  ETD_TRY(P.alloc(&d->Q, M * H)); ETD_TRY(P.alloc(&d->AO, M * H)); ETD_TRY(P.alloc(&d->DO, M * H));
  ETD_TRY(P.alloc(&d->M1, Mf * d->I)); ETD_TRY(P.alloc(&d->logits, (size_t)d->Mmax * d->V));
  ETD_TRY(P.alloc(&d->qkv_raw, (size_t)3 * H)); ETD_TRY(P.alloc(&d->hlast, (size_t)d->S * H));
  if (d->bf16w) {
    ETD_TRY(P.alloc(&d->X1b, M * H)); ETD_TRY(P.alloc(&d->X2b, M * H)); ETD_TRY(P.alloc(&d->AOb, M * H));
    ETD_TRY(P.alloc(&d->M1b, M * d->I));
    ETD_TRY(P.alloc(&d->Pk, (size_t)12 * DS_STEP_MAX_ROWS * H));     // split-K slabs of the decode step: 5 (down | dense) or 4 (down) + one per head (dense inside the attention workgroups)
    ETD_TRY(P.alloc(&d->row_cnt, (size_t)d->L * DS_STEP_MAX_ROWS, true));
    ETD_TRY(P.alloc(&d->Xcat, M * (d->I + H)));
    ETD_TRY(P.alloc(&d->Qb, M * H));      // RoPE'd queries of a batched prefill (K / V: the cache rows)
  }
  if (!d->bf16w) {
    ETD_TRY(P.alloc(&d->X1f, M * H)); ETD_TRY(P.alloc(&d->X2f, M * H));
    const size_t Sr = d->S > 1 ? d->S : 1;
    ETD_TRY(P.alloc(&d->t_q, Sr * H)); ETD_TRY(P.alloc(&d->t_ao, Sr * H)); ETD_TRY(P.alloc(&d->t_do, Sr * H)); ETD_TRY(P.alloc(&d->t_m1, Sr * d->I));
  }
  ETD_TRY(P.alloc(&d->samp_dev, (size_t)1, true)); ETD_TRY(P.alloc(&d->rng_key, (size_t)d->S, true));
  ETD_TRY(P.alloc(&d->row_sp, (size_t)2 * d->Mmax, true));
  ETD_TRY(P.alloc(&d->row_slot, (size_t)d->Mmax)); ETD_TRY(P.alloc(&d->row_pos, (size_t)d->Mmax)); ETD_TRY(P.alloc(&d->row_active, (size_t)d->Mmax));
  ETD_TRY(P.alloc(&d->ids, 10 * M + 13 * (size_t)d->S)); ETD_TRY(P.alloc(&d->slots_dev, (size_t)d->S));
  const size_t S = d->S;
  ETD_TRY(P.alloc(&d->cur_tok, S, true)); ETD_TRY(P.alloc(&d->len, S, true)); ETD_TRY(P.alloc(&d->done, S, true));
  ETD_TRY(P.alloc(&d->n_out, S, true)); ETD_TRY(P.alloc(&d->eos, S, true)); ETD_TRY(P.alloc(&d->limit, S, true));
  ETD_TRY(P.alloc(&d->tgt_proj, S * (size_t)d->H, true));
  ETD_TRY(P.alloc(&d->tgt_attrs, 4 * S, true)); ETD_TRY(P.alloc(&d->out_tok, S * d->out_cap, true));
  d->pin_stage_ints = 10 * M + 13 * S;
  if (hipHostMalloc((void**)&d->pin_stage, d->pin_stage_ints * 4, hipHostMallocDefault) != hipSuccess) { d->pin_stage = nullptr; (void)hipGetLastError(); }
  if (hipHostMalloc((void**)&d->pin_rb, (2 * S + S * (size_t)d->out_cap) * 4, hipHostMallocDefault) != hipSuccess) { d->pin_rb = nullptr; (void)hipGetLastError(); }
  if (d->pin_stage && hipEventCreateWithFlags(&d->pin_stage_evt, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(d->pin_stage); d->pin_stage = nullptr; d->pin_stage_evt = nullptr; }
  d->host_n_out.assign(S, 0);
  return ETD_OK;
}

// a handle that never reached its caller (create / clone failed half way): everything it owns so far
void free_unborn(etd_dec* d) {
  d->pool.free_all();
  if (d->pin_stage) (void)hipHostFree(d->pin_stage);
  if (d->pin_rb) (void)hipHostFree(d->pin_rb);
  if (d->pin_stage_evt) (void)hipEventDestroy(d->pin_stage_evt);
  delete d;
}

// provable bounds of one layer's activations, whatever the input (csrc/gemm3.h): LayerNorm outputs by their parameters, projections of them by Cauchy-Schwarz on the
// weight rows; the rotary embedding mixes two dims of a Q / K row (|x1 c - x2 s| <= |x1| + |x2|: q and k carry the factor 2); |gelu(u)| <= |u|
struct LayerBounds { float ln1, ln2, q, k, v, up; };
int layer_bounds(const WeightTable& L, const std::string& p, int H, int I, LayerBounds* B) {
  const float* g1 = L.get(p + "input_layernorm.weight", H); const float* b1 = L.get(p + "input_layernorm.bias", H);
  const float* g2 = L.get(p + "post_attention_layernorm.weight", H); const float* b2 = L.get(p + "post_attention_layernorm.bias", H);
  const float* Wq = L.get(p + "attention.query_key_value.weight", (int64_t)3 * H * H); const float* bq = L.get(p + "attention.query_key_value.bias", 3 * H);
  const float* Wu = L.get(p + "mlp.dense_h_to_4h.weight", (int64_t)I * H); const float* bu = L.get(p + "mlp.dense_h_to_4h.bias", I);
  if (!g1 || !b1 || !g2 || !b2 || !Wq || !bq || !Wu || !bu) return ETD_EINVAL;
  std::vector<float> rb((size_t)3 * H);
  g3_row_bounds_of_ln(Wq, bq, 3 * H, H, g1, b1, rb.data());
  float bnd[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < 3 * H; ++j) { const int part = (j % 192) >> 6; bnd[part] = fmaxf(bnd[part], rb[j]); }      // GPT-NeoX's [head][q|k|v][64] rows
  *B = LayerBounds{g3_bound_ln(g1, b1, H), g3_bound_ln(g2, b2, H), 2.f * bnd[0], 2.f * bnd[1], bnd[2], g3_bound_linear_of_ln(Wu, bu, I, H, g2, b2)};
  return ETD_OK;
}

}  // namespace

// 1 when the library was built with -DETD_EXPERIMENTS: the measured dead ends (in-launch row finish, 8 / 16-wave attention workgroups) are compiled in and their
// switches (ETD_ROWFIN, ETD_AD_WAVES) are live, as are ETD_LAUNCH_LOG and ETD_NO_GRAPH; the shipped build has one path per precision and ignores those switches
extern "C" int etd_has_experiments(void) {
#ifdef ETD_EXPERIMENTS
  return 1;
#else
  return 0;
#endif
}

extern "C" int etd_decoder_operand_type(void) { return ETD_DEC_IS_F16; }

extern "C" int etd_decoder_create(const etd_dec_cfg* cfg, const char* const* names, const float* const* host_ptrs,
                                  const int64_t* numels, int n, etd_dec** out) {
  if (!cfg || !names || !host_ptrs || !numels || !out) ETD_FAIL(ETD_EINVAL, "decoder_create: null argument");
  if (cfg->struct_bytes != (int)sizeof(etd_dec_cfg)) ETD_FAIL(ETD_EINVAL, "decoder_create: etd_dec_cfg of %d bytes, this library (ABI %d) expects %d -- caller built against another etude_hip.h", cfg->struct_bytes, ETD_ABI_VERSION, (int)sizeof(etd_dec_cfg));
  const etd_dec_cfg& c = *cfg;
  if (c.hidden_size % 256 || c.num_attention_heads <= 0 || c.hidden_size / c.num_attention_heads != 64 || c.intermediate_size % 128 ||
      (int)(64 * c.rotary_pct) != 16 || c.num_hidden_layers < 1 || c.vocab_size < 2 || c.max_streams < 1 || c.max_ctx < 16 ||
      c.attribute_emb_dim < 1 || c.num_attribute_bins < 1)
    ETD_FAIL(ETD_EINVAL, "decoder_create: unsupported config (need head_dim 64, rotary_ndims 16, hidden %% 256 == 0, intermediate %% 128 == 0)");
  etd_dec* d = new etd_dec();
  d->cfg = c; d->bf16w = c.precision == 1;
  d->H = c.hidden_size; d->I = c.intermediate_size; d->V = c.vocab_size; d->L = c.num_hidden_layers; d->nh = c.num_attention_heads;
  d->S = c.max_streams; d->ctx = c.max_ctx; d->out_cap = 1024;
  d->Mmax = d->ctx > d->S ? d->ctx : d->S;
  d->Mcap = c.max_prefill_rows > d->Mmax ? c.max_prefill_rows : d->Mmax;
  d->host_len.assign(d->S, 0);
  d->host_key.resize(d->S);
  for (int i = 0; i < d->S; ++i) d->host_key[i] = (unsigned long long)i;
  const WeightTable Ld(names, host_ptrs, numels, n);
  DevPool& P = d->pool;
  auto fail = [&](int rc) { free_unborn(d); return rc; };
  const int H = d->H, E = c.attribute_emb_dim, NB = c.num_attribute_bins;
  ETD_TRY_OR(fail, load_vec(d, Ld, "word_embeddings.weight", d->V * H, &d->word));
  ETD_TRY_OR(fail, load_vec(d, Ld, "class_embeddings.weight", c.num_classes * H, &d->cls_emb));
  {
    // attribute_projection(cat(e0,e1,e2,e3)) = bias + sum_a W[:, aE:(a+1)E] e_a  -> per (attribute, bin) vectors
    const char* an[4] = {"pitch_overlap_embeddings.weight", "polyphony_embeddings.weight", "note_sustain_embeddings.weight", "rhythm_intensity_embeddings.weight"};
    const float* pw = Ld.get("attribute_projection.weight", (int64_t)H * 4 * E);
    const float* pb = Ld.get("attribute_projection.bias", H);
    if (!pw || !pb) return fail(ETD_EINVAL);
    std::vector<float> tab((size_t)4 * NB * H);
    for (int a = 0; a < 4; ++a) {
      const float* em = Ld.get(an[a], (int64_t)NB * E);
      if (!em) return fail(ETD_EINVAL);
      for (int b = 0; b < NB; ++b)
        for (int o = 0; o < H; ++o) {
          double s = (a == 0) ? (double)pb[o] : 0.0;
          for (int e = 0; e < E; ++e) s += (double)pw[(size_t)o * 4 * E + a * E + e] * em[b * E + e];
          tab[((size_t)a * NB + b) * H + o] = (float)s;
        }
    }
    ETD_TRY_OR(fail, P.upload(&d->attr_tab, tab.data(), tab.size()));
  }
  d->layers.resize(d->L);
  for (int l = 0; l < d->L; ++l) {
    const std::string p = "transformer.layers." + std::to_string(l) + ".";
    Layer& w = d->layers[l];
    ETD_TRY_OR(fail, load_vec(d, Ld, p + "input_layernorm.weight", H, &w.ln1g));
    ETD_TRY_OR(fail, load_vec(d, Ld, p + "input_layernorm.bias", H, &w.ln1b));
    ETD_TRY_OR(fail, load_vec(d, Ld, p + "post_attention_layernorm.weight", H, &w.ln2g));
    ETD_TRY_OR(fail, load_vec(d, Ld, p + "post_attention_layernorm.bias", H, &w.ln2b));
    ETD_TRY_OR(fail, load_lin(d, Ld, p + "attention.query_key_value", 3 * H, H, true, &w.qkv));
    ETD_TRY_OR(fail, load_lin(d, Ld, p + "attention.dense", H, H, true, &w.dense));
    ETD_TRY_OR(fail, load_lin(d, Ld, p + "mlp.dense_h_to_4h", d->I, H, true, &w.up));
    ETD_TRY_OR(fail, load_lin(d, Ld, p + "mlp.dense_4h_to_h", H, d->I, true, &w.down));
    LayerBounds B = {};
    if (!d->bf16w || ETD_DEC_IS_F16) ETD_TRY_OR(fail, layer_bounds(Ld, p, H, d->I, &B));
    if (!d->bf16w) {
      // plane scales of the fp32-grade f16 path (csrc/gemm3.h); the attention output is a convex combination of V rows
      w.qkv.g3.x_log2 = g3_scale_log2(B.ln1); w.up.g3.x_log2 = g3_scale_log2(B.ln2);
      w.q_log2 = g3_scale_log2(B.q); w.k_log2 = g3_scale_log2(B.k); w.v_log2 = g3_scale_log2(B.v);
      w.dense.g3.x_log2 = w.v_log2; w.down.g3.x_log2 = g3_scale_log2(B.up);
    }
#if ETD_DEC_IS_F16
    if (d->bf16w) {
      // The 16-bit mode's operands are IEEE half (dec_kernels.h): unlike bf16 they END at 65 504, and an Inf in a LayerNorm row, a cache row or the hidden layer becomes NaN in
      // the softmax / the next LayerNorm.  Every 16-bit tensor of this path is a weight, a LayerNorm output, a projection of one (Q / K / V after the rotary mix, GELU(up): |gelu(u)| <= |u|)
      // or a convex combination of V rows: the same provable bounds the fp32-grade path takes its plane scales from (csrc/gemm3.h) say at load time whether THIS checkpoint
      // can leave the range, whatever the input.  A checkpoint that could is refused (a -DETD_DEC_BF16 build, or precision "fp32", takes it).
      const float bounds[4] = {B.ln1, B.ln2, fmaxf(B.q, fmaxf(B.k, B.v)), B.up};
      static const char* const what[4] = {"input_layernorm rows", "post_attention_layernorm rows", "Q / K / V rows", "gelu(dense_h_to_4h) rows"};
      for (int i = 0; i < 4; ++i)
        if (!(bounds[i] < 65504.f)) { g_etd_err = "decoder_create: layer " + std::to_string(l) + ": " + what[i] + " can reach " + std::to_string(bounds[i]) +
                                                  " (provable bound), beyond the IEEE-half range of the 16-bit serving mode; use precision \"fp32\" or a -DETD_DEC_BF16 build"; return fail(ETD_EINVAL); }
    }
#endif
    if (d->bf16w) {
      // h_new - h = W2 gelu(..) + b2 + Wd attn + bd  ==  [W2 | Wd] [gelu(..) ; attn] + (b2 + bd)
      const float* W2 = Ld.get(p + "mlp.dense_4h_to_h.weight", (int64_t)H * d->I);
      const float* Wd = Ld.get(p + "attention.dense.weight", (int64_t)H * H);
      const float* b2 = Ld.get(p + "mlp.dense_4h_to_h.bias", H);
      const float* bd = Ld.get(p + "attention.dense.bias", H);
      const int Kc = d->I + H;
      std::vector<uint16_t> wc((size_t)H * Kc);
      for (int o = 0; o < H; ++o) {
        for (int k = 0; k < d->I; ++k) wc[(size_t)o * Kc + k] = f2bf_h(W2[(size_t)o * d->I + k]);
        for (int k = 0; k < H; ++k) wc[(size_t)o * Kc + d->I + k] = f2bf_h(Wd[(size_t)o * H + k]);
      }
      uint16_t* pw; ETD_TRY_OR(fail, P.upload(&pw, wc.data(), wc.size()));
      std::vector<float> bc(H);
      for (int o = 0; o < H; ++o) bc[o] = b2[o] + bd[o];
      w.cat.W = pw; w.cat.N = H; w.cat.Npad = H; w.cat.K = Kc;
      {
        std::vector<uint16_t> dh((size_t)d->nh * H * 64);
        for (int hd = 0; hd < d->nh; ++hd)
          for (int o = 0; o < H; ++o)
            for (int dd = 0; dd < 64; ++dd) dh[((size_t)hd * H + o) * 64 + dd] = f2bf_h(Wd[(size_t)o * H + hd * 64 + dd]);
        uint16_t* pd; ETD_TRY_OR(fail, P.upload(&pd, dh.data(), dh.size()));
        w.dense_hw = pd;
      }
      if (H % 32 == 0 && Kc % 16 == 0) {
        std::vector<uint16_t> wp(wc.size());
        pack_wfrag_host(wc.data(), H, Kc, wp.data());
        uint16_t* pf; ETD_TRY_OR(fail, P.upload(&pf, wp.data(), wp.size()));
        w.cat.Wf = pf;
      }
      ETD_TRY_OR(fail, P.upload(&w.cat.b, bc.data(), H));
      if (H == 512 && d->I == 2048 && fused_pmlp_on()) {
        const float* W1 = Ld.get(p + "mlp.dense_h_to_4h.weight", (int64_t)d->I * H);
        if (!W1) return fail(ETD_EINVAL);
        std::vector<uint16_t> w1((size_t)d->I * H), ws((size_t)DMLP_STREAM_ELEMS);
        for (size_t i = 0; i < w1.size(); ++i) w1[i] = f2bf_h(W1[i]);
        pack_dmlp_weights(w1.data(), wc.data(), ws.data());
        uint16_t* pm; ETD_TRY_OR(fail, P.upload(&pm, ws.data(), ws.size()));
        w.mlp_frag = pm;
      }
    }
  }
  ETD_TRY_OR(fail, load_vec(d, Ld, "transformer.final_layer_norm.weight", H, &d->lnfg));
  ETD_TRY_OR(fail, load_vec(d, Ld, "transformer.final_layer_norm.bias", H, &d->lnfb));
  ETD_TRY_OR(fail, load_lin(d, Ld, "lm_head", d->V, H, false, &d->head));
  if (!d->bf16w) {
    const float* gf = Ld.get("transformer.final_layer_norm.weight", H); const float* bf_ = Ld.get("transformer.final_layer_norm.bias", H);
    if (!gf || !bf_) return fail(ETD_EINVAL);
    d->head.g3.x_log2 = g3_scale_log2(g3_bound_ln(gf, bf_, H));
  }
  if (d->bf16w && H % 16 == 0) {
    // the same d16 values in the order one wave's A-operand loads want them: (tile t, k-step s, lane l) holds row
    // 32 t + (l & 31), columns 16 s + 8 (l >> 5) .. +8 -- each load instruction then reads one contiguous 1 KiB block
    // instead of 32 B out of 32 different rows (the decode-step head kernel lives on one CU per 32 streams: its L1 traffic counts)
    const float* W = Ld.get("lm_head.weight", (int64_t)d->V * H);
    if (!W) return fail(ETD_EINVAL);
    const int tiles = d->head.Npad / 32, ks = H / 16;
    std::vector<uint16_t> hp((size_t)tiles * ks * 64 * 8, 0);
    for (int t = 0; t < tiles; ++t)
      for (int sx = 0; sx < ks; ++sx)
        for (int l = 0; l < 64; ++l) {
          const int row = t * 32 + (l & 31);
          if (row >= d->V) continue;
          for (int e = 0; e < 8; ++e) hp[(((size_t)t * ks + sx) * 64 + l) * 8 + e] = f2bf_h(W[(size_t)row * H + sx * 16 + (l >> 5) * 8 + e]);
        }
    uint16_t* pp; ETD_TRY_OR(fail, P.upload(&pp, hp.data(), hp.size()));
    d->head_frag = pp;
  }
  {
    // RoPE tables as HF builds them in fp32: inv_freq = 1/theta^(2i/rot), angle = pos * inv_freq (modeling_gpt_neox.py:72-107)
    std::vector<float> cs((size_t)d->ctx * 8), sn((size_t)d->ctx * 8);
    for (int i = 0; i < 8; ++i) {
      const float inv = 1.0f / powf(c.rope_theta, (float)(2 * i) / 16.0f);
      for (int p = 0; p < d->ctx; ++p) { const float ang = (float)p * inv; cs[(size_t)p * 8 + i] = cosf(ang); sn[(size_t)p * 8 + i] = sinf(ang); }
    }
    ETD_TRY_OR(fail, P.upload(&d->rope_cos, cs.data(), cs.size()));
    ETD_TRY_OR(fail, P.upload(&d->rope_sin, sn.data(), sn.size()));
  }
  d->n_weight_allocs = P.mark();
  ETD_TRY_OR(fail, alloc_workspaces(d));
  if (hipDeviceSynchronize() != hipSuccess) { g_etd_err = "decoder_create: device synchronisation failed"; return fail(ETD_EHIP); }
  *out = d;
  return ETD_OK;
}

// clone / destroy bookkeeping of a weight-sharing family (n_clones, zombie) runs under one process-wide lock: handles of a family
// may be cloned and destroyed from different threads
static std::mutex g_family_mu;

extern "C" int etd_decoder_clone(etd_dec* src, etd_dec** out) {
  if (!src || !out) ETD_FAIL(ETD_EINVAL, "decoder_clone: null argument");
  etd_dec* own = src->weights_owner ? src->weights_owner : src;
  {
    std::lock_guard<std::mutex> lk(g_family_mu);
    if (own->zombie) ETD_FAIL(ETD_EINVAL, "decoder_clone: the source handle was destroyed");
    ++own->n_clones;          // taken BEFORE the workspaces are built: the owner cannot free the weights underneath this clone
  }
  auto unref = [own]() {
    bool last;
    { std::lock_guard<std::mutex> lk(g_family_mu); last = --own->n_clones == 0 && own->zombie; }
    if (last) { own->pool.free_all(); delete own; }
  };
  etd_dec* d = new etd_dec();
  d->cfg = own->cfg; d->bf16w = own->bf16w;
  d->H = own->H; d->I = own->I; d->V = own->V; d->L = own->L; d->nh = own->nh; d->S = own->S; d->ctx = own->ctx;
  d->Mmax = own->Mmax; d->Mcap = own->Mcap; d->out_cap = own->out_cap;
  d->word = own->word; d->cls_emb = own->cls_emb; d->attr_tab = own->attr_tab; d->layers = own->layers;
  d->lnfg = own->lnfg; d->lnfb = own->lnfb; d->head = own->head; d->head_frag = own->head_frag;
  d->rope_cos = own->rope_cos; d->rope_sin = own->rope_sin;
  d->host_len.assign(d->S, 0);
  d->host_key.resize(d->S);
  for (int i = 0; i < d->S; ++i) d->host_key[i] = (unsigned long long)i;
  d->weights_owner = own;
  int rc = alloc_workspaces(d);
  if (!rc && hipDeviceSynchronize() != hipSuccess) { g_etd_err = "decoder_clone: device synchronisation failed"; rc = ETD_EHIP; }
  if (rc) { free_unborn(d); unref(); return rc; }
  *out = d;
  return ETD_OK;
}

extern "C" void etd_decoder_destroy(etd_dec* d) {
  if (!d) return;
  (void)hipDeviceSynchronize();   // kernels of this handle may still be in flight
  for (auto& kv : d->graphs) (void)hipGraphExecDestroy(kv.second);
  d->graphs.clear();
  if (d->trace) { (void)hipFree(d->trace); d->trace = nullptr; }
  if (d->trace_step) { (void)hipFree(d->trace_step); d->trace_step = nullptr; }
  if (d->trace_pk) { (void)hipFree(d->trace_pk); d->trace_pk = nullptr; }
  if (d->trace_q) { (void)hipFree(d->trace_q); d->trace_q = nullptr; }
  if (d->trace_dbg) { (void)hipFree(d->trace_dbg); d->trace_dbg = nullptr; }
  if (d->stamp_dev) { (void)hipFree(d->stamp_dev); d->stamp_dev = nullptr; }
  if (d->logits_dbg) { (void)hipFree(d->logits_dbg); d->logits_dbg = nullptr; }
  if (d->sc_i) { (void)hipFree(d->sc_i); d->sc_i = nullptr; }
  if (d->sc_f) { (void)hipFree(d->sc_f); d->sc_f = nullptr; }
  if (d->sc_d) { (void)hipFree(d->sc_d); d->sc_d = nullptr; }
  if (d->sc_x) { (void)hipFree(d->sc_x); d->sc_x = nullptr; }
  if (d->pin_stage) { (void)hipHostFree(d->pin_stage); d->pin_stage = nullptr; }
  if (d->pin_rb) { (void)hipHostFree(d->pin_rb); d->pin_rb = nullptr; }
  if (d->pin_stage_evt) { (void)hipEventDestroy(d->pin_stage_evt); d->pin_stage_evt = nullptr; }
  if (d->weights_owner) {
    etd_dec* own = d->weights_owner;
    d->pool.free_all();
    delete d;
    bool last;
    { std::lock_guard<std::mutex> lk(g_family_mu); last = --own->n_clones == 0 && own->zombie; }
    if (last) { own->pool.free_all(); delete own; }
    return;
  }
  bool keep;
  { std::lock_guard<std::mutex> lk(g_family_mu); keep = d->n_clones > 0; if (keep) d->zombie = true; }
  if (keep) {
    // clones still read the weights: release this handle's own workspaces now, the weights with the last clone
    d->pool.free_from(d->n_weight_allocs);
    return;
  }
  d->pool.free_all();
  delete d;
}

// token choice + stream state update from d->logits for M rows (the caller adds the sampling fields)
static DArgmaxArgs argmax_args(const etd_dec* d, const DecRows& rows, int M) {
  DArgmaxArgs am = {};
  am.logits = d->logits; am.ldl = d->V; am.V = d->V; am.M = M; am.rows = rows; am.eos = d->eos; am.limit = d->limit;
  am.cur_tok = d->cur_tok; am.len = d->len; am.done = d->done; am.n_out = d->n_out; am.out_tok = d->out_tok; am.out_cap = d->out_cap;
  return am;
}
extern "C" int etd_decoder_begin_bars(etd_dec* d, int n, const int32_t* slots, const int32_t* T, const int32_t* ids, const int32_t* cls,
                                      const int32_t* attrs4, const int32_t* tgt_attrs4, const int32_t* eos_ids, const int32_t* limits, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || n < 1 || !T || !tgt_attrs4 || !eos_ids || !limits) ETD_FAIL(ETD_EINVAL, "begin_bars: bad arguments");
  std::vector<int> init((size_t)7 * n);
  for (int i = 0; i < n; ++i) {
    if (limits[i] < 1 || limits[i] > d->out_cap) ETD_FAIL(ETD_EINVAL, "begin_bars: limit %d outside [1, %d]", limits[i], d->out_cap);
    // positions a bar touches: the prompt's T, then one per generated token that is fed back (all but the last) -- past max_ctx the
    // K/V rows could not be stored and the RoPE table would be read out of bounds
    if ((long long)T[i] + limits[i] - 1 > d->ctx) ETD_FAIL(ETD_EINVAL, "begin_bars: prompt of %d tokens + limit %d needs %d KV positions, max_ctx is %d", T[i], limits[i], T[i] + limits[i] - 1, d->ctx);
    for (int k = 0; k < 4; ++k) if (tgt_attrs4[4 * i + k] < 0 || tgt_attrs4[4 * i + k] >= d->cfg.num_attribute_bins) ETD_FAIL(ETD_EINVAL, "begin_bars: target attribute out of range");
    init[7 * i] = slots ? slots[i] : 0;
    for (int k = 0; k < 4; ++k) init[7 * i + 1 + k] = tgt_attrs4[4 * i + k];
    init[7 * i + 5] = eos_ids[i]; init[7 * i + 6] = limits[i];
  }
  if (d->sampling && d->keys_dirty) {
    HIP_TRY(hipMemcpyAsync(d->rng_key, d->host_key.data(), (size_t)d->S * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    d->keys_dirty = false;
  }
  // the row-finish counters (ETD_ROWFIN=1) are zero between launches by construction (the last arriver resets its word); a launch
  // that died half way would leave them poisoned for good, so every bar starts from zero anyway (16 KiB, on the stream)
  if (rowfin_on() && d->row_cnt) HIP_TRY(hipMemsetAsync(d->row_cnt, 0, (size_t)d->L * DS_STEP_MAX_ROWS * sizeof(int), st));
  Staged sg; float* hf = nullptr;
  bool compact = false;
  ETD_TRY(stage_and_forward(d, n, slots, T, ids, cls, attrs4, init.data(), &sg, &hf, st, &compact));
  // only each prompt's last position feeds the first generated token (etude_decoder.py:317)
  if (compact) {
    ETD_TRY(head_logits(d, hf, n, d->logits, st));           // (the last layer already ran on those rows alone)
  } else {
    ETD_TRY(launch_gather_rows(hf, sg.last_idx, n, d->H, d->hlast, st));
    ETD_TRY(head_logits(d, d->hlast, n, d->logits, st));
  }
  DArgmaxArgs am = argmax_args(d, DecRows{sg.last_slot, sg.last_pos, sg.last_active}, n);
  if (d->sampling) { am.samp = d->samp_dev; am.rng_key = d->rng_key; }
  ETD_TRY(launch_dargmax(am, st));
  d->bar_logit_rows = n;
  return ETD_OK;
}

extern "C" int etd_decoder_set_sampling(etd_dec* d, float temperature, float top_p, unsigned long long seed, void* stream) {
  if (!d || !(temperature >= 0.f) || !(top_p == top_p)) ETD_FAIL(ETD_EINVAL, "set_sampling: bad arguments");
  if (temperature > 0.f && d->V > 256) ETD_FAIL(ETD_EINVAL, "set_sampling: sampling supports vocabularies up to 256 entries");
  DSampleCfg c; c.inv_temp = temperature > 0.f ? 1.0f / temperature : 0.f; c.top_p = top_p; c.seed = seed;
  HIP_TRY(hipMemcpyAsync(d->samp_dev, &c, sizeof(c), hipMemcpyHostToDevice, (hipStream_t)stream));   // pageable source: staged before return
  d->sampling = temperature > 0.f;
  return ETD_OK;
}

extern "C" int etd_decoder_set_keys(etd_dec* d, int n, const int32_t* slots, const unsigned long long* keys) {
  if (!d || n < 1 || !slots || !keys) ETD_FAIL(ETD_EINVAL, "set_keys: bad arguments");
  for (int i = 0; i < n; ++i) { ETD_TRY(check_slot(d, slots[i])); d->host_key[slots[i]] = keys[i]; }
  d->keys_dirty = true;
  return ETD_OK;
}

extern "C" int etd_decoder_begin_bar(etd_dec* d, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                                     const int32_t* tgt_attrs4, int eos_id, int limit, void* stream) {
  const int32_t sl = slot, tt = T, eo = eos_id, li = limit;
  return etd_decoder_begin_bars(d, 1, &sl, &tt, ids, cls, attrs4, tgt_attrs4, &eo, &li, stream);
}

// the fused step's last launch: final LayerNorm + lm_head + token choice + stream state of `M` rows of hf, then the next step's rows, embeddings and layer-0 LayerNorms
static DHeadArgs head_args(const etd_dec* d, const float* hf, int M, int vpad) {
  const Layer& w0 = d->layers[0];
  DHeadArgs hd = {};
  hd.hfin = hf; hd.M = M; hd.H = d->H; hd.V = d->V; hd.Vpad = vpad;
  hd.lnf_g = d->lnfg; hd.lnf_b = d->lnfb; hd.eps = d->cfg.layer_norm_eps; hd.Whead = (const d16*)d->head_frag;
  hd.row_slot = d->row_slot; hd.row_pos = d->row_pos; hd.row_active = d->row_active; hd.row_sp = d->row_sp;
  hd.cur_tok = d->cur_tok; hd.len = d->len; hd.done = d->done; hd.n_out = d->n_out; hd.out_tok = d->out_tok; hd.out_cap = d->out_cap;
  hd.eos = d->eos; hd.limit = d->limit; hd.tgt_attrs = d->tgt_attrs; hd.tgt_proj = d->tgt_proj; hd.tgt_cls = 2; hd.n_bins = d->cfg.num_attribute_bins;
  hd.word = d->word; hd.cls_emb = d->cls_emb; hd.attr_tab = d->attr_tab;
  hd.g1 = w0.ln1g; hd.b1 = w0.ln1b; hd.g2 = w0.ln2g; hd.b2 = w0.ln2b;
  hd.h = d->h; hd.x1 = d->X1b; hd.x2 = d->X2b;
  hd.samp = d->samp_dev; hd.rng_key = d->rng_key;             // the device-side config selects greedy / sampling
  hd.logits_dbg = d->logits_dbg_on ? d->logits_dbg : nullptr;
  return hd;
}
extern "C" int etd_decoder_step(etd_dec* d, const int32_t* slots, int n_active, int n_steps, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !slots || n_active < 1 || n_active > d->S || n_steps < 1) ETD_FAIL(ETD_EINVAL, "decoder_step: bad args");
  for (int i = 0; i < n_active; ++i) ETD_TRY(check_slot(d, slots[i]));
  ETD_TRY(taps_fit(d, n_active, std::max(d->I / 512 + d->nh, DS_K_SPLITS)));      // (before the slot list is uploaded: a tapped call that does not fit launches nothing)
  if ((int)d->last_slots.size() != n_active || memcmp(d->last_slots.data(), slots, (size_t)n_active * 4)) {
    d->last_slots.assign(slots, slots + n_active);
    HIP_TRY(hipMemcpyAsync(d->slots_dev, d->last_slots.data(), (size_t)n_active * 4, hipMemcpyHostToDevice, st));
  }
  d->host_n_out_valid = false;
  {
    // Two rows of a head per attention workgroup (dec_kernels.hip, launch_dstep_attn_down) or one: BIT-IDENTICAL results
    // (tests/test_gpu_decoder.py::test_paired_rows_form_is_bit_identical), so the choice is a pure performance matter -- and it is a
    // deterministic function of (rows, mean context) alone, part of the captured graph's key.  Measured on MI355X (round 2: tools/README.md "pair
    // sweeps"; round 3 at 432 rows: profiles/r03_*): the pair form pays from 32 rows up at mean contexts 192 .. 1024 unless the launch's
    // workgroups quantise badly over the 256 CUs (64 + 8 M one-row workgroups of 1 unit against 32 + 4 M pair workgroups of 2 units: the
    // busiest CU decides), which matters up to ~128 rows only.
    double ctx_sum = 0;
    for (int i = 0; i < n_active; ++i) ctx_sum += d->host_len[slots[i]] + 1;
    const double mean_ctx = ctx_sum / n_active;
    bool pair = n_active >= 32 && mean_ctx >= 192.0 && mean_ctx <= 1024.0;
    if (pair && n_active <= 128) {
      const int u1 = (64 + 8 * n_active + 255) / 256, u2 = 2 * ((32 + 4 * n_active + 255) / 256);
      pair = u2 <= u1;
    }
    d->step_pair = d->force_pair < 0 ? pair : (d->force_pair > 0 && n_active >= 2);
  }
  d->rows_identity = true;
  for (int i = 0; i < n_active; ++i) if (slots[i] != i) { d->rows_identity = false; break; }
  // d16 batched decode step on the fused kernels: [embed + LayerNorm] once per call, then per step 4 launches per layer
  // (QKV|up, attention, down|dense, residual + LayerNorm) and one head launch that also prepares the next step's rows
  const int vpad = (d->V + 31) / 32 * 32;
  // A single stream steps on the fused kernels too (round 3; before: the GEMV sequence of rounds 1-2): 25 launches per step instead of ~36 and the same
  // arithmetic as inside a batch -- one job of 92 bars x 48 tokens 1.09 -> 0.66 s (tools/runs3/r3_run20.sh), every decoder golden unchanged.
  const bool fused = d->bf16w && n_active <= DS_STEP_MAX_ROWS && step_shape(d) && vpad <= 256 && vpad <= d->head.Npad && d->head_frag;
  d->last_step_fused = fused;
  d->stamp_on = d->stamp_armed && d->stamp_skip <= 0;          // (a whole call is stamped or not: the scheduler issues one bar's steps per call)
  if (d->stamp_armed && d->stamp_skip > 0) d->stamp_skip -= n_steps;
  auto embed = [&](hipStream_t s_) -> int {
    DEmbedArgs e = {};
    e.slots = d->slots_dev; e.len = d->len; e.done = d->done; e.row_slot_out = d->row_slot; e.row_pos_out = d->row_pos; e.row_active_out = d->row_active; e.row_sp_out = d->row_sp;
    e.cur_tok = d->cur_tok; e.tgt_attrs = d->tgt_attrs; e.tgt_cls = 2 /* TGT_CLASS_ID, etude/data/dataset.py:19 */;
    e.M = n_active; e.H = d->H; e.n_bins = d->cfg.num_attribute_bins;
    e.word = d->word; e.cls_emb = d->cls_emb; e.attr_tab = d->attr_tab; e.h = d->h;
    e.rows = DecRows{d->row_slot, d->row_pos, d->row_active};
    return launch_dembed(e, s_);
  };
  // K and V rows one layer's attention launch reads at step `s` of this call: every row's context so far (+ the row it appends)
  const double kv_row_bytes = (double)d->nh * 64 * 2 * (d->bf16w ? 2 : 4);
  auto step_kv_bytes = [&](int s) {
    double b = 0;
    for (int i = 0; i < n_active; ++i) { const int c = d->host_len[slots[i]] + 1 + s; b += (double)(c < d->ctx ? c : d->ctx) * kv_row_bytes; }
    return b;
  };
  int eager_step = 0;
  auto one_step = [&](hipStream_t s_) -> int {
    d->attn_bytes_hint = step_kv_bytes(eager_step);     // K/V bytes ONE layer's attention launch of this step reads (profiler byte counts)
    ++eager_step;
    const DecRows rows{d->row_slot, d->row_pos, d->row_active};
    if (!fused) ETD_TRY(embed(s_));
    if (fused && d->taps_on) {
      if (d->taps.step_slot) HIP_TRY(hipMemcpyAsync(d->taps.step_slot, d->row_slot, (size_t)n_active * 4, hipMemcpyDeviceToDevice, s_));
      if (d->taps.step_pos) HIP_TRY(hipMemcpyAsync(d->taps.step_pos, d->row_pos, (size_t)n_active * 4, hipMemcpyDeviceToDevice, s_));
    }
    float* hf = nullptr;
    ETD_TRY(fused ? forward_skinny16(d, n_active, rows, true, s_, &hf) : forward_rows(d, n_active, rows, nullptr, nullptr, s_, &hf, nullptr));
    if (fused) {
      ETD_TRY(launch_dstep_head(head_args(d, hf, n_active, vpad), s_));
      if (d->taps_on) {
        ETD_TRY(tap_rows(d, d->taps.next_h, 0, d->h, n_active, d->H, 4, s_));
        ETD_TRY(tap_rows(d, d->taps.next_ln1, 0, d->X1b, n_active, d->H, 2, s_));
        ETD_TRY(tap_rows(d, d->taps.next_ln2, 0, d->X2b, n_active, d->H, 2, s_));
        ETD_TRY(tap_rows(d, d->taps.next_pos, 0, d->row_pos, n_active, 1, 4, s_));
      }
      if (d->trace) {
        ETD_TRY(trace_rows(d, d->h, d->H, d->H, 1, 0, n_active, ETD_TRACE_LAYER * d->L * n_active, s_));
        ETD_TRY(trace_rows(d, d->cur_tok, 1, 1, 1, 0, n_active, ETD_TRACE_LAYER * d->L * n_active + n_active, s_));
        hipLaunchKernelGGL(k_trace_next, dim3(1), dim3(1), 0, s_, d->trace_step);
      }
      return ETD_OK;
    }
    ETD_TRY(head_logits(d, hf, n_active, d->logits, s_));
    DArgmaxArgs am = argmax_args(d, rows, n_active);
    am.samp = d->samp_dev; am.rng_key = d->rng_key;
    ETD_TRY(launch_dargmax(am, s_));
    return ETD_OK;
  };
  if (fused) {
    // rows, embeddings and first-layer LayerNorms of the FIRST step of this call (every later step gets them from the head kernel)
    ETD_TRY(embed(st));
    ETD_TRY(ln_rows16(d, 0, d->h, n_active, st));
  }
  // The step is ~50 short dependent kernels: replay it as a hipGraph (captured once per n_active; every
  // kernel argument is a fixed workspace/state pointer, the slot list lives in device memory).  Capture needs
  // a non-default stream and must not contain the profiler's event records.
  const bool use_graph = st != nullptr && !prof_enabled() && !ETD_XENV("ETD_NO_GRAPH");
  if (use_graph) {
    const int gkey = 16 * n_active + (d->logits_dbg_on ? 8 : 0) + (d->stamp_on ? 4 : 0) + (d->step_pair ? 2 : 0) + (d->rows_identity ? 1 : 0);
    auto it = d->graphs.find(gkey);
    if (it == d->graphs.end()) {
      hipGraph_t g = nullptr;
      HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const int rc = one_step(st);
      const hipError_t ce = hipStreamEndCapture(st, &g);
      eager_step = 0;                                   // (the capture ran one_step once without executing it)
      if (rc != ETD_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
      if (ce != hipSuccess || !g) ETD_FAIL(ETD_EHIP, "decoder_step: stream capture failed: %s", hipGetErrorString(ce));
      hipGraphExec_t ge = nullptr;
      const hipError_t ie = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (ie != hipSuccess) ETD_FAIL(ETD_EHIP, "decoder_step: graph instantiate failed: %s", hipGetErrorString(ie));
      it = d->graphs.emplace(gkey, ge).first;
    }
    for (int s = 0; s < n_steps; ++s) HIP_TRY(hipGraphLaunch(it->second, st));
  } else {
    for (int s = 0; s < n_steps; ++s) ETD_TRY(one_step(st));
  }
  // exact host-side accounting of what was just issued (graph replays included), then the contexts move on
  {
    double kv = 0;
    for (int s2 = 0; s2 < n_steps; ++s2) kv += step_kv_bytes(s2);
    kv *= d->L;
    d->stat_steps += n_steps; d->stat_row_steps += (double)n_steps * n_active; d->stat_kv_bytes += kv; d->stat_attn_launches += (double)n_steps * d->L;
    if (d->stamp_on) d->stat_stamp_bytes += kv + (fused ? (double)n_steps * d->L * ((double)d->I + d->H) * d->H * 2.0 : 0.0);     // + the down and dense weights each fused launch streams (fp32: the attention launch alone)
    for (int i = 0; i < n_active; ++i) { int& hl = d->host_len[slots[i]]; hl = hl + n_steps < d->ctx - 1 ? hl + n_steps : d->ctx - 1; }
  }
  return ETD_OK;
}

extern "C" int etd_decoder_stats(etd_dec* d, double* out, int n, void* stream) {
  if (!d || !out || n < 1) ETD_FAIL(ETD_EINVAL, "decoder_stats: bad arguments");
  unsigned long long sum_ticks = 0, n_stamped = 0;
  if (d->stamp_dev) {
    std::vector<unsigned long long> sp(ETD_STAMP_HDR);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(sp.data(), d->stamp_dev, ETD_STAMP_HDR * 8, hipMemcpyDeviceToHost));
    sum_ticks = sp[0]; n_stamped = sp[1];
    for (int bank = 0; bank < 2; ++bank) {              // the launch(es) no later launch has folded in yet
      unsigned long long e = 0;
      for (int i = 0; i < 64; ++i) e = std::max(e, sp[8 + 64 * bank + i]);
      if (sp[2 + bank] != 0 && e > sp[2 + bank]) { sum_ticks += e - sp[2 + bank]; ++n_stamped; }
    }
  }
  double w = 0;
  for (const Layer& l : d->layers) w += ((double)l.qkv.N * l.qkv.K + (double)l.dense.N * l.dense.K + (double)l.up.N * l.up.K + (double)l.down.N * l.down.K) * (d->bf16w ? 2.0 : 4.0);
  w += (double)d->V * d->H * (d->bf16w ? 2.0 : 4.0);
  const double v[8] = {d->stat_steps, d->stat_row_steps, d->stat_kv_bytes, d->stat_attn_launches, (double)n_stamped, (double)sum_ticks * 1e-8 /* 100 MHz ticks -> s */, d->stat_stamp_bytes, w};
  for (int i = 0; i < n; ++i) out[i] = i < 8 ? v[i] : 0.0;
  return ETD_OK;
}

// (start, end) of every stamped attention launch since the last reset, in 100 MHz ticks of the device's s_memrealtime (ONE clock for every queue of the chip: the
// logs of several engines can be merged); out_pairs [cap][2]; *n = launches written (the log keeps the first ETD_STAMP_LOGCAP)
extern "C" int etd_decoder_stamp_log(etd_dec* d, unsigned long long* out_pairs, long long cap, long long* n, void* stream) {
  if (!d || !out_pairs || cap < 1 || !n) ETD_FAIL(ETD_EINVAL, "decoder_stamp_log: bad arguments");
  *n = 0;
  if (!d->stamp_dev) return ETD_OK;
  std::vector<unsigned long long> sp(ETD_STAMP_WORDS);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemcpy(sp.data(), d->stamp_dev, ETD_STAMP_WORDS * 8, hipMemcpyDeviceToHost));
  long long k = (long long)std::min<unsigned long long>(sp[1], ETD_STAMP_LOGCAP), w = 0;
  for (long long i = 0; i < k && w < cap; ++i, ++w) { out_pairs[2 * w] = sp[ETD_STAMP_HDR + 2 * i]; out_pairs[2 * w + 1] = sp[ETD_STAMP_HDR + 2 * i + 1]; }
  for (int bank = 0; bank < 2 && w < cap; ++bank) {     // the launch(es) no later launch has folded in yet
    unsigned long long e = 0;
    for (int i = 0; i < 64; ++i) e = std::max(e, sp[8 + 64 * bank + i]);
    if (sp[2 + bank] != 0 && e > sp[2 + bank]) { out_pairs[2 * w] = sp[2 + bank]; out_pairs[2 * w + 1] = e; ++w; }
  }
  *n = w;
  return ETD_OK;
}

extern "C" int etd_decoder_stats_reset(etd_dec* d, void* stream) {
  if (!d) ETD_FAIL(ETD_EINVAL, "decoder_stats_reset: null handle");
  d->stat_steps = d->stat_row_steps = d->stat_kv_bytes = d->stat_attn_launches = d->stat_stamp_bytes = 0;
  if (d->stamp_dev) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemset(d->stamp_dev, 0, ETD_STAMP_HDR * 8));          // (the log behind the header is indexed by the launch count, which restarts at zero)
  }
  return ETD_OK;
}

extern "C" int etd_decoder_stamp(etd_dec* d, int on, int skip_steps, void* stream) {
  if (!d || skip_steps < 0) ETD_FAIL(ETD_EINVAL, "decoder_stamp: bad arguments");
  if (on && !d->stamp_dev) {
    HIP_TRY(hipMalloc((void**)&d->stamp_dev, ETD_STAMP_WORDS * 8));
    HIP_TRY(hipMemset(d->stamp_dev, 0, ETD_STAMP_WORDS * 8));
  }
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  d->stamp_armed = on != 0; d->stamp_on = false; d->stamp_skip = on ? skip_steps : 0;
  return ETD_OK;
}

// test hook: pin the attention form of the fused decode step (-1: the host rule; 0: one row per workgroup; 1: two rows of a head per workgroup)
extern "C" int etd_debug_decoder_force_pair(etd_dec* d, int mode) {
  if (!d || mode < -1 || mode > 1) ETD_FAIL(ETD_EINVAL, "force_pair: bad arguments");
  d->force_pair = mode;
  return ETD_OK;
}

// test hook: after etd_debug_decoder_step_logits(d, 1, ...) every decode step stores its logits; out_host (may be null when switching)
// receives the LAST step's [n_active][V] rows, fused d16 step and unfused steps alike
extern "C" int etd_debug_decoder_step_logits(etd_dec* d, int on, float* out_host, int n_active, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || n_active < 0 || n_active > d->S) ETD_FAIL(ETD_EINVAL, "step_logits: bad arguments");
  HIP_TRY(hipStreamSynchronize(st));
  if (out_host && n_active > 0) {
    if (d->last_step_fused && !(d->logits_dbg_on && d->logits_dbg)) ETD_FAIL(ETD_EINVAL, "step_logits: the fused step stores its logits only while the hook is on");
    const float* src = d->last_step_fused ? d->logits_dbg : d->logits;       // (unfused steps leave [n][V] logits in the workspace anyway)
    HIP_TRY(hipMemcpy(out_host, src, (size_t)n_active * d->V * 4, hipMemcpyDeviceToHost));
  }
  if (on && !d->logits_dbg) HIP_TRY(hipMalloc((void**)&d->logits_dbg, (size_t)d->S * d->V * 4));
  d->logits_dbg_on = on != 0;
  return ETD_OK;
}

// test hook: the [n][V] last-position logits the latest begin_bars drew its first tokens from (they stay in the workspace)
extern "C" int etd_debug_decoder_bar_logits(etd_dec* d, float* out_host, int n, void* stream) {
  if (!d || !out_host || n < 1 || n > d->bar_logit_rows) ETD_FAIL(ETD_EINVAL, "bar_logits: bad arguments (the latest begin_bars had %d streams)", d ? d->bar_logit_rows : 0);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemcpy(out_host, d->logits, (size_t)n * d->V * 4, hipMemcpyDeviceToHost));
  return ETD_OK;
}

extern "C" int etd_decoder_poll(etd_dec* d, const int32_t* slots, int n, int32_t* done_out, int32_t* n_out_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !slots || n < 1 || !done_out || !n_out_out) ETD_FAIL(ETD_EINVAL, "decoder_poll: bad args");
  std::vector<int> dnv, nov;
  int *dn, *no;
  if (d->pin_rb) { dn = d->pin_rb; no = d->pin_rb + d->S; }
  else { dnv.resize(d->S); nov.resize(d->S); dn = dnv.data(); no = nov.data(); }
  HIP_TRY(hipMemcpyAsync(dn, d->done, (size_t)d->S * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(no, d->n_out, (size_t)d->S * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) { ETD_TRY(check_slot(d, slots[i])); done_out[i] = dn[slots[i]]; n_out_out[i] = no[slots[i]]; }
  memcpy(d->host_n_out.data(), no, (size_t)d->S * 4);
  d->host_n_out_valid = true;                     // nothing has been launched on this handle's streams since: read_many can size its copy
  return ETD_OK;
}

extern "C" int etd_decoder_read_tokens(etd_dec* d, int slot, int32_t* out, int cap, int* n, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  ETD_TRY(check_slot(d, slot));
  if (!out || !n) ETD_FAIL(ETD_EINVAL, "read_tokens: null");
  int cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d->n_out + slot, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (cnt > d->out_cap) cnt = d->out_cap;
  *n = cnt;
  if (cnt > cap) ETD_FAIL(ETD_ENOMEM, "read_tokens: need room for %d tokens", cnt);
  if (cnt > 0) {
    HIP_TRY(hipMemcpyAsync(out, d->out_tok + (size_t)slot * d->out_cap, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return ETD_OK;
}

extern "C" int etd_decoder_read_many(etd_dec* d, int n, const int32_t* slots, int32_t* out, int cap, int32_t* counts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || n < 1 || !slots || !out || !counts || cap < 1) ETD_FAIL(ETD_EINVAL, "read_many: bad args");
  for (int i = 0; i < n; ++i) ETD_TRY(check_slot(d, slots[i]));
  if (!d->host_n_out_valid) {
    HIP_TRY(hipMemcpyAsync(d->host_n_out.data(), d->n_out, (size_t)d->S * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // only the columns that hold tokens travel: [S rows][widest requested count] out of [S][out_cap]
  int wmax = 0;
  for (int i = 0; i < n; ++i) { int c = d->host_n_out[slots[i]]; if (c > d->out_cap) c = d->out_cap; if (c > wmax) wmax = c; }
  std::vector<int> allv;
  int* all;
  if (d->pin_rb) all = d->pin_rb + 2 * (size_t)d->S; else { allv.resize((size_t)d->S * (wmax > 0 ? wmax : 1)); all = allv.data(); }
  if (wmax > 0) {
    HIP_TRY(hipMemcpy2DAsync(all, (size_t)wmax * 4, d->out_tok, (size_t)d->out_cap * 4, (size_t)wmax * 4, (size_t)d->S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  for (int i = 0; i < n; ++i) {
    int c = d->host_n_out[slots[i]]; if (c > d->out_cap) c = d->out_cap;
    if (c > cap) ETD_FAIL(ETD_ENOMEM, "read_many: slot %d holds %d tokens (cap %d)", slots[i], c, cap);
    counts[i] = c;
    memcpy(out + (size_t)i * cap, all + (size_t)slots[i] * wmax, (size_t)c * 4);
  }
  return ETD_OK;
}

extern "C" int etd_decoder_generate_bar(etd_dec* d, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                                        const int32_t* tgt_attrs4, int eos_id, int limit, int32_t* out, int* n_out, void* stream) {
  ETD_TRY(etd_decoder_begin_bar(d, slot, ids, cls, attrs4, T, tgt_attrs4, eos_id, limit, stream));
  int dn = 0, no = 0;
  const int32_t sl = slot;
  int chunk = 8;
  while (true) {
    ETD_TRY(etd_decoder_poll(d, &sl, 1, &dn, &no, stream));
    if (dn) break;
    ETD_TRY(etd_decoder_step(d, &sl, 1, chunk, stream));
    if (chunk < 32) chunk *= 2;
  }
  return etd_decoder_read_tokens(d, slot, out, limit, n_out, stream);
}

extern "C" int etd_decoder_prefill_logits(etd_dec* d, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                                          float* logits_host, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits_host) ETD_FAIL(ETD_EINVAL, "prefill_logits: null");
  if (T > d->Mmax) ETD_FAIL(ETD_EINVAL, "prefill_logits: T=%d exceeds %d", T, d->Mmax);
  const int32_t sl = slot, tt = T;
  Staged sg; float* hf = nullptr;
  ETD_TRY(stage_and_forward(d, 1, &sl, &tt, ids, cls, attrs4, nullptr, &sg, &hf, st));
  ETD_TRY(head_logits(d, hf, T, d->logits, st));
  HIP_TRY(hipMemcpyAsync(logits_host, d->logits, (size_t)T * d->V * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}

// Teacher-forced scoring of n packed sequences (etude_hip.h).  Sequences go through the batched prefill in chunks of at most S sequences
// (the handle's slots are the scratch KV caches) and at most Mcap rows -- in the fp32 mode at most 512 rows unless one sequence is longer:
// a sequence then runs on the weight-streaming kernels (<= 512 rows) or alone on the 128-row tiles (longer) whatever its neighbours are,
// so its scores do not depend on max_streams or on the other sequences of the call.  The LM head runs on the rows that are scored only,
// gathered into blocks of a fixed score_hb rows (one head kernel for every block: again independent of the layout), into d->logits.
extern "C" int etd_decoder_score(etd_dec* d, int n, const int32_t* T, const int32_t* ids, const int32_t* cls, const int32_t* attrs4,
                                 const int32_t* labels, double* seq_logprob, int32_t* seq_tokens, int32_t* seq_hits,
                                 float* row_lp, int32_t* row_argmax, float* logits_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || n < 1 || !T || !ids || !cls || !attrs4 || !labels || !seq_logprob || !seq_tokens || !seq_hits) ETD_FAIL(ETD_EINVAL, "score: bad arguments");
  long long M = 0;
  for (int i = 0; i < n; ++i) {
    if (T[i] < 1 || T[i] > d->ctx) ETD_FAIL(ETD_EINVAL, "score: sequence %d has %d rows (max_ctx=%d)", i, T[i], d->ctx);
    M += T[i];
  }
  if (M > 0x7fffffffLL) ETD_FAIL(ETD_EINVAL, "score: %lld rows in one call", M);
  for (long long r = 0; r < M; ++r) {
    if (ids[r] < 0 || ids[r] >= d->V) ETD_FAIL(ETD_EINVAL, "score: token id %d out of range [0, %d) at row %lld", ids[r], d->V, r);
    if (cls[r] < 0 || cls[r] >= d->cfg.num_classes) ETD_FAIL(ETD_EINVAL, "score: class id %d out of range [0, %d) at row %lld", cls[r], d->cfg.num_classes, r);
    for (int k = 0; k < 4; ++k)
      if (attrs4[k * M + r] < 0 || attrs4[k * M + r] >= d->cfg.num_attribute_bins) ETD_FAIL(ETD_EINVAL, "score: attribute bin %d out of range [0, %d) at row %lld", attrs4[k * M + r], d->cfg.num_attribute_bins, r);
    if (labels[r] != ETD_IGNORE_LABEL && (labels[r] < 0 || labels[r] >= d->V)) ETD_FAIL(ETD_EINVAL, "score: label %d at row %lld is neither -100 nor in [0, %d)", labels[r], r, d->V);
  }
  const int S = d->S, Mcap = d->Mcap;
  if (!d->sc_x) {                                          // (allocated last: a call that failed half way through allocating starts over)
    for (void* p : {(void*)d->sc_i, (void*)d->sc_f, (void*)d->sc_d}) if (p) (void)hipFree(p);
    d->sc_i = nullptr; d->sc_f = nullptr; d->sc_d = nullptr;
    d->score_hb = d->Mmax < 256 ? d->Mmax : 256;
    const int hb = d->score_hb;
    HIP_TRY(hipMalloc((void**)&d->sc_i, ((size_t)3 * Mcap + hb + 4 * (size_t)S) * sizeof(int)));
    HIP_TRY(hipMalloc((void**)&d->sc_f, (size_t)2 * Mcap * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&d->sc_d, (size_t)S * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&d->sc_x, (size_t)hb * d->H * sizeof(float)));
  }
  const int hb = d->score_hb;
  int* lab_dev = d->sc_i; int* idx_dev = lab_dev + Mcap; int* r0_dev = idx_dev + Mcap + hb; int* len_dev = r0_dev + S;
  int* am_dev = len_dev + S; int* tok_dev = am_dev + Mcap; int* hit_dev = tok_dev + S;
  float* lp_dev = d->sc_f; float* lse_dev = lp_dev + Mcap;
  const int rowcap = d->bf16w ? Mcap : std::min(Mcap, G3_MIN_ROWS - 1);
  const bool full = logits_dev != nullptr;
  std::vector<int32_t> slots(S), a4c, up;
  for (int i = 0; i < S; ++i) slots[i] = i;
  long long r0 = 0;
  for (int i0 = 0; i0 < n;) {
    int k = 0; long long Mc = 0;
    while (i0 + k < n && k < S && (k == 0 || Mc + T[i0 + k] <= rowcap)) Mc += T[i0 + k++];
    const int mc = (int)Mc;
    // chunk rows [r0, r0 + mc): attributes re-laid out as [4][mc]; upload = [labels mc][row list, padded to whole head blocks][row0 k][len k]
    a4c.resize((size_t)4 * mc);
    for (int a = 0; a < 4; ++a) memcpy(a4c.data() + (size_t)a * mc, attrs4 + a * M + r0, (size_t)mc * 4);
    up.assign(labels + r0, labels + r0 + mc);
    for (int r = 0; r < mc; ++r) if (full || labels[r0 + r] != ETD_IGNORE_LABEL) up.push_back(r);
    const int nl = (int)up.size() - mc;
    const int nblk = (nl + hb - 1) / hb;
    up.resize((size_t)mc + (size_t)nblk * hb, 0);          // padding rows gather row 0 of the chunk; their results are never stored
    HIP_TRY(hipMemcpyAsync(lab_dev, up.data(), (size_t)mc * 4, hipMemcpyHostToDevice, st));
    if (nblk) HIP_TRY(hipMemcpyAsync(idx_dev, up.data() + mc, (size_t)nblk * hb * 4, hipMemcpyHostToDevice, st));
    up.clear();
    for (int i = 0, row = 0; i < k; ++i) { up.push_back(row); row += T[i0 + i]; }
    up.insert(up.end(), T + i0, T + i0 + k);
    HIP_TRY(hipMemcpyAsync(r0_dev, up.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(len_dev, up.data() + k, (size_t)k * 4, hipMemcpyHostToDevice, st));
    if (row_lp || row_argmax) {
      HIP_TRY(hipMemsetAsync(lp_dev, 0, (size_t)mc * 4, st));
      HIP_TRY(hipMemsetAsync(am_dev, 0xff, (size_t)mc * 4, st));      // -1: row not scored
    }
    Staged sg; float* hf = nullptr;
    ETD_TRY(stage_and_forward(d, k, slots.data(), T + i0, ids + r0, cls + r0, a4c.data(), nullptr, &sg, &hf, st));
    for (int b = 0; b < nblk; ++b) {
      const int nb = std::min(hb, nl - b * hb);
      ETD_TRY(launch_gather_rows(hf, idx_dev + (size_t)b * hb, hb, d->H, d->sc_x, st));
      ETD_TRY(head_logits(d, d->sc_x, hb, d->logits, st));
      ETD_TRY(launch_row_logprob(d->logits, d->V, d->V, nb, idx_dev + (size_t)b * hb, lab_dev, lp_dev, lse_dev, am_dev, st));
      if (full) HIP_TRY(hipMemcpyAsync(logits_dev + (size_t)(r0 + (long long)b * hb) * d->V, d->logits, (size_t)nb * d->V * 4, hipMemcpyDeviceToDevice, st));
    }
    ETD_TRY(launch_seq_reduce(r0_dev, len_dev, k, lab_dev, lp_dev, am_dev, d->sc_d, tok_dev, hit_dev, st));
    HIP_TRY(hipMemcpyAsync(seq_logprob + i0, d->sc_d, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(seq_tokens + i0, tok_dev, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(seq_hits + i0, hit_dev, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (row_lp) HIP_TRY(hipMemcpyAsync(row_lp + r0, lp_dev, (size_t)mc * 4, hipMemcpyDeviceToHost, st));
    if (row_argmax) HIP_TRY(hipMemcpyAsync(row_argmax + r0, am_dev, (size_t)mc * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                     // the host staging vectors and the device scratch are reused by the next chunk
    i0 += k; r0 += mc;
  }
  return ETD_OK;
}

// diagnostic: a 64-bit sum over every 32-bit word of everything this handle allocated except its weights (KV cache, workspaces,
// stream state) -- changes if anybody, this handle or another, writes a single word of it
__global__ void k_sum_words(const unsigned* __restrict__ p, long long n, unsigned long long* out) {
  unsigned long long s = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) s += (unsigned long long)p[i] * (unsigned long long)((i & 1023) + 1);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}
// out[0] = the sum over everything; out[1 + i] = allocation i of alloc_workspaces (in its order: K cache, V cache, h, h2, Q, AO, DO, M1,
// logits, qkv_raw, hlast, X1b, X2b, AOb, M1b, Pk, row_cnt, Xcat, Qb, samp, rng_key, row_sp, row_slot, ...) while cap allows
extern "C" int etd_debug_decoder_checksum(etd_dec* d, unsigned long long* out, int cap, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !out || cap < 1) ETD_FAIL(ETD_EINVAL, "decoder_checksum: bad arguments");
  const size_t first = d->weights_owner ? 0 : d->n_weight_allocs;
  const size_t n = d->pool.ptrs.size() - first;
  unsigned long long* acc = nullptr;
  HIP_TRY(hipMalloc(&acc, 8 * (n + 1)));
  HIP_TRY(hipMemsetAsync(acc, 0, 8 * (n + 1), st));
  for (size_t i = 0; i < n; ++i)
    hipLaunchKernelGGL(k_sum_words, dim3(1024), dim3(256), 0, st, (const unsigned*)d->pool.ptrs[first + i], (long long)(d->pool.bytes[first + i] / 4), acc + 1 + i);
  std::vector<unsigned long long> h(n + 1);
  HIP_TRY(hipMemcpyAsync(h.data(), acc, 8 * (n + 1), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  (void)hipFree(acc);
  for (size_t i = 1; i <= n; ++i) h[0] += h[i];
  for (int i = 0; i < cap; ++i) out[i] = (size_t)i <= n ? h[i] : 0ull;
  return ETD_OK;
}

// diagnostic: out[(layer * S + slot) * ctx + pos] = 32-bit sum over the K and V words of that position (all heads), d16 caches only
__global__ void k_kv_rowsums(const unsigned* __restrict__ K, const unsigned* __restrict__ V, int L, int S, int nh, int ctx, unsigned* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)L * S * ctx) return;
  const int pos = (int)(i % ctx), slot = (int)((i / ctx) % S), l = (int)(i / ((long long)ctx * S));
  unsigned s = 0;
  for (int hd = 0; hd < nh; ++hd) {
    const long long w0 = ((((long long)l * S + slot) * nh + hd) * ctx + pos) * 32;      // 64 d16 = 32 words
    for (int w = 0; w < 32; ++w) s += K[w0 + w] * (unsigned)(w + 1 + 64 * hd) + V[w0 + w] * (unsigned)(w + 33 + 64 * hd);
  }
  out[i] = s;
}
extern "C" int etd_debug_decoder_kv_rowsums(etd_dec* d, unsigned* out_host, long long cap, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !out_host || !d->bf16w) ETD_FAIL(ETD_EINVAL, "kv_rowsums: d16 handles only");
  const long long n = (long long)d->L * d->S * d->ctx;
  if (cap < n) ETD_FAIL(ETD_ENOMEM, "kv_rowsums: need room for %lld words", n);
  unsigned* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, n * 4));
  hipLaunchKernelGGL(k_kv_rowsums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned*)d->Kc, (const unsigned*)d->Vc, d->L, d->S, d->nh, d->ctx, dev);
  HIP_TRY(hipMemcpyAsync(out_host, dev, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  (void)hipFree(dev);
  return ETD_OK;
}

// Step trace (tools/probe_trace.py): after trace_begin every decode step of the d16 fused path records a hash of each row of each
// kernel's outputs -- per layer Q, gelu(up), the 12 split-K slabs, the residual stream and the next LayerNorm rows; then the next
// step's embeddings and tokens -- into a ring of cap_steps records.  words_per_step = (49 * layers + 2) * n_active.
extern "C" int etd_debug_decoder_trace_begin(etd_dec* d, int cap_steps, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || cap_steps < 1 || !d->bf16w) ETD_FAIL(ETD_EINVAL, "trace_begin: bad args");
  HIP_TRY(hipStreamSynchronize(st));
  for (auto& kv : d->graphs) (void)hipGraphExecDestroy(kv.second);       // the captured steps do not hold the trace launches
  d->graphs.clear();
  if (d->trace) { (void)hipFree(d->trace); d->trace = nullptr; }
  if (d->trace_step) { (void)hipFree(d->trace_step); d->trace_step = nullptr; }
  if (d->trace_pk) { (void)hipFree(d->trace_pk); d->trace_pk = nullptr; }
  if (d->trace_q) { (void)hipFree(d->trace_q); d->trace_q = nullptr; }
  HIP_TRY(hipMalloc(&d->trace_pk, (size_t)12 * d->S * d->H * 4));
  HIP_TRY(hipMalloc(&d->trace_q, (size_t)d->S * d->H * 4));
  if (!d->trace_dbg) HIP_TRY(hipMalloc(&d->trace_dbg, (size_t)d->nh * d->S * 256 * 8 * 4));
  const size_t bytes = (size_t)cap_steps * trace_wps(d, d->S) * 4;
  HIP_TRY(hipMalloc(&d->trace, bytes));
  HIP_TRY(hipMalloc(&d->trace_step, 4));
  HIP_TRY(hipMemsetAsync(d->trace, 0, bytes, st));
  HIP_TRY(hipMemsetAsync(d->trace_step, 0, 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  d->trace_cap = cap_steps;
  return ETD_OK;
}
extern "C" int etd_debug_decoder_trace_slabs(etd_dec* d, float* out_host, long long cap_floats, int n_active, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !d->trace_pk || !out_host || n_active < 1 || n_active > d->S) ETD_FAIL(ETD_EINVAL, "trace_slabs: bad args");
  const long long n = 12LL * n_active * d->H;
  if (cap_floats < n) ETD_FAIL(ETD_ENOMEM, "trace_slabs: need room for %lld floats", n);
  HIP_TRY(hipMemcpyAsync(out_host, d->trace_pk, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
// layer 0's queries [n_active][hidden] of the last traced step, and one (layer, slot, head)'s K and V cache rows [n_pos][64] (d16 bit patterns)
// the attention workgroups' per-lane softmax state of layer 0 in the last traced step: [heads][n_active][256][8]
extern "C" int etd_debug_decoder_trace_lanes(etd_dec* d, float* out_host, long long cap_floats, int n_active, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)(d ? d->nh : 0) * n_active * 256 * 8;
  if (!d || !d->trace_dbg || !out_host || n_active < 1 || n_active > d->S || cap_floats < n) ETD_FAIL(ETD_EINVAL, "trace_lanes: bad args");
  HIP_TRY(hipMemcpyAsync(out_host, d->trace_dbg, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
extern "C" int etd_debug_decoder_trace_q(etd_dec* d, float* out_host, long long cap_floats, int n_active, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !d->trace_q || !out_host || n_active < 1 || n_active > d->S || cap_floats < (long long)n_active * d->H) ETD_FAIL(ETD_EINVAL, "trace_q: bad args");
  HIP_TRY(hipMemcpyAsync(out_host, d->trace_q, (size_t)n_active * d->H * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
extern "C" int etd_debug_decoder_peek_kv(etd_dec* d, int layer, int slot, int head, int n_pos, unsigned short* k_out, unsigned short* v_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !d->bf16w || layer < 0 || layer >= d->L || slot < 0 || slot >= d->S || head < 0 || head >= d->nh || n_pos < 1 || n_pos > d->ctx || !k_out || !v_out)
    ETD_FAIL(ETD_EINVAL, "peek_kv: bad args");
  const size_t off = ((size_t)layer * d->layer_stride + (size_t)slot * d->slot_stride + (size_t)head * d->ctx * 64) * 2;
  HIP_TRY(hipMemcpyAsync(k_out, (const char*)d->Kc + off, (size_t)n_pos * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(v_out, (const char*)d->Vc + off, (size_t)n_pos * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
extern "C" int etd_debug_decoder_peek_kv_many(etd_dec* d, int layer, int n, const int32_t* slots, int n_pos, unsigned short* k_out, unsigned short* v_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !d->bf16w || layer < 0 || layer >= d->L || n < 1 || !slots || n_pos < 1 || n_pos > d->ctx || !k_out || !v_out) ETD_FAIL(ETD_EINVAL, "peek_kv_many: bad args");
  for (int i = 0; i < n; ++i) ETD_TRY(check_slot(d, slots[i]));
  for (int i = 0; i < n; ++i) {
    const size_t off = ((size_t)layer * d->layer_stride + (size_t)slots[i] * d->slot_stride) * 2, dst = (size_t)i * d->nh * n_pos * 64;
    // [heads][max_ctx][64] -> [heads][n_pos][64]
    HIP_TRY(hipMemcpy2DAsync(k_out + dst, (size_t)n_pos * 128, (const char*)d->Kc + off, (size_t)d->ctx * 128, (size_t)n_pos * 128, (size_t)d->nh, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpy2DAsync(v_out + dst, (size_t)n_pos * 128, (const char*)d->Vc + off, (size_t)d->ctx * 128, (size_t)n_pos * 128, (size_t)d->nh, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}
extern "C" int etd_debug_decoder_stage_taps(etd_dec* d, const etd_debug_dec_taps* t, void* stream) {
  if (!d || !d->bf16w) ETD_FAIL(ETD_EINVAL, "stage_taps: 16-bit handles only");
  if (t) {
    if (t->struct_bytes != (int)sizeof(etd_debug_dec_taps)) ETD_FAIL(ETD_EINVAL, "stage_taps: etd_debug_dec_taps of %d bytes, this library expects %d", t->struct_bytes, (int)sizeof(etd_debug_dec_taps));
    if (d->L > 31 || t->layer_mask >> d->L) ETD_FAIL(ETD_EINVAL, "stage_taps: layer_mask %#x names a layer beyond the model's %d", t->layer_mask, d->L);
    if (t->rows < 1 || t->hidden != d->H || t->intermediate != d->I || (t->slabs && t->slab_cap < 1))
      ETD_FAIL(ETD_EINVAL, "stage_taps: buffers stated for rows %d, hidden %d, intermediate %d, slab_cap %d; the model has hidden %d, intermediate %d", t->rows, t->hidden, t->intermediate, t->slab_cap, d->H, d->I);
    if (t->slices < __builtin_popcount(t->layer_mask)) ETD_FAIL(ETD_EINVAL, "stage_taps: layer_mask %#x needs %d slices, the buffers are stated to hold %d", t->layer_mask, __builtin_popcount(t->layer_mask), t->slices);
    if (rowfin_on()) ETD_FAIL(ETD_EINVAL, "stage_taps: not with ETD_ROWFIN=1 (the in-launch row finish leaves no slabs to tap)");
  }
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  for (auto& kv : d->graphs) (void)hipGraphExecDestroy(kv.second);       // captured steps hold the copies of the taps they were captured with, or none
  d->graphs.clear();
  d->taps_on = t != nullptr;
  d->taps = t ? *t : etd_debug_dec_taps{};
  return ETD_OK;
}
extern "C" int etd_debug_decoder_trace_read(etd_dec* d, unsigned* out_host, long long cap_words, int n_active, int* steps_done, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!d || !d->trace || !out_host || !steps_done || n_active < 1 || n_active > d->S) ETD_FAIL(ETD_EINVAL, "trace_read: bad args");
  const long long n = (long long)d->trace_cap * trace_wps(d, n_active);
  if (cap_words < n) ETD_FAIL(ETD_ENOMEM, "trace_read: need room for %lld words", n);
  HIP_TRY(hipMemcpyAsync(out_host, d->trace, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(steps_done, d->trace_step, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}

extern "C" double etd_decoder_step_bytes(const etd_dec* d, int n_streams, int ctx) {
  // weights once + per stream K and V of `ctx` positions over all layers (+ the appended K/V row)
  const double esz = d->bf16w ? 2.0 : 4.0;
  double w = 0;
  for (const Layer& l : d->layers) w += ((double)l.qkv.N * l.qkv.K + (double)l.dense.N * l.dense.K + (double)l.up.N * l.up.K + (double)l.down.N * l.down.K) * esz;
  w += (double)d->V * d->H * esz;
  const double kv = (double)n_streams * 2.0 * d->L * (double)(ctx + 1) * d->H * esz;
  return w + kv;
}
