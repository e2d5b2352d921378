/* etude_hip_debug.h -- diagnostic, measurement and test hooks of libetude_hip.so.
 *
 * NOT part of the drop-in boundary (include/etude_hip.h): nothing in etude_amd/'s serving path calls these.  They exist for
 * tests/ (taps, step logits, prompt assembly), tools/ (traces, aggressors, microbenchmarks) and the investigations recorded in
 * LABNOTES.md.  Same conventions as etude_hip.h (0 / negative ETD_E* codes, etd_last_error()). */
#ifndef ETUDE_HIP_DEBUG_H
#define ETUDE_HIP_DEBUG_H
#include "etude_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* measurement hook: device time per dependent (empty) kernel, launched eagerly vs replayed from a hipGraph */
int etd_debug_boundary_cost(int n_nodes, int iters, int big_args, void* stream, double* eager_us, double* graph_us);
/* measurement hook: average time (us) of the token-major bf16 GEMM kernel on a synthetic [M,K] x [N,K]^T problem (N % 256 == 0, K % 128 == 0) */
int etd_debug_linear(int M, int N, int K, int iters, void* stream, double* us);
/* Diagnostic aggressors (tools/probe_race.py): `iters` launches of one kernel type on private random buffers:
   which 0 = k_attn (extractor shape), 1 = k_attn causal ragged (prefill shape), 2 = k_linear with the LayerNorm epilogue, 3 = k_ln_rows. */
int etd_debug_kernel_loop(int which, int iters, void* stream);
/* Diagnostic: one launch of an empty kernel with k_embed's footprint (82 KiB static LDS, 296 registers) on the given grid. */
int etd_debug_empty_launch(int gx, int gy, int gz, int* sink_dev, void* stream);

/* test hook: fp32 velocity logits of the time heads [rows][n_note][128] for the NEXT transcript call (NULL = off) */
int etd_extractor_debug_vel_logits(etd_ext*, float* vel_logits_dev);
/* test hook: after stage s of the FIRST chunk copy the bf16 activation buffer to dst_dev (NULL = off).
 * 0 embed, 1-3 encoder layers, 4-6 freq-decoder layers [frames*n_note][256], 7 time input, 8-10 time layers. */
int etd_extractor_debug_tap(etd_ext*, int stage, void* dst_dev);

/* test hook (host only): the prompt etd_decoder_run_jobs builds for a bar given n_hist past (X, Y, attrs4) pairs; attrs4_out is [4][cap] */
int etd_debug_assemble_prompt(const etd_sched_cfg* cfg, int n_hist, const int32_t* const* hx, const int32_t* hxn, const int32_t* const* hy,
                              const int32_t* hyn, const int32_t* hattrs4, const int32_t* x, int xn, const int32_t* y_attrs4,
                              int32_t* ids_out, int32_t* cls_out, int32_t* attrs4_out, int cap, int* T_out);
/* test hook (host only): the teacher-forced sequence etd_decoder_score_jobs builds for a cover bar y ([Bar_BOS] + tokens, yn >= 1) after the
   same history: ids / cls / attrs4 = that prompt + y[1 : yn-1] (target class, y_attrs4), labels = -100 on every prompt row but the last, then y[1:].
   *T_out = rows (also when cap is too small: ETD_ENOMEM).  A bar of more than max_bar_token_limit tokens, or one not led by Bar_BOS, is ETD_EINVAL. */
int etd_debug_assemble_scored(const etd_sched_cfg* cfg, int n_hist, const int32_t* const* hx, const int32_t* hxn, const int32_t* const* hy,
                              const int32_t* hyn, const int32_t* hattrs4, const int32_t* x, int xn, const int32_t* y, int yn, const int32_t* y_attrs4,
                              int32_t* ids_out, int32_t* cls_out, int32_t* attrs4_out, int32_t* labels_out, int cap, int* T_out);

/* Diagnostic (tools/probe_race.py): weighted 64-bit sums over the words of the handle's KV cache, workspaces and stream state:
   out[0] = everything, out[1 + i] = its i-th allocation (as many as `cap` allows). */
int etd_debug_decoder_checksum(etd_dec*, unsigned long long* out, int cap, void* stream);
/* Diagnostic: out[(layer * max_streams + slot) * max_ctx + pos] = 32-bit sum over the K and V rows of that position (bf16 handles). */
int etd_debug_decoder_kv_rowsums(etd_dec*, unsigned* out_host, long long cap, void* stream);
/* Diagnostic step trace (tools/probe_trace.py): after trace_begin every bf16 decode step records a hash of each row of each kernel's
 * outputs into a ring of cap_steps records of (49 * layers + 2) * n_active words; trace_read copies the ring and the step count. */
int etd_debug_decoder_trace_begin(etd_dec*, int cap_steps, void* stream);
/* layer 0's 12 split-K slabs [12][n_active][512] of the last traced step */
int etd_debug_decoder_trace_slabs(etd_dec*, float* out_host, long long cap_floats, int n_active, void* stream);
/* layer 0's queries [n_active][hidden] of the last traced step; one (layer, slot, head)'s K / V cache rows [n_pos][64] as bf16 bit patterns */
/* per-lane softmax state of layer 0's attention workgroups in the last traced step: [heads][n_active][256][8] =
 * lr, mr, o[0] after the key loop; lr after merge stages 8, 16, 32; o[0] after stages 8 and 32 */
int etd_debug_decoder_trace_lanes(etd_dec*, float* out_host, long long cap_floats, int n_active, void* stream);
int etd_debug_decoder_trace_q(etd_dec*, float* out_host, long long cap_floats, int n_active, void* stream);
int etd_debug_decoder_peek_kv(etd_dec*, int layer, int slot, int head, int n_pos, unsigned short* k_out, unsigned short* v_out, void* stream);
int etd_debug_decoder_trace_read(etd_dec*, unsigned* out_host, long long cap_words, int n_active, int* steps_done, void* stream);

/* test hook: pin the attention form of the fused bf16 decode step: -1 = the library's rule (a function of rows and mean context), 0 = one row per
 * 4-wave workgroup, 1 = two rows of a head per 8-wave workgroup.  Both forms give bit-identical results (tests/test_gpu_decoder_parity.py). */
int etd_debug_decoder_force_pair(etd_dec*, int mode);
/* test hook: switch the per-step logit store of the decode step on / off and (out_host != NULL) copy out the LAST step's logits
 * [n_active][vocab] fp32 -- the fused bf16 step keeps its logits in LDS otherwise.  Stamped / logged steps use their own captured graphs. */
int etd_debug_decoder_step_logits(etd_dec*, int on, float* out_host, int n_active, void* stream);
/* test hook: the last-position logits [n][vocab] fp32 that the latest etd_decoder_begin_bars chose its n first tokens from (row i = the
 * call's i-th stream).  Valid until the next begin_bars, prefill or unfused decode step. */
int etd_debug_decoder_bar_logits(etd_dec*, float* out_host, int n, void* stream);
/* test hook (tests/test_gpu_decoder_stages.py): float taps of every stage of the 16-bit sequences (fused decode step, skinny sequence, batched prefill and
 * its last-rows tail).  While registered, each launch's output is copied (hipMemcpyAsync, device to device, right behind the launch) into the caller's DEVICE
 * buffers; a NULL member is off, etd_debug_decoder_stage_taps(d, NULL, ..) switches everything off.  Only layers in `layer_mask` are tapped; layer l's slice of a
 * buffer is slice popcount(layer_mask & ((1 << l) - 1)), and ONE MORE slice behind them belongs to the last-rows tail of a batched prefill (the last layer on the
 * prompts' last rows only, when that layer is in the mask).  Every buffer is [slices][rows][width] of the stated type; a call of M rows fills rows 0 .. M - 1 of
 * a slice (the tail: 0 .. n - 1).  `slabs` is [slices][slab_cap * rows * hidden] floats and receives the launch's split-K slabs as [n_slab][M][hidden], contiguous
 * (fused step: intermediate / 512 down slabs, then one dense slab per head; split-K down projection: 5).  In a multi-step call the last step's taps stay.
 * The sizes the caller states (rows, slices, hidden, intermediate, slab_cap) are checked against every call BEFORE anything is launched: a call that does not fit is
 * ETD_EINVAL.  Registering or clearing taps drops the captured step graphs, so a tapped step never replays a production graph and the reverse. */
typedef struct etd_debug_dec_taps {
  int struct_bytes;                   /* sizeof(etd_debug_dec_taps) of the caller */
  unsigned layer_mask;
  int rows, hidden, intermediate, slab_cap;
  int slices;                         /* slices every buffer holds: a call that would write more (layers in the mask, + 1 for a batched prefill's tail) is ETD_EINVAL */
  float* hin;                         /* fp32 [slices][rows][hidden]: residual stream entering the layer */
  void *ln1, *ln2;                    /* 16-bit [slices][rows][hidden]: the layer's two LayerNorm rows (X1b, X2b) */
  float* q;                           /* fp32 [slices][rows][hidden]: RoPE'd queries (step, skinny sequence, tail) */
  void* qb;                           /* 16-bit [slices][rows][hidden]: RoPE'd queries of the batched prefill */
  void* xcat;                         /* 16-bit [slices][rows][intermediate + hidden]: GELU(up) | attention output as the layer left it (the fused step writes no
                                         attention block, the fused prefill MLP no GELU block: those columns are stale) */
  float* slabs;                       /* fp32, see above */
  float* hout;                        /* fp32 [slices][rows][hidden]: residual stream leaving the layer */
  int32_t *step_slot, *step_pos;      /* int32 [rows]: the fused step's row -> (slot, position) as its layers read them */
  float* next_h; void *next_ln1, *next_ln2; int32_t* next_pos;      /* fused step's head kernel: next step's embeddings fp32 [rows][hidden], layer-0 LayerNorm rows, positions */
} etd_debug_dec_taps;
int etd_debug_decoder_stage_taps(etd_dec*, const etd_debug_dec_taps* taps, void* stream);
/* test hook: K and V cache rows of one layer, all heads: for each of n listed slots positions 0 .. n_pos - 1 -> k_out / v_out host [n][heads][n_pos][64] 16-bit patterns */
int etd_debug_decoder_peek_kv_many(etd_dec*, int layer, int n, const int32_t* slots, int n_pos, unsigned short* k_out, unsigned short* v_out, void* stream);

/* test hook (tests/test_gpu_sampling_exact.py): the sampler alone.  Token of each of M rows of V <= 256 device logits (row stride ld >= V) drawn by
 * the decoder's own sampling routine with per-row keys and draw counters (device arrays); temperature > 0.  No decoder state is involved. */
int etd_debug_sample_rows(const float* logits_dev, int M, int V, int ld, float temperature, float top_p, unsigned long long seed,
                          const unsigned long long* keys_dev, const unsigned* ctrs_dev, int* out_tok_dev, void* stream);

/* test hooks of the fp32-grade f16-split kernels (csrc/gemm3.h; tests/test_gpu_gemm3.py):
 * y[M][N] = x[M][K] w[N][K]^T + bias (x, y device fp32 row-major; w, bias host; x_bound = bound of |x| for the plane scale; gelu != 0: erf-GELU epilogue).
 * 2 .. 512 rows with K % 512 == 0 take the weight-streaming kernel (k_gemm3_s), which can apply LayerNorm(x; ln_g, ln_b, eps 1e-5) over K first (host vectors or NULL;
 * x_bound then bounds the LayerNorm output); everything else the 128 x 128 tile kernel (k_gemm3, no fused LayerNorm). */
int etd_debug_gemm3(const float* x_dev, int M, int K, const float* w_host, const float* bias_host, int N, float x_bound, int gelu, float* y_dev,
                    const float* ln_g_host, const float* ln_b_host, void* stream);
/* test hook (tests/test_gpu_gemm3_epilogues.py): ONE launch of k_gemm3 / k_gemm3_s with any epilogue, row strides and row metadata, through the code the engines
 * use (g3_lin_upload, g3_lin_args, launch_gemm3 / launch_gemm3_s).  Everything is validated on the host first -- every extent against the allocation sizes the caller
 * states, every slot / position against n_slots / rope_rows -- and a case that does not hold is ETD_EINVAL before anything is launched. */
enum { ETD_G3_KERNEL_AUTO = 0 /* gemm3_s_takes decides, as the decoder does */, ETD_G3_KERNEL_TILE = 1 /* k_gemm3 */, ETD_G3_KERNEL_SMALL = 2 /* k_gemm3_s */ };
enum { ETD_G3_EPI_BIAS = 0, ETD_G3_EPI_GELU = 1, ETD_G3_EPI_RESID = 2, ETD_G3_EPI_LOGITS = 3, ETD_G3_EPI_QKV = 4, ETD_G3_EPI_RELU = 6 };
typedef struct etd_debug_g3_case {
  int struct_bytes;                            /* sizeof(etd_debug_g3_case) of the caller */
  int kernel, epi;                             /* ETD_G3_KERNEL_*, ETD_G3_EPI_* */
  int M, N, K, ldx, ldy;                       /* row i of X = the K floats at X + i * ldx (ldx < K: overlapping rows); ldy >= N: BIAS / GELU / RELU / LOGITS */
  const float* X; long long x_elems;           /* device; floats allocated: (M - 1) ldx + K must fit */
  const float* W; const float* bias;           /* host [N][K], [N] or NULL (LOGITS never reads it) */
  float x_bound;                               /* bound of |x| (of the LayerNorm output when ln_g is set) for the plane scale */
  const float* ln_g; const float* ln_b; float ln_eps;      /* host [K] or NULL: LayerNorm over K fused in front (k_gemm3_s only) */
  float* Y; long long y_elems;                 /* device; (M - 1) ldy + N must fit */
  const float* add; const float* hin; float* hout; long long h_elems;      /* RESID, device [M][N] each (h_elems floats): hout = (y + add) + hin; add NULL = 0 (k_gemm3 only);
                                                                              hin == hout is allowed */
  const int32_t* pos; const int32_t* slot; const int32_t* active;          /* QKV, host [M]: 0 <= pos < rope_rows, 0 <= slot < n_slots */
  int n_heads, max_ctx, n_slots, rope_rows;    /* N == n_heads * 192; rows with pos >= max_ctx or active == 0 write no K / V */
  const float* rope_cos; const float* rope_sin;            /* host [rope_rows][8] */
  float* Q; long long q_elems;                 /* device [M][n_heads * 64] */
  float* Kc; float* Vc; long long kv_elems;    /* device [n_slots][n_heads][max_ctx][64] each */
} etd_debug_g3_case;
int etd_debug_gemm3_case(const etd_debug_g3_case* c, void* stream);
/* test hook: launch_ln_rows_f32 -- x1 = LayerNorm(h; g1, b1), x2 = LayerNorm(h; g2, b2) over rows of H features (h, x1, x2 device [M][H]; g / b host [H]; g2, b2, x2 all NULL or all set) */
int etd_debug_ln_rows_f32(const float* h_dev, int M, int H, const float* g1_host, const float* b1_host, const float* g2_host, const float* b2_host, float eps,
                          float* x1_dev, float* x2_dev, void* stream);
/* host-only test hook: g3_pack_weights_host of W [N][K] (K % 32 == 0) -- planes_out receives the f16 bit patterns in the streaming order
 * [Npad / 128 tile][K / 32 chunk][hi | lo][128 rows][32 k], Npad = N rounded up to 128; *n_out = their number (also when cap is too small: ETD_ENOMEM); *log2_out = log2 of the scale */
int etd_debug_g3_pack(const float* W, int N, int K, uint16_t* planes_out, long long cap, long long* n_out, int32_t* log2_out);

/* o = softmax(q k^T / 8) v per (sequence, head), head_dim 64: q / o [n_seq][Sq][heads * 64], k / v [n_seq][Sk][heads * 64] device fp32; causal != 0: query t sees keys 0 .. t
 * through the RAGGED path (K / V then laid out as a KV cache [n_seq slots][heads][Sk][64], lens_host[n_seq] prompt lengths <= Sq == Sk, q / o rows packed prompt after prompt) */
int etd_debug_attn3(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int n_seq, int n_heads, int Sq, int Sk, float q_bound, float k_bound, float v_bound,
                    int causal, const int32_t* lens_host, void* stream);
/* test hook (tests/test_gpu_attn3.py): ONE launch_attn3 call with every Attn3Args field the engines set -- row strides, sequence strides, buffers that interleave
 * Q | K | V, and for the ragged causal form the decoder's slots, slot stride and max_ctx.  seq_len == NULL is the strided form (every sequence Sq queries against Sk
 * keys, sequence s at X + s * x_seq); otherwise sequence s is a prompt of seq_len[s] rows: its Q / O rows are the global rows row0 + (lengths before it) + t of Q / O
 * (row stride ldq / ldo), its K / V rows positions 0 .. seq_len[s] - 1 of slot slot_of_seq[s] of a cache [n_slots][slot_stride], head h at h * max_ctx * 64 inside
 * the slot; Sq, Sk and the *_seq strides are not read.  The plane scales are g3_scale_log2 of the three bounds and are returned in log2_out3 (host, may be NULL).
 * Everything is validated on the host first: every element the kernel can read or write must lie inside the *_elems floats the caller states for that pointer, every
 * slot inside n_slots; a case that does not hold is ETD_EINVAL before anything is launched.  Synchronous. */
struct etd_debug_attn3_case {                  /* (the hook's own name: refer to it as `struct etd_debug_attn3_case`) */
  int struct_bytes;                            /* sizeof(struct etd_debug_attn3_case) of the caller */
  int n_seq, n_heads, Sq, Sk;
  const float* Q; long long q_elems; int ldq; long long q_seq;      /* device; ld* >= n_heads * 64, multiples of 4 like the *_seq strides */
  const float* K; long long k_elems; int ldk; long long k_seq;
  const float* V; long long v_elems; int ldv; long long v_seq;
  float* O; long long o_elems; int ldo; long long o_seq;            /* sequences of O must not overlap */
  float q_bound, k_bound, v_bound;             /* bounds of |q|, |k|, |v| for the plane scales */
  const int32_t* seq_len; const int32_t* slot_of_seq;               /* ragged causal: host [n_seq], 1 <= seq_len <= max_ctx, 0 <= slot_of_seq < n_slots */
  long long slot_stride; int max_ctx, n_slots, row0;                /* slot_stride >= n_heads * max_ctx * 64, a multiple of 4; row0 >= 0: global row of the first prompt's first query */
  int32_t* log2_out3;                          /* host [3] or NULL: q_log2, k_log2, v_log2 as used */
};
int etd_debug_attn3_case(const struct etd_debug_attn3_case* c, void* stream);
/* test hook (tests/test_gpu_attn3.py): ONE launch_dattn call of the fp32 decode-step attention (k_dattn<float>): row i's query q_dev [M][n_heads * 64] against positions
 * 0 .. min(pos_host[i], max_ctx - 1) of slot slot_host[i] of the fp32 caches kc_dev / vc_dev [n_slots][n_heads][max_ctx][64] (kv_elems floats each) -> o_dev
 * [M][n_heads * 64] (q_dev, o_dev: qo_elems floats each).  form 0: DecRows slot / pos arrays; 1: (slot, pos) pairs in row_sp; 2: row_sp with the `identity` promise
 * (row i is slot i), refused unless slot_host[i] == i and max_ctx >= 64, as launch_dattn's own rule implies.  Validated on the host first; synchronous. */
int etd_debug_dattn_f32(const float* q_dev, const float* kc_dev, const float* vc_dev, float* o_dev, long long qo_elems, long long kv_elems, int M, int n_heads, int n_slots,
                        int max_ctx, const int32_t* slot_host, const int32_t* pos_host, int form, void* stream);

/* host-only test hook: the load-time bounds behind the plane scales of csrc/gemm3.h -- out4 = { bound of LayerNorm(.; g, b) over K features, bound of W LN(.) + c,
 * bound of W x + c for |x| <= elem_bound, largest |value| in the packed f16 planes of W }, log2_out4 = the scale logarithms chosen for the three bounds and for W */
int etd_debug_g3_bounds(const float* W, const float* c, int N, int K, const float* g, const float* b, float elem_bound, float* out4, int32_t* log2_out4);

/* test hook: during the following etd_beat_forward calls copy the token rows after the conv front end and after time layer 0 ([rows][256], rows in the call's
 * global row order) to front_dev / layer0_dev (NULL = off). */
int etd_beat_debug_taps(etd_beat*, float* front_dev, float* layer0_dev);
/* test hook (tests/test_gpu_beat_stages.py): fp32 taps of every launch of the Beat-Transformer engine.  While registered, etd_beat_forward copies each launch's output
 * out of the shared workspace (hipMemcpyAsync, device to device, right behind the launch, on the call's stream) into the caller's DEVICE buffers, in the call's global
 * row ((song, instr, t)), frame ((song, t)) and tempo-segment order, whatever the chunking; the outputs of the call are bit-identical with taps on and off.  A NULL member
 * is off; etd_beat_debug_stage_taps(e, NULL), or a struct with a zero layer_mask and no front-end / part pointer, switches everything off.  Only the time layers in
 * `layer_mask` are tapped: layer l's slice of a per-layer buffer is slice popcount(layer_mask & ((1 << l) - 1)), and of an instrument-layer buffer (layers 3 .. 5)
 * popcount(layer_mask & 0x38 & ((1 << l) - 1)).  The sizes the caller states are checked against every call BEFORE anything is launched (a call with more rows,
 * frames or segments than stated is ETD_EINVAL), the geometry at registration. */
typedef struct etd_debug_beat_taps {
  int struct_bytes;                   /* sizeof(etd_debug_beat_taps) of the caller */
  unsigned layer_mask;
  int rows, frames, segs;             /* every buffer's extent per slice: rows = instr x frames of the call, segs = sum over songs of ceil(T / 128) */
  int d_hid;
  int slices, islices;                /* slices the per-layer / per-instrument-layer buffers hold */
  float *c1, *c2, *x3, *c3, *front;   /* front end: [rows][42][32] conv1 + pool + ReLU, [rows * 42][64] conv2 + bias (columns 31 .. 41 of a row read past it), [rows * 3][1152]
                                         conv3 patches, [rows * 3][256] conv3 + bias, [rows][256] tokens */
  float *ln1, *qkv, *skip, *x_attn, *tacc, *ln2, *hid, *x_ffn;      /* time layer: [slices][rows][256 | 768 | 256 | 256], tacc [slices][frames][256], [slices][rows][256 | d_hid | 256] */
  float *iln1, *iqkv, *iao, *ix_attn, *iln2, *ihid, *ix_ffn;        /* instrument layer: [islices][rows][256 | 768 | 256 | 256 | 256 | d_hid | 256] */
  float* part;                        /* [segs][256] tempo partial sums (calls with a tempo output) */
} etd_debug_beat_taps;
int etd_beat_debug_stage_taps(etd_beat*, const etd_debug_beat_taps* taps);

/* test hook: the Viterbi kernel of etd_dbn_track alone, on supplied densities: densities_dev fp64 device [T][K] (K = 2 for HMM 0, 3 for a bar HMM; -inf allowed)
 * -> path_out host int32 [T] (state per frame) and *logprob_out (host).  Synchronous, default stream. */
int etd_dbn_debug_viterbi(etd_dbn*, int hmm_index, const double* densities_dev, long long T, int32_t* path_out, double* logprob_out);

/* test hooks of etd_dtw_align, one pair each, feat_ptrs as there ([4] device pointers); synchronous, default stream, buffers of their own.
 * _cost: the fp32 cost matrix [N1][N2] the final DTW would see with the origin shifted by `shift` (0..11), formed by the kernel's own cost function -> cost_dev (device);
 *        more than 2^22 cells is ETD_EINVAL.  _total: D[-1,-1] of the final DTW with that shift (no transposition search) -> *total_host. */
int etd_dtw_debug_cost(etd_dtw*, const float* const* feat_ptrs, long long N1, long long N2, int shift, float* cost_dev);
int etd_dtw_debug_total(etd_dtw*, const float* const* feat_ptrs, long long N1, long long N2, int shift, double* total_host);
/* ... and its unfiltered step path, LAST point first: path_host int32 [cap][2] of (cover frame, origin frame), *n_out = points (<= N1 + N2 - 1); ETD_ENOMEM when cap is short */
int etd_dtw_debug_path(etd_dtw*, const float* const* feat_ptrs, long long N1, long long N2, int shift, int32_t* path_host, long long cap, long long* n_out);

/* HOST ONLY test hook: the stage taps of etd_alignfeat_run.  After a run the caller's workspace holds every intermediate stage of every song; this returns where song
 * `song` of a call with these lengths keeps them: out int64 [24] =
 *   [0] T  [1..3] samples of tiers 0, 1, 2  [4..6] chunks  [7..9] novelty frames  then BYTE offsets into the workspace: [10] x1 fp32  [11] x2 fp32
 *   [12] u fp64 (forward-filtered bands)  [13] y fp32 (zero-phase bands)  [14] chunk states fp64 [.][12]  [15] E fp32 [88][T]  [16] novelty fp32  [17] peak height fp32
 *   (0 = no peak)  [18] peak frame int32  [19] L = log(1 + 10000 CO) fp32 [12][T]  [20] g  [21] G fp32 [T]  [22] D fp32 [12][T];  [23] floats before the song's block
 *   in chroma_dev / dlnco_dev.  Per-band arrays hold bands 0 .. 87 in order, bands 0 .. 38 with tier 2's count, 39 .. 74 with tier 1's, 75 .. 87 with tier 0's. */
int etd_alignfeat_debug_layout(const etd_alignfeat*, int n_songs, const int64_t* N_host, int song, int64_t* out, int n_out);

/* HOST ONLY test hook: the stage taps of etd_tuning_run.  After a run the caller's workspace holds the stages of every song; this returns where song `song` of a call
 * with these lengths keeps them: out int64 [7] = [0] frames F = 1 + N / 8192  [1] groups of 8 frames  then BYTE offsets into the workspace: [2] the groups' partial
 * sums fp32 [groups][8193]  [3] Y fp32 [8193]  [4] Yi fp64 [8400]  [5] R fp64 [8400]  [6] sim fp64 [100]. */
int etd_tuning_debug_layout(const etd_tuning*, int n_songs, const int64_t* N_host, int song, int64_t* out, int n_out);
/* test hook: during the following etd_tuning_run calls the frame kernel also writes the power P[f][0 .. 8192] (fp32) of frames frames_host[0 .. n_frames) of song
 * `song` to power_dev [n_frames][8193] (device); n_frames 1 .. 8; a frame the song does not have makes the run ETD_EINVAL.  power_dev = NULL turns it off.  No
 * launch is added either way. */
int etd_tuning_debug_power(etd_tuning*, int song, const int32_t* frames_host, int n_frames, float* power_dev);

/* HOST ONLY test hook: the plan of an etd_resample_run with these shapes, one record per workgroup in launch order: out int64 [n_tiles][4] = song, channel (0 for a
 * mono song), first output n0, outputs (256, fewer in a channel's last tile).  *n_tiles is always set; capacity (in records) below it, or out = NULL, is ETD_ENOMEM. */
int etd_resample_debug_layout(const etd_resample*, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* mono_host, int64_t* out,
                              long long capacity, long long* n_tiles);

/* test hook: during the following etd_rhythm_run calls the kernel also copies out what it clustered: logioi_dev (DEVICE fp64, as long as onsets_dev): the centred,
 * clipped log-IOIs of cover b at [offsets[b] .. offsets[b + 1] - 1) -- the device's own logarithm, which may differ from numpy's by an ulp --; labels_dev (DEVICE
 * int8, same layout): the final labels; centres_dev (DEVICE fp64 [n_covers][8]): the final centres on the centred axis, NaN past k.  Entries of covers without an IPE
 * score are left untouched.  All three NULL turns it off.  No launch is added either way. */
int etd_rhythm_debug_logioi(etd_rhythm*, double* logioi_dev, signed char* labels_dev, double* centres_dev);

/* test hooks of the training engine (csrc/dec_train.hip), DEVICE fp32 buffers.
 * The GEMM family: C [M][N] (row stride ldc) = (accumulate ? C : 0) + product (+ bias [N], may be NULL), in the three forms of a linear layer:
 *   form 0  A [M][K] (lda) x B [N][K]^T (ldb)      Y  = X W^T
 *   form 1  A [M][K] (lda) x B [K][N]   (ldb)      dX = dY W
 *   form 2  A [K][M]^T (lda) x B [K][N] (ldb)      dW += dY^T X (the sum over K = batch rows in ascending order)
 * A row stride shorter than its row is ETD_EINVAL.  Asynchronous. */
int etd_debug_dtrain_gemm(int form, int M, int N, int K, const float* A_dev, int lda, const float* B_dev, int ldb, const float* bias_dev, float* C_dev, int ldc,
                          int accumulate, void* stream);
/* Causal attention forward + backward over n_seq packed sequences of T_host[s] rows, head_dim 64, no RoPE: qkv_dev [M][n_heads][q | k | v][64], dO_dev [M][n_heads * 64]
 * -> O_dev [M][n_heads * 64], lse_dev [M][n_heads], dqkv_dev in qkv's layout (scale 1 / 8 on the scores).  Synchronous. */
int etd_debug_dtrain_attn(int n_seq, const int32_t* T_host, int n_heads, const float* qkv_dev, const float* dO_dev, float* O_dev, float* lse_dev, float* dqkv_dev,
                          void* stream);
/* Stage taps of the training engine: every row and elementwise kernel on a caller's input, through the launcher (kernel, grid, block) the engine itself calls.
 * DEVICE fp32 buffers unless named _host.  A malformed argument is ETD_EINVAL before anything is launched.  Asynchronous unless said.
 *   ln          x [M][H] (any H >= 1) -> y1 = xhat g1 + b1; with g2, b2, y2 (all three or none) also y2; with mean, rstd [M] (both or neither) the statistics.
 *               With dy [M][H]: dx [M][H] += the input gradient of y1 (needs mean and rstd; dx is the caller's to initialise).
 *   gelu        x [n] -> y = gelu(x) (erf form); with dy [n]: dy *= gelu'(x) in place
 *   add3        out [n] = (m + a) + h
 *   rope        qkv [M][n_heads][q | k | v][64] in place: dims 0 .. 15 of q and k rotated by the handle's table at pos [M] (DEVICE int32, read back and checked
 *               against max_position_embeddings: synchronous up to the launch); sign +1 forward, -1 the inverse rotation
 *   embed       ids, cls [M] and attrs4 [4][M] (HOST int32, checked against V, NC, NB) -> A4 [M][4 E] = the four attribute rows side by side and
 *               h [M][H] = (word[ids] + cemb[cls]) + h_in (h may be h_in).  Synchronous.
 *   ce          logits [M][V] in place -> (softmax - onehot) * scale, zero rows where labels_host [M] is -100; row_loss [M] = lse - logit[label] (0 there).  Synchronous.
 *   colred      mode 0: g0 [N] += sum_r dy[r][c] over dy [M][N] with row stride ld >= N.  mode 1: also g1 [N] += sum_r dy[r][c] xhat[r][c], xhat from x [M][N]
 *               (row stride N), mean, rstd [M].  Any N >= 1.
 *   embed_grad  grad [n_rows][width] += per table row i != pad_row the sum of src[r][col0 .. col0 + width) (src [M][ld]) over the rows r with idx_host[r] == i, in
 *               ascending r: the engine's own grouping and launch; a batch with no such row launches nothing.  Synchronous.
 *   adamw       clip (g *= coef) and one AdamW step of p, g, m, v [n] at optimizer step `step` (1-based), the scalars formed from the doubles exactly as
 *               etd_dtrain_clip_and_step forms them; `norm` is the gradient norm the clipping coefficient is taken from
 *   sumsq       *norm = sqrt(sum g[i]^2) of g [n], the fp64 reduction both trainers' clip_and_step use.  Synchronous. */
int etd_debug_dtrain_ln(const float* x_dev, int M, int H, float eps, float* mean_dev, float* rstd_dev, const float* g1_dev, const float* b1_dev, float* y1_dev,
                        const float* g2_dev, const float* b2_dev, float* y2_dev, const float* dy_dev, float* dx_dev, void* stream);
int etd_debug_dtrain_gelu(const float* x_dev, long long n, float* y_dev, float* dy_dev, void* stream);
int etd_debug_dtrain_add3(const float* m_dev, const float* a_dev, const float* h_dev, long long n, float* out_dev, void* stream);
int etd_debug_dtrain_rope(etd_dtrain*, float* qkv_dev, int n_heads, int M, const int32_t* pos_dev, int sign, void* stream);
int etd_debug_dtrain_embed(int M, int H, int E, int V, int NC, int NB, const int32_t* ids_host, const int32_t* cls_host, const int32_t* attrs4_host,
                           const float* word_dev, const float* cemb_dev, const float* attr0_dev, const float* attr1_dev, const float* attr2_dev,
                           const float* attr3_dev, const float* h_in_dev, float* A4_dev, float* h_dev, void* stream);
int etd_debug_dtrain_ce(float* logits_dev, int M, int V, const int32_t* labels_host, float scale, float* row_loss_dev, void* stream);
int etd_debug_dtrain_colred(int mode, const float* dy_dev, int ld, int M, int N, const float* x_dev, const float* mean_dev, const float* rstd_dev, float* g0_dev,
                            float* g1_dev, void* stream);
int etd_debug_dtrain_embed_grad(const float* src_dev, int ld, int col0, int width, int M, const int32_t* idx_host, int n_rows, int pad_row, float* grad_dev,
                                void* stream);
int etd_debug_dtrain_adamw(float* p_dev, float* g_dev, float* m_dev, float* v_dev, long long n, double max_norm, double norm, double lr, double beta1, double beta2,
                           double eps, double weight_decay, long long step, void* stream);
int etd_debug_dtrain_sumsq(const float* g_dev, long long n, double* norm, void* stream);

/* test hook, HOST ONLY: the plan etd_render_run makes of a call, without a device: first_end_host int64 [notes][2] = per note the first sample it sounds on and the
 * first it no longer does; ranges_host int32 [blocks][2] = per block of 1 024 samples (cover after cover) the candidate notes [lo, hi) of its cover.  Either may be
 * NULL.  Refuses what etd_render_run refuses about the notes. */
int etd_render_debug_plan(etd_render*, const etd_note* notes_host, const int64_t* note_offsets_host, int n_covers, const int64_t* num_samples_host,
                          int64_t* first_end_host, int32_t* ranges_host);

/* test hooks of the separator (csrc/separator.hip): each stage of etd_sep_run on a caller's input, with the launchers etd_sep_run uses.  DEVICE fp32 buffers; a
 * complex number is two consecutive floats.  Asynchronous on `stream` once the handle's weights are on the device.
 *   stft    wav [n_channels][N] -> X [n_channels][Tf][n_fft / 2 + 1] complex, Tf = etd_sep_num_frames(N)
 *   layer   one U-Net layer of instrument `instr` on n_units inputs back to back.  kind 0: encoder l = layer (1 .. 6): x0 [T >> (l-1)][F >> (l-1)][Cin] ->
 *           pre [T >> l][F >> l][Cout] (conv + bias) and act = ELU(a pre + s) (either may be NULL).  kind 1: decoder j = layer: x0 = the skip (j = 1: conv_6),
 *           x1 = the previous decoder output (j = 1: NULL), both [T >> (7-j)][F >> (7-j)][.] -> act [T >> (6-j)][F >> (6-j)][Cout] = a ELU(deconv + bias) + s.
 *           kind 2: the head: x0 [T][F][1] -> pre [T][F][n_channels].
 *   mask    logits [segs][n_instr][T][F][n_channels], mag [segs * T][F][n_channels], X [n_channels][Tf][F] complex (segs = ceil(Tf / T)) ->
 *           Y [n_instr][n_channels][Tf][F] complex
 *   istft   Y [n_instr][n_channels][Tf][F] complex (bins >= F are zero), Tf = etd_sep_num_frames(N) -> out [n_instr][n_channels][N] */
int etd_sep_debug_stft(etd_sep*, const float* wav_dev, long long N, float* X_dev, void* stream);
int etd_sep_debug_layer(etd_sep*, int instr, int kind, int layer, const float* x0_dev, const float* x1_dev, int n_units, float* pre_dev, float* act_dev, void* stream);
int etd_sep_debug_mask(etd_sep*, const float* logits_dev, const float* mag_dev, const float* X_dev, long long Tf, float* Y_dev, void* stream);
int etd_sep_debug_istft(etd_sep*, const float* Y_dev, long long N, float* out_dev, void* stream);
/*   mwf     the Wiener stage of etd_sep_set_mwf on a tapped input, by the launcher etd_sep_run uses: X [n_channels][Tf][F] complex, Y [n_instr][n_channels][Tf][F]
 *           complex, refined IN PLACE by `iterations` (0 .. 8; 0 leaves Y untouched) passes.  Synchronises `stream` when the workspace grows. */
int etd_sep_debug_mwf(etd_sep*, const float* X_dev, float* Y_dev, long long Tf, int iterations, void* stream);

/* stage taps of separator training (csrc/separator_train.hip): each backward kernel on a caller's input, with the launchers etd_septrain_forward_backward uses.
 * DEVICE fp32; every tensor holds B x n_instr units back to back, unit u = b * n_instr + instrument, each with its instrument's weights.
 *   dx    kind 0: encoder layer l (2 .. 6): dy [T >> l][F >> l][Cout] -> out0 [T >> (l-1)][F >> (l-1)][Cin].  kind 1: decoder j: dy [2H][2W][Cout] (H = T >> (7-j))
 *         -> out0 = the skip's gradient [H][W][C skip], out1 = the gradient of decoder j - 1's output [H][W][..] (j > 1).  kind 2: the head: dy [T][F][C] -> [T][F][1]
 *   dw    the weight gradient of encoder `layer` (x0 = its input; layer 1: [B] units, shared by the instruments), decoder `layer` (x0 = skip, x1 = up, dy = the
 *         gradient of the transposed convolution's output) or the head, ADDED to dw [n_instr][the state tensor's shape]
 *   norm  norm n (1 .. 12) on x: the batch statistics, y = the normalised output (encoder: ELU(norm(x)); decoder: norm(ELU(x))), stats (may be NULL) = [mean | biased
 *         variance], [n_instr][C] each; with dy: dx = the gradient at x, and gamma's / beta's gradients are ADDED to the handle's.  Moves no running statistic.
 *   loss  logits [B][n_instr][T][F][C], mix [B][..], target [n_instr][B][..] -> *loss and dlogits = loss_scale x the gradient.  Synchronous. */
int etd_septrain_debug_dx(etd_septrain*, int kind, int layer, const float* dy_dev, int B, float* out0_dev, float* out1_dev, void* stream);
int etd_septrain_debug_dw(etd_septrain*, int kind, int layer, const float* x0_dev, const float* x1_dev, const float* dy_dev, int B, float* dw_dev, void* stream);
int etd_septrain_debug_norm(etd_septrain*, int norm, const float* x_dev, int B, const float* dy_dev, float* y_dev, float* dx_dev, float* stats_dev, void* stream);
int etd_septrain_debug_loss(etd_septrain*, const float* logits_dev, const float* mix_dev, const float* target_dev, int B, double loss_scale, double* loss,
                            float* dlogits_dev, void* stream);
/* the dropout mask of decoder level j (1 .. 3) at call counter `call`, with the handle's p and seed: out = keep ? y * s : 0 over the first numel elements of
 * y [B][n_instr][pos][C] (numel = 0: all of them; a count that is no multiple of 4 ends inside a Philox block).  out may be y.  Moves no counter. */
int etd_septrain_debug_dropout(etd_septrain*, int j, const float* y_dev, int B, long long numel, long long call, float* out_dev, void* stream);

/* stage taps of BSS Eval (csrc/bss.hip), each stage on a caller's input with the launchers etd_bss_run uses.  DEVICE buffers; fp64 unless said.
 *   corr     ref, est [J][C][N] fp32 -> r [S][S][L] (r[p][q][l] = sum_n x_p[n] x_q[n + l]) and d [S][S][L] (d[p][e][l] = sum_n x_p[n] y_e[n + l]), S = J C
 *   solve    a caller's SPD matrix G [n][n] (n <= 8192; not changed) and right-hand sides [n][m] (m <= 16) -> x [n][m] and *status (1 = a pivot <= 0 or not finite)
 *   filters  ref, est -> A [S L][S] and B [J][C L][C]
 *   project  ref, window `window_index` of the track and a caller's A, B -> ps [J][C][Wout], pa [J][C][Wout], Wout = the window's length + L - 1
 *   timing   on != 0: the following etd_bss_run calls time their stages with events; stage_ms5 (may be NULL) receives the last run's milliseconds of the
 *            correlations, the factorisations, the substitutions, the projections and the energies */
int etd_bss_debug_corr(etd_bss*, const float* ref_dev, const float* est_dev, int J, int C, long long N, double* r_dev, double* d_dev, void* stream);
int etd_bss_debug_solve(etd_bss*, const double* G_dev, const double* rhs_dev, int n, int m, double* x_dev, int32_t* status_dev, void* stream);
int etd_bss_debug_filters(etd_bss*, const float* ref_dev, const float* est_dev, int J, int C, long long N, double* A_dev, double* B_dev, int32_t* status_dev, void* stream);
int etd_bss_debug_project(etd_bss*, const float* ref_dev, int J, int C, long long N, int window_index, const double* A_dev, const double* B_dev, double* ps_dev,
                          double* pa_dev, void* stream);
int etd_bss_debug_timing(etd_bss*, int on, double* stage_ms5);

/* stage taps of the Beat-Transformer trainer (csrc/beat_train.hip): every kernel and host pipeline on a caller's DEVICE inputs, through the launchers
 * etd_btrain_loss_backward uses.  Songs are given as for etd_beat_forward (T_host [n_seq], rows = instr x frames, at most 2^17).  Malformed arguments are ETD_EINVAL
 * before the device is touched.
 *   dattn      dilated attention of time layer `layer`: qkv [rows][768], Er [8][32][5], xin [rows][256] -> prob [rows][8][5], skip [rows][256], xout = xin + skip; with
 *              dO [rows][256] also dl [rows][8][5], dqkv [rows][768] (every column written; head 7's key columns zeros), and dEr [8][32][5] += the two-level row sum
 *              (part: scratch of ceil(rows / 64) x 1280 floats)
 *   iattn      instrument attention: qkv [rows][768] -> ao [rows][256]; with dao also dqkv [rows][768]
 *   fold2      conv2's input gradient: dpatch [rows 24][384], c1 [rows][42][32] -> dc1 [rows][42][32]
 *   conv1_bwd  conv1's dw [32][15] += and db [32] += from feat [rows][128] and dc1 [rows][42][32] (part: scratch of ceil(rows / 16) x 512 floats)
 *   bce        z, y [frames][ntoken], pos_weight, coef [ntoken] -> cell, dz [frames][ntoken]
 *   tempo_ce   t, p [n][300], has [n] int32 -> row [n], dt [n][300]
 *   front_fwd  which 0: conv1 + pool + ReLU, in = feat [rows][128], w [32][15], b [32] -> out = c1 [rows][42][32]; 1: conv2's patches, in = c1 -> x2 [rows 24][384];
 *              2: conv3's patches through pool2 + ReLU, in = c2 [rows][24][64] -> x3 [rows 3][1152]; 3: pool3 + ReLU, in = c3 [rows][3][256] -> x [rows][256]
 *              (w, b are read by which 0 only)
 *   front_bwd  which 0: c = c3, g = dx [rows][256] -> dc3 [rows][3][256]; 1: c = c2, g = dx3 [rows 3][1152] -> dc2 [rows][24][64] (every float written)
 *   repack     k_bt_repack on native [co][ci][kk] and packed [co][kk][ci]: dir 0 packed = native, dir 1 native += packed
 *   colsum     out [N] += the column sums of dy [M][N] (row stride ld >= N): slices of 256 rows, then slice_sum (part: scratch of ceil(M / 256) x N floats)
 *   slice_sum  out [width] += the sum of part [n_slices][width] over the slices: 16 at a time in order, then the groups in order
 *   means      which 0: skipacc, a = skip [rows][256] -> out = tacc [frames][256] (first_layer 1: overwritten, 0: added to); 1: dskip, a = dx [rows][256],
 *              b = dtf [frames][256] -> dsk [rows][256]; 2: hmean, a = x [rows][256] -> hm [frames][256]; 3: hmean_bwd, a = x, b = dhm [frames][256] -> dx [rows][256];
 *              4: tmean, a = tacc [frames][256] -> tm [n_seq][256]; 5: tmean_bwd, a = tacc, b = dtm [n_seq][256] -> dtf [frames][256]
 *   relu       x [n] -> y = max(x, 0) (y may be NULL); then dy = x > 0 ? dy : 0 in place (dy may be NULL)
 *   conv_wgrad dw [M][N] = dY^T X over K rows (dY [K][M], X [K][N]) in segments of 4 096 rows, then slice_sum; dw is overwritten (seg: scratch of
 *              ceil(K / 4096) x M x N floats)
 *   ffn_bwd    one feed-forward sublayer's backward (act 0 GELU, 1 ReLU) over R <= max_rows rows on the handle's scratch, with the handle's d_hid = H: x [R][256], its
 *              LayerNorm statistics mean, rstd [R], pre = W1 LN(x) + b1 [R][H], P = gain [256] | bias [256] | linear1.weight [H][256] | linear1.bias [H] |
 *              linear2.weight [256][H] | linear2.bias [256]; dx [R][256] holds the gradient of the sublayer's output on entry and of x on exit; the six parameter
 *              gradients are ADDED to G (P's layout).  The handle's parameters, accumulated gradients and moments are neither read nor written.
 *   proj_bwd   a fused q | k | v projection's backward from dqkv [R][768]: P = gain [256] | bias [256] | weight [768][256] | bias [768]; dx [R][256] += the gradient of
 *              x, G (P's layout) += the parameter gradients; the key third of the bias gradient is not touched.  The handle as for ffn_bwd.
 *   read_rows  per-row results of the handle's last etd_btrain_loss_backward, to the HOST: what 0 = the gradient of the front end's tokens [rows][256], 1 = the logits
 *              [frames][ntoken], 2 = the gradient of conv1's pooled output [rows][42][32].  Synchronous. */
int etd_debug_btrain_dattn(int n_seq, const int64_t* T_host, int instr, int layer, const float* qkv_dev, const float* Er_dev, const float* xin_dev, const float* dO_dev,
                           float* prob_dev, float* skip_dev, float* xout_dev, float* dl_dev, float* dqkv_dev, float* part_dev, float* dEr_dev, void* stream);
int etd_debug_btrain_iattn(int n_seq, const int64_t* T_host, int instr, const float* qkv_dev, const float* dao_dev, float* ao_dev, float* dqkv_dev, void* stream);
int etd_debug_btrain_fold2(int rows, const float* dpatch_dev, const float* c1_dev, float* dc1_dev, void* stream);
int etd_debug_btrain_conv1_bwd(int n_seq, const int64_t* T_host, int instr, const float* feat_dev, const float* dc1_dev, const float* w_dev, const float* b_dev,
                               float* part_dev, float* dw_dev, float* db_dev, void* stream);
int etd_debug_btrain_bce(const float* z_dev, const float* y_dev, const float* pos_weight_dev, const float* coef_dev, int frames, int ntoken, float* cell_dev, float* dz_dev,
                         void* stream);
int etd_debug_btrain_tempo_ce(const float* t_dev, const float* p_dev, const int32_t* has_dev, float coef, int n, float* row_dev, float* dt_dev, void* stream);
int etd_debug_btrain_read_rows(etd_btrain*, int what, float* out_host, long long numel, void* stream);
int etd_debug_btrain_front_fwd(int which, int n_seq, const int64_t* T_host, int instr, const float* in_dev, const float* w_dev, const float* b_dev, float* out_dev,
                               void* stream);
int etd_debug_btrain_front_bwd(int which, int n_seq, const int64_t* T_host, int instr, const float* c_dev, const float* g_dev, float* out_dev, void* stream);
int etd_debug_btrain_repack(int dir, int co, int ci, int kk, float* native_dev, float* packed_dev, void* stream);
int etd_debug_btrain_colsum(const float* dy_dev, int ld, int M, int N, float* part_dev, float* out_dev, void* stream);
int etd_debug_btrain_slice_sum(const float* part_dev, int n_slices, int width, float* out_dev, void* stream);
int etd_debug_btrain_means(int which, int n_seq, const int64_t* T_host, int instr, const float* a_dev, const float* b_dev, int first_layer, float* out_dev, void* stream);
int etd_debug_btrain_relu(const float* x_dev, long long n, float* y_dev, float* dy_dev, void* stream);
int etd_debug_btrain_conv_wgrad(int M, int N, int K, const float* dY_dev, const float* X_dev, float* seg_dev, float* dw_dev, void* stream);
int etd_debug_btrain_ffn_bwd(etd_btrain*, int R, int act, const float* x_dev, const float* mean_dev, const float* rstd_dev, const float* pre_dev, const float* P_dev,
                             float* G_dev, float* dx_dev, void* stream);
int etd_debug_btrain_proj_bwd(etd_btrain*, int R, const float* x_dev, const float* mean_dev, const float* rstd_dev, const float* dqkv_dev, const float* P_dev, float* G_dev,
                              float* dx_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
