// Training engine of the Beat-Transformer (etd_btrain_*): saved activations, this project's beat / tempo loss, the backward pass for every parameter, global-norm
// clipping and AdamW, all in fp32.  The forward's conv1, conv3 patches, pool3, dilated attention, skip accumulation and instrument attention are the
// inference engine's kernels (beat.h: launch_beat_*), on the engine's song table (BeatChunk, one chunk per call).  Dense products, LayerNorm, GELU, the column reductions,
// the gradient norm and the AdamW update are the trainers' shared kernels (train_kernels.h).  These are the launchers of the kernels that are new here; every one is
// also reachable on its own through include/etude_hip_debug.h (etd_debug_btrain_*: dattn, iattn, fold2, conv1_bwd, bce, tempo_ce, front_fwd, front_bwd, repack, colsum,
// slice_sum, means, relu, conv_wgrad, and the two host pipelines ffn_bwd and proj_bwd on a handle's scratch).
// Nothing here uses a floating-point atomic: every sum runs in an order fixed by the shapes alone.
#pragma once
#include "beat.h"
#include "train_kernels.h"

#define BT_C1_ROWS 16         // rows per slice of the conv1 weight reduction
#define BT_ER_ROWS 64         // rows per slice of the dEr reduction
#define BT_SEG_ROWS 4096      // rows per segment of a conv layer's weight-gradient reduction
#define BT_CS_ROWS 256        // rows per slice of a bias gradient's column sum
#define BT_TEMPO 300

// dilated attention of time layer `layer` (dilation 2^layer; forward: launch_beat_dattn_train), backward from dO [rows][256] (the gradient of skip): dl [rows][8][5] (the logits' gradient), dqkv [rows][768] complete (head 7's key columns are zeros),
// dEr[8][32][5] += the two-level sum over rows (part: [ceil(rows / BT_ER_ROWS)][1280] scratch)
int launch_bt_dattn_bwd(const float* qkv, const float* prob, const float* dO, const BeatChunk& S, const float* Er, int dil, float* dl, float* dqkv, float* part,
                        float* dEr, hipStream_t st);
// instrument attention over the instr rows of each frame (forward: launch_beat_iattn), backward: one thread per (frame, head)
int launch_bt_iattn_bwd(const float* qkv, const float* dao, const BeatChunk& S, float* dqkv, hipStream_t st);
// conv2's input gradient: dc1[r][p][ci] = (c1 > 0) sum_{kw ascending, 0 <= p - kw < 24} dpatch[r 24 + p - kw][kw 32 + ci]
int launch_bt_fold2(const float* dpatch, const float* c1, int rows, float* dc1, hipStream_t st);
// conv1's weight and bias gradient from dc1 (already masked by the ReLU): slices of BT_C1_ROWS rows (part: [slices][32][16] scratch), then an ordered sum; dw [32][15], db [32] +=
int launch_bt_conv1_bwd(const float* feat, const float* dc1, const BeatChunk& S, const float* w, const float* b, float* part, float* dw, float* db, hipStream_t st);
// beat loss: cell [frames][ntoken] = w_c(y) bce_with_logits(z, y) (0 where y = -1), dz = coef[c] w_c(y) (sigmoid(z) - y)
int launch_bt_bce(const float* z, const float* y, const float* pos_weight, const float* coef, int frames, int ntoken, float* cell, float* dz, hipStream_t st);
// tempo loss: row[s] = -sum_k p_k log_softmax(t)_k (0 where has[s] = 0), dt = coef (softmax(t) sum_k p_k - p)
int launch_bt_tempo_ce(const float* t, const float* p, const int* has, float coef, int n, int n_out, float* row, float* dt, hipStream_t st);
// out[c] += sum over the M rows of dy[r][c] (row stride ld), c < N: slices of BT_CS_ROWS rows, then an ordered sum (part: [ceil(M / BT_CS_ROWS)][N] scratch)
int launch_bt_colsum(const float* dy, int ld, int M, int N, float* part, float* out, hipStream_t st);
// ---- the conv front end (conv1, conv3's patches and pool3: launch_beat_*).  conv2's patches: c1 [rows][42][32] -> x2 [rows 24][384]
int launch_bt_patch2(const float* c1, int rows, float* x2, hipStream_t st);
// a conv weight between the state dict's [co][ci][kk] and the GEMM's [co][kk][ci].  dir 0: packed = native; dir 1: native += packed
int launch_bt_repack(float* native, float* packed, int co_n, int ci_n, int kk_n, int dir, hipStream_t st);
// through pool + ReLU: the gradient goes to the first maximal entry of a triple, nowhere when the maximum is not positive.  patch3_bwd first gathers dx3 [rows 3][1152]
// per pooled cell (kt ascending, then c ascending)
int launch_bt_pool3_bwd(const float* c3, const float* dx, int rows, float* dc3, hipStream_t st);
int launch_bt_patch3_bwd(const float* c2, const float* dx3, const BeatChunk& S, float* dc2, hipStream_t st);
// out[e] += sum over the slices, 16 at a time in order, then the groups in order, of part[slice][e], e < width
int launch_bt_slice_sum(const float* part, int n_slices, int width, float* out, hipStream_t st);
// dw [M][N] = dY^T X over K rows (dY [K][M], X [K][N]) in segments of BT_SEG_ROWS rows (seg: [ceil(K / BT_SEG_ROWS)][M][N] scratch), then the ordered sum; dw is overwritten
int launch_bt_conv_wgrad(int M, int N, int K, const float* dY, const float* X, float* seg, float* dw, hipStream_t st);
// the instrument means and the tempo mean with their backward passes (frames are (song, t); see the kernels; the skip mean itself is launch_beat_skipacc)
int launch_bt_dskip(const float* dx, const float* dtf, const BeatChunk& S, float* dsk, hipStream_t st);
int launch_bt_hmean(const float* x, const BeatChunk& S, float* hm, hipStream_t st);
int launch_bt_hmean_bwd(const float* x, const float* dhm, const BeatChunk& S, float* dx, hipStream_t st);
int launch_bt_tmean(const float* tacc, const BeatChunk& S, float* tm, hipStream_t st);
int launch_bt_tmean_bwd(const float* tacc, const float* dtm, const BeatChunk& S, float* dtf, hipStream_t st);
int launch_bt_relu(const float* x, float* y, long long n, hipStream_t st);
int launch_bt_relu_bwd(const float* x, float* dy, long long n, hipStream_t st);      // dy = x > 0 ? dy : 0
