// Training engine of the Beat-Transformer (etd_btrain_*): the model of beat.hip with saved activations, this project's beat / tempo loss, the backward pass for
// every parameter, global-norm clipping and AdamW, all in fp32.  Dense products are launch_tgemm of dec_train.h; LayerNorm, GELU, the column
// reductions, the gradient norm and the AdamW update are the decoder trainer's kernels.  These are the launchers of the kernels that are new here; the ones with a
// slice or tap edge are also reachable on their own through include/etude_hip_debug.h.
// Nothing here uses a floating-point atomic: every sum runs in an order fixed by the shapes alone.
#pragma once
#include "beat.h"
#include "dec_train.h"

#define BT_C2_COLS 24         // conv2 columns the model reads (8 pooled columns x 3); the patches and conv2's output are [row][24][.]
#define BT_C1_ROWS 16         // rows per slice of the conv1 weight reduction
#define BT_ER_ROWS 64         // rows per slice of the dEr reduction
#define BT_SEG_ROWS 4096      // rows per segment of a conv layer's weight-gradient reduction
#define BT_CS_ROWS 256        // rows per slice of a bias gradient's column sum
#define BT_TEMPO 300

// the songs of a call: global row / frame offsets [n + 1] on the device
struct BtSongs { const int* row0; const int* frame0; int n, rows, frames, instr; };

// dilated attention of time layer `layer` (dilation 2^layer).  forward: prob [rows][8][5], skip [rows][256], xout = xin + skip
int launch_bt_dattn_fwd(const float* qkv, const BtSongs& S, const float* Er, int dil, const float* xin, float* prob, float* skip, float* xout, hipStream_t st);
// backward from dO [rows][256] (the gradient of skip): dl [rows][8][5] (the logits' gradient), dqkv [rows][768] complete (head 7's key columns are zeros),
// dEr[8][32][5] += the two-level sum over rows (part: [ceil(rows / BT_ER_ROWS)][1280] scratch)
int launch_bt_dattn_bwd(const float* qkv, const float* prob, const float* dO, const BtSongs& S, const float* Er, int dil, float* dl, float* dqkv, float* part,
                        float* dEr, hipStream_t st);
// instrument attention over the instr rows of each frame, one thread per (frame, head)
int launch_bt_iattn_fwd(const float* qkv, const BtSongs& S, float* ao, hipStream_t st);
int launch_bt_iattn_bwd(const float* qkv, const float* dao, const BtSongs& S, float* dqkv, hipStream_t st);
// conv2's input gradient: dc1[r][p][ci] = (c1 > 0) sum_{kw ascending, 0 <= p - kw < 24} dpatch[r 24 + p - kw][kw 32 + ci]
int launch_bt_fold2(const float* dpatch, const float* c1, int rows, float* dc1, hipStream_t st);
// conv1's weight and bias gradient from dc1 (already masked by the ReLU): slices of BT_C1_ROWS rows (part: [slices][32][16] scratch), then an ordered sum; dw [32][15], db [32] +=
int launch_bt_conv1_bwd(const float* feat, const float* dc1, const BtSongs& S, const float* w, const float* b, float* part, float* dw, float* db, hipStream_t st);
// beat loss: cell [frames][ntoken] = w_c(y) bce_with_logits(z, y) (0 where y = -1), dz = coef[c] w_c(y) (sigmoid(z) - y)
int launch_bt_bce(const float* z, const float* y, const float* pos_weight, const float* coef, int frames, int ntoken, float* cell, float* dz, hipStream_t st);
// tempo loss: row[s] = -sum_k p_k log_softmax(t)_k (0 where has[s] = 0), dt = coef (softmax(t) sum_k p_k - p)
int launch_bt_tempo_ce(const float* t, const float* p, const int* has, float coef, int n, int n_out, float* row, float* dt, hipStream_t st);
// out[c] += sum over the M rows of dy[r][c] (row stride ld), c < N: slices of BT_CS_ROWS rows, then an ordered sum (part: [ceil(M / BT_CS_ROWS)][N] scratch)
int launch_bt_colsum(const float* dy, int ld, int M, int N, float* part, float* out, hipStream_t st);
