// Training engine of the Beat-Transformer (beat_train.h): Demixed_DilatedTransformerModel in eval arithmetic (no dropout) with saved activations, this
// project's beat / tempo loss, the backward pass for every parameter, gradient accumulation, clip_grad_norm_ and AdamW.
//
// The non-GEMM forward stages are the inference engine's kernels, launched through beat.h: k_beat_conv1, k_beat_patch3 (its 24-column instance), k_beat_pool3,
// k_beat_dattn (its instance that keeps the probabilities and writes out of place), k_beat_skipacc and k_beat_iattn.  Forward kernels of this file: k_bt_patch2
// (conv2's explicit patches; the engine's GEMM reads overlapping rows instead), k_bt_hmean and k_bt_tmean (the heads' means, which feed launch_tgemm; the engine fuses
// them with its GEMVs) and k_bt_relu.  Everything else here is loss and backward.  The song table is the engine's BeatChunk, one chunk for the whole call
// (beat_whole_call: its rows must fit the workspace sized at create), and the backward kernels locate rows, load, dot and recompute conv1 with beat.h's helpers.
// Rows are (song, instr, t) as in beat.hip: song s owns rows [row0_s, row0_s + instr T_s) laid out [instr][T_s]; frames are (song, t).
// Arithmetic: fp32 operands and accumulation.  Every dense product (the linear layers, conv2 and conv3 on explicit patches, the two heads) is launch_tgemm of
// train_kernels.h in its forward, input-gradient and weight-gradient form.  No floating-point atomics: a kernel either owns its output element and adds its terms in an
// order fixed by the shapes (taps ascending, kw ascending, instruments ascending), or reduces over rows in fixed slices followed by an ordered sum.  Every gradient
// is formed for the call and then added once to the accumulated one.
#include "beat_train.h"

#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "etude_hip.h"
#include "etude_hip_debug.h"
#include "train_store.h"

// ================================================================================================ conv front end, forward
// conv2's patches: x2[r 24 + col][kw 32 + ci] = c1[r][col + kw][ci], the 384 floats from (r 42 + col) 32 on
__global__ __launch_bounds__(256) void k_bt_patch2(const float* __restrict__ c1, int rows, float* __restrict__ x2) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * BEAT_C2_COLS * BEAT_K2) return;
  const long long rc = gid / BEAT_K2;
  const int k = (int)(gid - rc * BEAT_K2);
  const long long r = rc / BEAT_C2_COLS;
  const int col = (int)(rc - r * BEAT_C2_COLS);
  x2[gid] = c1[(r * BEAT_W1 + col) * BEAT_C1 + k];
}
// a conv weight between the state dict's [co][ci][kk] and the GEMM's [co][kk][ci].  dir 0: packed = native; dir 1: native += packed (a gradient)
__global__ __launch_bounds__(256) void k_bt_repack(float* __restrict__ native, float* __restrict__ packed, int co_n, int ci_n, int kk_n, int dir) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)co_n * ci_n * kk_n) return;
  const int co = (int)(gid / (ci_n * kk_n)), rem = (int)(gid - (long long)co * ci_n * kk_n), ci = rem / kk_n, kk = rem - ci * kk_n;
  const long long pk = ((long long)co * kk_n + kk) * ci_n + ci;
  if (dir == 0) packed[pk] = native[gid];
  else native[gid] += packed[pk];
}

// ================================================================================================ conv front end, backward
// max-pool over 3 + ReLU: the gradient goes to the first maximal entry, and nowhere when the maximum is not positive
__device__ __forceinline__ void bt_pool_route(float v0, float v1, float v2, float g, float& g0, float& g1, float& g2) {
  const float m = fmaxf(fmaxf(v0, v1), v2);
  g0 = g1 = g2 = 0.f;
  if (!(m > 0.f)) return;
  if (v0 == m) g0 = g; else if (v1 == m) g1 = g; else g2 = g;
}
__global__ __launch_bounds__(256) void k_bt_pool3_bwd(const float* __restrict__ c3, const float* __restrict__ dx, int rows, float* __restrict__ dc3) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * BEAT_DMODEL) return;
  const long long r = gid >> 8;
  const int co = (int)(gid & 255);
  const long long o = r * 3 * BEAT_DMODEL + co;
  float g0, g1, g2;
  bt_pool_route(c3[o], c3[o + BEAT_DMODEL], c3[o + 2 * BEAT_DMODEL], dx[gid], g0, g1, g2);
  dc3[o] = g0; dc3[o + BEAT_DMODEL] = g1; dc3[o + 2 * BEAT_DMODEL] = g2;
}
// conv3's patch gradient gathered back through pool2 + ReLU into conv2's output gradient: the pooled cell (r, pc, ci) is read by the patches (r - kt + 1, c, kw = pc - c);
// its terms are added kt ascending, then c ascending.  One thread per (row, pooled column < 8, ci), writing the cell's three conv2 columns.
__global__ __launch_bounds__(256) void k_bt_patch3_bwd(const float* __restrict__ c2, const float* __restrict__ dx3, BeatChunk S, float* __restrict__ dc2) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.rows * 8 * BEAT_C2) return;
  const int r = (int)(gid / (8 * BEAT_C2)), rem = (int)(gid - (long long)r * 8 * BEAT_C2), pc = rem / BEAT_C2, ci = rem - pc * BEAT_C2;
  int s, T, t;
  beat_row_at(S, r, s, T, t);
  float g = 0.f;
  for (int kt = 0; kt < 3; ++kt) {
    const int tq = t - kt + 1;
    if (tq < 0 || tq >= T) continue;
    for (int c = 0; c < 3; ++c) {
      const int kw = pc - c;
      if (kw < 0 || kw >= 6) continue;
      g += dx3[((long long)(r - kt + 1) * 3 + c) * BEAT_K3 + kt * 384 + kw * 64 + ci];
    }
  }
  const long long o = ((long long)r * BEAT_C2_COLS + 3 * pc) * BEAT_C2 + ci;
  float g0, g1, g2;
  bt_pool_route(c2[o], c2[o + BEAT_C2], c2[o + 2 * BEAT_C2], g, g0, g1, g2);
  dc2[o] = g0; dc2[o + BEAT_C2] = g1; dc2[o + 2 * BEAT_C2] = g2;
}
__global__ __launch_bounds__(256) void k_bt_fold2(const float* __restrict__ dpatch, const float* __restrict__ c1, int rows, float* __restrict__ dc1) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * BEAT_W1 * BEAT_C1) return;
  const long long r = gid / (BEAT_W1 * BEAT_C1);
  const int rem = (int)(gid - r * (BEAT_W1 * BEAT_C1)), p = rem / BEAT_C1, ci = rem - p * BEAT_C1;
  float g = 0.f;
  for (int kw = 0; kw < 12; ++kw) {
    const int col = p - kw;
    if (col < 0 || col >= BEAT_C2_COLS) continue;
    g += dpatch[(r * BEAT_C2_COLS + col) * BEAT_K2 + kw * BEAT_C1 + ci];
  }
  dc1[gid] = c1[gid] > 0.f ? g : 0.f;
}
// conv1 dW / db, level 1: workgroup = one slice of BT_C1_ROWS rows; thread = (co, one of 8 sub-slices of the slice's (row, p) cells, taken every 8th in ascending order);
// the 8 sub-slices are added in order.  part[slice][co][16]: 15 weights + the bias.
__global__ __launch_bounds__(256) void k_bt_conv1_bwd(const float* __restrict__ feat, const float* __restrict__ dc1, BeatChunk S, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ part) {
  __shared__ float ps[8][32][17];
  const int tid = threadIdx.x, co = tid & 31, sub = tid >> 5;
  const long long r0 = (long long)blockIdx.x * BT_C1_ROWS;
  const int nr = (int)(S.rows - r0 < BT_C1_ROWS ? S.rows - r0 : BT_C1_ROWS);
  float wr[15], acc[16];
#pragma unroll
  for (int k = 0; k < 15; ++k) wr[k] = w[co * 15 + k];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.f;
  const float bc = b[co];
  for (int idx = sub; idx < nr * BEAT_W1; idx += 8) {
    const int r = (int)r0 + idx / BEAT_W1, p = idx % BEAT_W1;
    const float dm = dc1[((long long)r * BEAT_W1 + p) * BEAT_C1 + co];
    if (dm == 0.f) continue;                           // (adds exact zeros)
    int s, T, t;
  beat_row_at(S, r, s, T, t);
    float m = -INFINITY;
    int um = 0;
#pragma unroll 1
    for (int u = 0; u < 3; ++u) {
      const float v = beat_conv1_at(feat, r, t, T, p, u, wr, bc);      // the chain k_beat_conv1 runs: the maximum the forward took
      if (v > m) { m = v; um = u; }                    // strict: the first maximal column
    }
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      const int tt = t + kt - 2;
      if (tt < 0 || tt >= T) continue;
      const float* xr = feat + ((long long)r + kt - 2) * BEAT_MELS + 3 * p + um;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc[kt * 3 + kw] = fmaf(dm, xr[kw], acc[kt * 3 + kw]);
    }
    acc[15] += dm;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) ps[sub][co][k] = acc[k];
  __syncthreads();
  if (sub == 0) {
    for (int k = 0; k < 16; ++k) {
      float tot = ps[0][co][k];
      for (int q = 1; q < 8; ++q) tot += ps[q][co][k];
      part[((long long)blockIdx.x * 32 + co) * 16 + k] = tot;
    }
  }
}
// level 2 of a sliced reduction: out[e] += sum over slices, in slice order (16 at a time, then the groups in order), of part[slice][e]; remap != 0 is conv1's [co][16] -> dw [co][15] (out) and db [co] (out2)
__global__ __launch_bounds__(256) void k_bt_slice_sum(const float* __restrict__ part, int n_slices, int width, int n_out, float* __restrict__ out, float* __restrict__ out2, int remap) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out) return;
  float tot = 0.f;
  for (int q0 = 0; q0 < n_slices; q0 += 16) {          // groups of 16 slices, then the groups: two short chains instead of one of n_slices terms
    const int q1 = q0 + 16 < n_slices ? q0 + 16 : n_slices;
    float grp = 0.f;
    for (int q = q0; q < q1; ++q) grp += part[(long long)q * width + e];
    tot += grp;
  }
  if (!remap) { out[e] += tot; return; }
  const int co = e >> 4, k = e & 15;
  if (k < 15) out[co * 15 + k] += tot; else out2[co] += tot;
}

// Column sums over the batch rows (a bias gradient), level 1: workgroup = 32 columns x one slice of BT_CS_ROWS rows; thread = (column, one of 8 sub-slices taking every
// 8th row in ascending order); the 8 partial sums are added in order.  Level 2 is k_bt_slice_sum.  (train_kernels.hip's k_tcolred runs 8 chains over ALL rows: at 5 150 rows
// its chains of 644 terms missed the bound of DESIGN.md 4s on four biases by ratios of 4.1 .. 5.2.)
__global__ __launch_bounds__(256) void k_bt_colsum_part(const float* __restrict__ dy, int ld, int M, int N, float* __restrict__ part) {
  __shared__ float ps[8][32];
  const int t = threadIdx.x, c = blockIdx.x * 32 + (t & 31), sub = t >> 5;
  const long long r0 = (long long)blockIdx.y * BT_CS_ROWS, r1 = r0 + BT_CS_ROWS < M ? r0 + BT_CS_ROWS : M;
  float a = 0.f;
  if (c < N)
    for (long long r = r0 + sub; r < r1; r += 8) a += dy[r * ld + c];
  ps[sub][t & 31] = a;
  __syncthreads();
  if (sub == 0 && c < N) {
    float tot = ps[0][t];
    for (int k = 1; k < 8; ++k) tot += ps[k][t];
    part[(long long)blockIdx.y * N + c] = tot;
  }
}

// ================================================================================================ dilated 5-tap attention
// backward, query side: dl[r][h][j] = p_j (dO . v_j - sum_i p_i dO . v_i) / sqrt(32), dq = sum_j dl_j (k_j + Er[h][:, j]), taps ascending
__global__ __launch_bounds__(256) void k_bt_dattn_dq(const float* __restrict__ qkv, const float* __restrict__ prob, const float* __restrict__ dO, BeatChunk S,
                                                     const float* __restrict__ Er, int dil, float* __restrict__ dl, float* __restrict__ dqkv) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.rows * BEAT_HEADS) return;
  const int r = (int)(gid >> 3), h = (int)(gid & 7), kh = h == 7 ? 6 : h;
  int s, T, t;
  beat_row_at(S, r, s, T, t);
  float go[32];
  beat_load32(go, dO + (long long)r * BEAT_DMODEL + h * 32);
  float p[BEAT_TAPS], dp[BEAT_TAPS];
  bool ok[BEAT_TAPS];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) {
    const long long o = (long long)beat_tap_off(h, j) * dil, tt = t + o;
    ok[j] = tt >= 0 && tt < T;
    p[j] = prob[gid * BEAT_TAPS + j];
    dp[j] = ok[j] ? beat_dot32(go, qkv + (r + o) * 768 + 512 + h * 32) : 0.f;
    sum = fmaf(p[j], dp[j], sum);
  }
  float dq[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) dq[d] = 0.f;
  const float* er = Er + h * 32 * BEAT_TAPS;
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) {
    const float g = ok[j] ? p[j] * (dp[j] - sum) / BEAT_SCALE : 0.f;
    dl[gid * BEAT_TAPS + j] = g;
    if (!ok[j]) continue;
    const float* kp = qkv + (r + (long long)beat_tap_off(h, j) * dil) * 768 + 256 + kh * 32;
#pragma unroll
    for (int d = 0; d < 32; ++d) dq[d] = fmaf(g, kp[d] + er[d * BEAT_TAPS + j], dq[d]);
  }
  beat_store32(dqkv + (long long)r * 768 + h * 32, dq);
}
// backward, key side: one thread per (key row, head).  dv = sum over the taps j (ascending) whose query row r - o_h(j) dil lies in the song of p_j dO; dk likewise of dl_j q,
// key head 6 first from query head 6 and then from query head 7 (which reads head 6's keys); key head 7 is read by no query: exact zeros
__global__ __launch_bounds__(256) void k_bt_dattn_dkv(const float* __restrict__ qkv, const float* __restrict__ prob, const float* __restrict__ dl,
                                                      const float* __restrict__ dO, BeatChunk S, int dil, float* __restrict__ dqkv) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.rows * BEAT_HEADS) return;
  const int r = (int)(gid >> 3), h = (int)(gid & 7);
  int s, T, t;
  beat_row_at(S, r, s, T, t);
  float dk[32], dv[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) {
    const long long o = (long long)beat_tap_off(h, j) * dil, tq = t - o;
    if (tq < 0 || tq >= T) continue;
    const long long rq = r - o;
    beat_axpy32(dv, prob[(rq * 8 + h) * BEAT_TAPS + j], dO + rq * BEAT_DMODEL + h * 32);
  }
  if (h != 7) {
    for (int qh = h; qh < (h == 6 ? 8 : h + 1); ++qh) {
#pragma unroll
      for (int j = 0; j < BEAT_TAPS; ++j) {
        const long long o = (long long)beat_tap_off(qh, j) * dil, tq = t - o;
        if (tq < 0 || tq >= T) continue;
        const long long rq = r - o;
        beat_axpy32(dk, dl[(rq * 8 + qh) * BEAT_TAPS + j], qkv + rq * 768 + qh * 32);
      }
    }
  }
  beat_store32(dqkv + (long long)r * 768 + 256 + h * 32, dk);
  beat_store32(dqkv + (long long)r * 768 + 512 + h * 32, dv);
}
// dEr, level 1: part[slice][h][d][j] = sum over the slice's rows, ascending, of dl[r][h][j] q[r][h][d]; 1280 outputs, 5 per thread
__global__ __launch_bounds__(256) void k_bt_der_part(const float* __restrict__ qkv, const float* __restrict__ dl, int rows, float* __restrict__ part) {
  const long long r0 = (long long)blockIdx.x * BT_ER_ROWS, r1 = r0 + BT_ER_ROWS < rows ? r0 + BT_ER_ROWS : rows;
  for (int e = threadIdx.x; e < 1280; e += 256) {
    const int h = e / 160, d = (e - h * 160) / 5, j = e % 5;
    float a = 0.f;
    for (long long r = r0; r < r1; ++r) a = fmaf(dl[(r * 8 + h) * BEAT_TAPS + j], qkv[r * 768 + h * 32 + d], a);
    part[(long long)blockIdx.x * 1280 + e] = a;
  }
}

// ================================================================================================ instrument attention: one thread per (frame, head)
// backward: the softmax is recomputed as the forward computes it; dq of query i adds its keys in ascending order, dk and dv of key j their queries in ascending order
__global__ __launch_bounds__(64) void k_bt_iattn_bwd(const float* __restrict__ qkv, const float* __restrict__ dao, BeatChunk S, float* __restrict__ dqkv) {
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (long long)S.frames * BEAT_HEADS) return;
  const int f = (int)(gid >> 3), h = (int)(gid & 7), ni = S.instr;
  int s, T, rb;
  beat_frame_at(S, f, s, T, rb);
  float p[8][8], ds[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { p[i][j] = 0.f; ds[i][j] = 0.f; }
    if (i >= ni) continue;
    float q[32], go[32], lg[8], dp[8];
    beat_load32(q, qkv + (rb + (long long)i * T) * 768 + h * 32);
    beat_load32(go, dao + (rb + (long long)i * T) * BEAT_DMODEL + h * 32);
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lg[j] = -INFINITY; dp[j] = 0.f;
      if (j < ni) {
        lg[j] = beat_dot32(q, qkv + (rb + (long long)j * T) * 768 + 256 + h * 32) / BEAT_SCALE;
        mx = fmaxf(mx, lg[j]);
        dp[j] = beat_dot32(go, qkv + (rb + (long long)j * T) * 768 + 512 + h * 32);
      }
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { lg[j] = j < ni ? expf(lg[j] - mx) : 0.f; den += lg[j]; }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { p[i][j] = lg[j] / den; sum = fmaf(p[i][j], dp[j], sum); }
    float dq[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) dq[d] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= ni) continue;
      ds[i][j] = p[i][j] * (dp[j] - sum) / BEAT_SCALE;
      beat_axpy32(dq, ds[i][j], qkv + (rb + (long long)j * T) * 768 + 256 + h * 32);
    }
    beat_store32(dqkv + (rb + (long long)i * T) * 768 + h * 32, dq);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= ni) continue;
    float dk[32], dv[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i >= ni) continue;
      beat_axpy32(dk, ds[i][j], qkv + (rb + (long long)i * T) * 768 + h * 32);
      beat_axpy32(dv, p[i][j], dao + (rb + (long long)i * T) * BEAT_DMODEL + h * 32);
    }
    beat_store32(dqkv + (rb + (long long)j * T) * 768 + 256 + h * 32, dk);
    beat_store32(dqkv + (rb + (long long)j * T) * 768 + 512 + h * 32, dv);
  }
}

// ================================================================================================ skip sum, heads and their backward passes
// every time layer's skip gets the same gradient from the tempo head, dtf[f] (already divided by instr): dsk[r] = dx[r] + dtf[frame of r]
__global__ __launch_bounds__(256) void k_bt_dskip(const float* __restrict__ dx, const float* __restrict__ dtf, BeatChunk S, float* __restrict__ dsk) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.rows * BEAT_DMODEL) return;
  const int r = (int)(gid >> 8), d = (int)(gid & 255);
  int s, T, t;
  beat_row_at(S, r, s, T, t);
  dsk[gid] = dx[gid] + dtf[((long long)S.frame0[s] - S.frame_base + t) * BEAT_DMODEL + d];
}
// hm[f][d] = (sum_i relu(x[row(i, f)][d])) / instr: the beat head's input
__global__ __launch_bounds__(256) void k_bt_hmean(const float* __restrict__ x, BeatChunk S, float* __restrict__ hm) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.frames * BEAT_DMODEL) return;
  const int f = (int)(gid >> 8), d = (int)(gid & 255);
  int s, T, rb;
  beat_frame_at(S, f, s, T, rb);
  float sum = 0.f;
  for (int i = 0; i < S.instr; ++i) sum += fmaxf(x[(rb + (long long)i * T) * BEAT_DMODEL + d], 0.f);
  hm[gid] = sum / (float)S.instr;
}
__global__ __launch_bounds__(256) void k_bt_hmean_bwd(const float* __restrict__ x, const float* __restrict__ dhm, BeatChunk S, float* __restrict__ dx) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.rows * BEAT_DMODEL) return;
  const int r = (int)(gid >> 8), d = (int)(gid & 255);
  int s, T, t;
  beat_row_at(S, r, s, T, t);
  dx[gid] = x[gid] > 0.f ? dhm[((long long)S.frame0[s] - S.frame_base + t) * BEAT_DMODEL + d] / (float)S.instr : 0.f;
}
// tm[s][d] = (sum over segments of BEAT_SEG frames, in order, of the segment's sum of relu(tacc[f][d]) in frame order) / T: the tempo head's input.  One workgroup per song.
__global__ __launch_bounds__(256) void k_bt_tmean(const float* __restrict__ tacc, BeatChunk S, float* __restrict__ tm) {
  const int s = S.first + blockIdx.x, d = threadIdx.x, T = S.frame0[s + 1] - S.frame0[s];
  const float* p = tacc + (long long)(S.frame0[s] - S.frame_base) * BEAT_DMODEL + d;
  float tot = 0.f;
  for (int f0 = 0; f0 < T; f0 += BEAT_SEG) {
    const int f1 = f0 + BEAT_SEG < T ? f0 + BEAT_SEG : T;
    float sum = 0.f;
    for (int f = f0; f < f1; ++f) sum += fmaxf(p[(long long)f * BEAT_DMODEL], 0.f);
    tot += sum;
  }
  tm[(long long)blockIdx.x * BEAT_DMODEL + d] = tot / (float)T;
}
// dtf[f][d] = (tacc > 0) dtm[s][d] / T / instr
__global__ __launch_bounds__(256) void k_bt_tmean_bwd(const float* __restrict__ tacc, const float* __restrict__ dtm, BeatChunk S, float* __restrict__ dtf) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)S.frames * BEAT_DMODEL) return;
  const int f = (int)(gid >> 8), d = (int)(gid & 255);
  int s, T, rb;
  beat_frame_at(S, f, s, T, rb);
  dtf[gid] = tacc[gid] > 0.f ? dtm[(long long)(s - S.first) * BEAT_DMODEL + d] / (float)T / (float)S.instr : 0.f;
}
__global__ void k_bt_relu(const float* __restrict__ x, float* __restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = fmaxf(x[i], 0.f);
}
__global__ void k_bt_relu_bwd(const float* __restrict__ x, float* __restrict__ dy, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dy[i] = x[i] > 0.f ? dy[i] : 0.f;
}

// ================================================================================================ the two loss kernels
__device__ __forceinline__ float add_scalar(float a, float b) {
  float r;
  asm volatile("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__global__ __launch_bounds__(256) void k_bt_bce(const float* __restrict__ z, const float* __restrict__ y, const float* __restrict__ pos_weight,
                                                const float* __restrict__ coef, long long n, int ntoken, float* __restrict__ cell, float* __restrict__ dz) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % ntoken);
  const float yi = y[i], zi = z[i];
  if (yi < 0.f) { cell[i] = 0.f; dz[i] = 0.f; return; }      // -1: not scored
  // (scalar adds and multiplies of their own: left to itself the SLP vectoriser pairs this kernel's independent ones into crossed v_pk_add_f32, the packed form
  // tests/test_isa_guard.py keeps out of the library; see mul_scalar in train_kernels.h)
  const float w = add_scalar(1.f, mul_scalar(add_scalar(pos_weight[c], -1.f), yi));
  const float e = expf(-fabsf(zi));
  const float den = add_scalar(1.f, e);
  const float sg = (zi >= 0.f ? 1.f : e) / den;
  const float lin = add_scalar(fmaxf(zi, 0.f), -mul_scalar(zi, yi));
  cell[i] = mul_scalar(w, add_scalar(lin, logf(den)));      // log(1 + e^-|z|), 1 + e in (1, 2]: within 2^-24 absolute (log1pf's own code pairs into the packed form)
  dz[i] = mul_scalar(coef[c], mul_scalar(w, add_scalar(sg, -yi)));
}
// one wave per song
__global__ __launch_bounds__(64) void k_bt_tempo_ce(const float* __restrict__ t, const float* __restrict__ p, const int* __restrict__ has, float coef, int n_out,
                                                    float* __restrict__ row, float* __restrict__ dt) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const float* tr = t + (long long)s * n_out;
  const float* pr = p + (long long)s * n_out;
  float* dr = dt + (long long)s * n_out;
  if (!has[s]) {                                       // (uniform)
    for (int k = lane; k < n_out; k += 64) dr[k] = 0.f;
    if (lane == 0) row[s] = 0.f;
    return;
  }
  float mx = -INFINITY;
  for (int k = lane; k < n_out; k += 64) mx = fmaxf(mx, tr[k]);
  mx = wave_max(mx);
  float se = 0.f, sp = 0.f;
  for (int k = lane; k < n_out; k += 64) { se += expf(tr[k] - mx); sp += pr[k]; }
  se = wave_sum(se); sp = wave_sum(sp);
  const float lse = mx + logf(se);
  float l = 0.f;
  for (int k = lane; k < n_out; k += 64) {
    l = fmaf(pr[k], lse - tr[k], l);
    dr[k] = coef * ((expf(tr[k] - mx) / se) * sp - pr[k]);
  }
  l = wave_sum(l);
  if (lane == 0) row[s] = l;
}

// ================================================================================================ launchers
static inline dim3 bt_grid(long long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

#define BT_LAUNCHED() do { HIP_TRY(hipGetLastError()); return ETD_OK; } while (0)
// ---- this file's kernels: one launcher per kernel, which the engine and the taps of include/etude_hip_debug.h both call (the shared forward stages: beat.h)
int launch_bt_patch2(const float* c1, int rows, float* x2, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_patch2, bt_grid((long long)rows * BEAT_C2_COLS * BEAT_K2), dim3(256), 0, st, c1, rows, x2);
  BT_LAUNCHED();
}
int launch_bt_repack(float* native, float* packed, int co_n, int ci_n, int kk_n, int dir, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_repack, bt_grid((long long)co_n * ci_n * kk_n), dim3(256), 0, st, native, packed, co_n, ci_n, kk_n, dir);
  BT_LAUNCHED();
}
int launch_bt_pool3_bwd(const float* c3, const float* dx, int rows, float* dc3, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_pool3_bwd, bt_grid((long long)rows * BEAT_DMODEL), dim3(256), 0, st, c3, dx, rows, dc3);
  BT_LAUNCHED();
}
int launch_bt_patch3_bwd(const float* c2, const float* dx3, const BeatChunk& S, float* dc2, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_patch3_bwd, bt_grid((long long)S.rows * 8 * BEAT_C2), dim3(256), 0, st, c2, dx3, S, dc2);
  BT_LAUNCHED();
}
int launch_bt_slice_sum(const float* part, int n_slices, int width, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_slice_sum, bt_grid(width), dim3(256), 0, st, part, n_slices, width, width, out, (float*)nullptr, 0);
  BT_LAUNCHED();
}
int launch_bt_dskip(const float* dx, const float* dtf, const BeatChunk& S, float* dsk, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_dskip, bt_grid((long long)S.rows * 256), dim3(256), 0, st, dx, dtf, S, dsk);
  BT_LAUNCHED();
}
int launch_bt_hmean(const float* x, const BeatChunk& S, float* hm, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_hmean, bt_grid((long long)S.frames * 256), dim3(256), 0, st, x, S, hm);
  BT_LAUNCHED();
}
int launch_bt_hmean_bwd(const float* x, const float* dhm, const BeatChunk& S, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_hmean_bwd, bt_grid((long long)S.rows * 256), dim3(256), 0, st, x, dhm, S, dx);
  BT_LAUNCHED();
}
int launch_bt_tmean(const float* tacc, const BeatChunk& S, float* tm, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_tmean, dim3(S.count), dim3(256), 0, st, tacc, S, tm);
  BT_LAUNCHED();
}
int launch_bt_tmean_bwd(const float* tacc, const float* dtm, const BeatChunk& S, float* dtf, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_tmean_bwd, bt_grid((long long)S.frames * 256), dim3(256), 0, st, tacc, dtm, S, dtf);
  BT_LAUNCHED();
}
int launch_bt_relu(const float* x, float* y, long long n, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_relu, bt_grid(n), dim3(256), 0, st, x, y, n);
  BT_LAUNCHED();
}
int launch_bt_relu_bwd(const float* x, float* dy, long long n, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_relu_bwd, bt_grid(n), dim3(256), 0, st, x, dy, n);
  BT_LAUNCHED();
}

// out[c] += sum over the M rows of dy[r][c] (row stride ld), c < N; part: [ceil(M / BT_CS_ROWS)][N] scratch
int launch_bt_colsum(const float* dy, int ld, int M, int N, float* part, float* out, hipStream_t st) {
  const int ns = (M + BT_CS_ROWS - 1) / BT_CS_ROWS;
  hipLaunchKernelGGL(k_bt_colsum_part, dim3((N + 31) / 32, ns), dim3(256), 0, st, dy, ld, M, N, part);
  return launch_bt_slice_sum(part, ns, N, out, st);
}
int launch_bt_dattn_bwd(const float* qkv, const float* prob, const float* dO, const BeatChunk& S, const float* Er, int dil, float* dl, float* dqkv, float* part,
                        float* dEr, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_dattn_dq, bt_grid((long long)S.rows * 8), dim3(256), 0, st, qkv, prob, dO, S, Er, dil, dl, dqkv);
  hipLaunchKernelGGL(k_bt_dattn_dkv, bt_grid((long long)S.rows * 8), dim3(256), 0, st, qkv, prob, dl, dO, S, dil, dqkv);
  const int ns = (S.rows + BT_ER_ROWS - 1) / BT_ER_ROWS;
  hipLaunchKernelGGL(k_bt_der_part, dim3(ns), dim3(256), 0, st, qkv, dl, S.rows, part);
  return launch_bt_slice_sum(part, ns, 1280, dEr, st);
}
int launch_bt_iattn_bwd(const float* qkv, const float* dao, const BeatChunk& S, float* dqkv, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_iattn_bwd, bt_grid((long long)S.frames * 8, 64), dim3(64), 0, st, qkv, dao, S, dqkv);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_bt_fold2(const float* dpatch, const float* c1, int rows, float* dc1, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_fold2, bt_grid((long long)rows * BEAT_W1 * BEAT_C1), dim3(256), 0, st, dpatch, c1, rows, dc1);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_bt_conv1_bwd(const float* feat, const float* dc1, const BeatChunk& S, const float* w, const float* b, float* part, float* dw, float* db, hipStream_t st) {
  const int ns = (S.rows + BT_C1_ROWS - 1) / BT_C1_ROWS;
  hipLaunchKernelGGL(k_bt_conv1_bwd, dim3(ns), dim3(256), 0, st, feat, dc1, S, w, b, part);
  hipLaunchKernelGGL(k_bt_slice_sum, bt_grid(512), dim3(256), 0, st, part, ns, 512, 512, dw, db, 1);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_bt_bce(const float* z, const float* y, const float* pos_weight, const float* coef, int frames, int ntoken, float* cell, float* dz, hipStream_t st) {
  const long long n = (long long)frames * ntoken;
  hipLaunchKernelGGL(k_bt_bce, bt_grid(n), dim3(256), 0, st, z, y, pos_weight, coef, n, ntoken, cell, dz);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_bt_tempo_ce(const float* t, const float* p, const int* has, float coef, int n, int n_out, float* row, float* dt, hipStream_t st) {
  hipLaunchKernelGGL(k_bt_tempo_ce, dim3(n), dim3(64), 0, st, t, p, has, coef, n_out, row, dt);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ================================================================================================ the engine
namespace {
struct BTime { size_t qkv_w, qkv_b, Er, n1w, n1b, n2w, n2b, l1w, l1b, l2w, l2b; };
struct BInstr { size_t in_w, in_b, out_w, out_b, n1w, n1b, n2w, n2b, l1w, l1b, l2w, l2b; };
// what one time layer (and the instrument layer behind it) keeps from forward to backward, per row: x 256, qkv 768, prob 40, x after attention 256, pre d_hid, 4 statistics
struct BSavedT { float *xin, *qkv, *prob, *xat, *pre, *m1, *r1, *m2, *r2; };
struct BSavedI { float *xin, *qkv, *ao, *xat, *pre, *m1, *r1, *m2, *r2; };
}  // namespace

struct etd_btrain {
  etd_btrain_cfg cfg;
  std::vector<float> pos_weight;
  TrainStore ps;                           // every tensor is trained: the norm and the step run over n_total
  size_t c1w = 0, c1b = 0, c2w = 0, c2b = 0, c3w = 0, c3b = 0, ow = 0, ob = 0, tw = 0, tb = 0;
  std::vector<BTime> tl;
  std::vector<BInstr> il;                  // for time layers 3 .. 5 (those below nlayers)
  // packed conv weights and their gradients ([co][kk][ci])
  float *w2p = nullptr, *w3p = nullptr, *dw2p = nullptr, *dw3p = nullptr;
  // saved activations
  float *c1 = nullptr, *x2 = nullptr, *c2o = nullptr, *x3 = nullptr, *c3o = nullptr, *xL = nullptr, *tacc = nullptr, *hm = nullptr, *tm = nullptr, *logits = nullptr, *tlog = nullptr;
  std::vector<BSavedT> st;
  std::vector<BSavedI> si;
  // scratch
  float *wI = nullptr, *tx = nullptr, *dxn = nullptr, *dx = nullptr, *dsk = nullptr, *dqkv = nullptr, *dl = nullptr, *big = nullptr, *part = nullptr, *dtf = nullptr, *dhm = nullptr,
        *dtm = nullptr, *seg = nullptr, *cpart = nullptr, *dz = nullptr, *dt = nullptr, *cell = nullptr, *trow = nullptr, *ytgt = nullptr, *ttgt = nullptr, *fl = nullptr;
  int* ints = nullptr;
  std::vector<float> h_cell, h_trow;
  int last_rows = 0, last_frames = 0;      // of the last call that ran (etd_debug_btrain_read_rows)
  size_t workspace_bytes = 0;
  DevPool pool;
};

static int btrain_check_cfg(const etd_btrain_cfg* cfg) {
  if (!cfg) ETD_FAIL(ETD_EINVAL, "etd_btrain: null config");
  ETD_CHECK_CFG(cfg, etd_btrain_cfg, "etd_btrain");
  const etd_btrain_cfg& c = *cfg;
  if (c.nhead != 8) ETD_FAIL(ETD_EINVAL, "etd_btrain: nhead = %d; the dilated head table is written for 8 heads", c.nhead);
  if (c.attn_len != 5) ETD_FAIL(ETD_EINVAL, "etd_btrain: attn_len = %d; the dilated head table is written for 5 taps", c.attn_len);
  if (c.dmodel != 256) ETD_FAIL(ETD_EINVAL, "etd_btrain: dmodel = %d; this engine takes dmodel = 256 (head_dim 32)", c.dmodel);
  if (!c.norm_first) ETD_FAIL(ETD_EINVAL, "etd_btrain: norm_first = 0 (post-norm layers) is not supported");
  if (c.n_mels != 128) ETD_FAIL(ETD_EINVAL, "etd_btrain: n_mels = %d; the conv front end pools 128 mel bins to one token", c.n_mels);
  if (c.instr < 1 || c.instr > 8) ETD_FAIL(ETD_EINVAL, "etd_btrain: instr = %d (1 .. 8)", c.instr);
  if (c.d_hid < 256 || c.d_hid % 256 || c.d_hid > 8192) ETD_FAIL(ETD_EINVAL, "etd_btrain: d_hid = %d (a multiple of 256, <= 8192)", c.d_hid);
  if (c.nlayers < 1 || c.nlayers > 16) ETD_FAIL(ETD_EINVAL, "etd_btrain: nlayers = %d (1 .. 16)", c.nlayers);
  if (c.ntoken < 1 || c.ntoken > 64) ETD_FAIL(ETD_EINVAL, "etd_btrain: ntoken = %d (1 .. 64)", c.ntoken);
  if (c.tempo_out != BT_TEMPO) ETD_FAIL(ETD_EINVAL, "etd_btrain: tempo_out = %d; the tempo head has %d classes", c.tempo_out, BT_TEMPO);
  if (c.max_rows < 1 || c.max_rows > (1 << 17)) ETD_FAIL(ETD_EINVAL, "etd_btrain: max_rows = %d (1 .. 2^17)", c.max_rows);
  if (c.max_seqs < 1 || c.max_seqs > 65535) ETD_FAIL(ETD_EINVAL, "etd_btrain: max_seqs = %d (1 .. 65535)", c.max_seqs);
  if (!(c.dropout == 0.f)) ETD_FAIL(ETD_EINVAL, "etd_btrain: dropout = %g; the trained arithmetic is the inference arithmetic, dropout is not implemented and must be 0", (double)c.dropout);
  if (!(c.tempo_weight >= 0.f) || !std::isfinite(c.tempo_weight)) ETD_FAIL(ETD_EINVAL, "etd_btrain: tempo_weight must be finite and >= 0");
  return ETD_OK;
}

static int n_instr_layers(int nlayers) { return nlayers > 6 ? 3 : nlayers > 3 ? nlayers - 3 : 0; }

// scratch of launch_bt_colsum: the widest of its uses (d_hid or 768 columns over R rows, 64 over 24 R, 256 over 3 R, 300 over the songs)
static long long btrain_cpart_floats(const etd_btrain_cfg& c) {
  const long long R = c.max_rows, W = c.d_hid > 768 ? c.d_hid : 768, S = BT_CS_ROWS;
  return std::max(std::max((R + S - 1) / S * W, (BEAT_C2_COLS * R + S - 1) / S * 64), std::max((3 * R + S - 1) / S * 256, ((long long)c.max_seqs + S - 1) / S * BT_TEMPO));
}

// floats of saved activations and scratch for these arguments (the allocations of create, in its order)
static long long btrain_ws_floats(const etd_btrain_cfg& c) {
  const long long R = c.max_rows, H = c.d_hid, n = c.max_seqs, nt = c.ntoken;
  long long f = R * (BEAT_W1 * BEAT_C1 + BEAT_C2_COLS * BEAT_K2 + BEAT_C2_COLS * BEAT_C2 + 3 * BEAT_K3 + 3 * 256 + 256 + 256 + 256);      // c1 x2 c2o x3 c3o xL tacc hm
  f += n * 256 + R * nt + n * BT_TEMPO;                                                                                             // tm logits tlog
  f += (long long)c.nlayers * R * (256 + 768 + 40 + 256 + H + 4);
  f += (long long)n_instr_layers(c.nlayers) * R * (256 + 768 + 256 + 256 + H + 4);
  f += R * (H + 256 * 4 + 768 + 40 + (long long)BEAT_C2_COLS * BEAT_K2 + 256 + 256);                                                     // wI tx dxn dx dsk dqkv dl big dtf dhm
  f += ((R + BT_C1_ROWS - 1) / BT_C1_ROWS) * 512 + ((R + BT_ER_ROWS - 1) / BT_ER_ROWS) * 1280;                                      // part (the larger is used; both counted)
  f += std::max((3 * R + BT_SEG_ROWS - 1) / BT_SEG_ROWS * (256LL * BEAT_K3 + 256), (BEAT_C2_COLS * R + BT_SEG_ROWS - 1) / BT_SEG_ROWS * (64LL * BEAT_K2 + 64));      // seg
  f += btrain_cpart_floats(c);
  f += n * 256 + R * nt * 3 + n * BT_TEMPO * 2 + n + 2 * nt;                                                                        // dtm dz cell ytgt dt ttgt trow fl
  return f;
}

extern "C" long long etd_btrain_workspace_bytes(const etd_btrain_cfg* cfg) {
  if (btrain_check_cfg(cfg) != ETD_OK) return ETD_EINVAL;
  return 4 * btrain_ws_floats(*cfg);
}

extern "C" int etd_btrain_create(const etd_btrain_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n,
                                 const float* pos_weight, etd_btrain** out) {
  if (!out) ETD_FAIL(ETD_EINVAL, "etd_btrain_create: null out");
  *out = nullptr;
  ETD_TRY(btrain_check_cfg(cfg));
  if (!names || !host_ptrs || !numels || n < 1) ETD_FAIL(ETD_EINVAL, "etd_btrain_create: no weights");
  const etd_btrain_cfg& c = *cfg;
  if (pos_weight)
    for (int k = 0; k < c.ntoken; ++k)
      if (!(pos_weight[k] > 0.f) || !std::isfinite(pos_weight[k])) ETD_FAIL(ETD_EINVAL, "etd_btrain_create: pos_weight[%d] must be finite and > 0", k);
  etd_btrain* d = new etd_btrain();
  auto fail = [&](int rc) { d->pool.free_all(); delete d; return rc; };
  d->cfg = c;
  d->pos_weight.assign(c.ntoken, 1.f);
  if (pos_weight) d->pos_weight.assign(pos_weight, pos_weight + c.ntoken);
  const size_t D = 256, H = c.d_hid;
  TrainStore& ps = d->ps;
  d->c1w = ps.add("conv1.weight", 32 * 15); d->c1b = ps.add("conv1.bias", 32);
  d->c2w = ps.add("conv2.weight", 64 * BEAT_K2); d->c2b = ps.add("conv2.bias", 64);
  d->c3w = ps.add("conv3.weight", D * BEAT_K3); d->c3b = ps.add("conv3.bias", D);
  for (int l = 0; l < c.nlayers; ++l) {
    const std::string p = "Transformer_layers.time_attention_" + std::to_string(l) + ".";
    BTime t;
    // query | key | value back to back: one [768][256] weight and one [768] bias for the fused projection (every tensor is a multiple of 64 floats: no gaps)
    t.qkv_w = ps.add(p + "self_attn.query.weight", D * D); ps.add(p + "self_attn.key.weight", D * D); ps.add(p + "self_attn.value.weight", D * D);
    t.qkv_b = ps.add(p + "self_attn.query.bias", D); ps.add(p + "self_attn.key.bias", D); ps.add(p + "self_attn.value.bias", D);
    t.Er = ps.add(p + "self_attn.Er", 8 * 32 * 5);
    t.n1w = ps.add(p + "norm1.weight", D); t.n1b = ps.add(p + "norm1.bias", D); t.n2w = ps.add(p + "norm2.weight", D); t.n2b = ps.add(p + "norm2.bias", D);
    t.l1w = ps.add(p + "linear1.weight", H * D); t.l1b = ps.add(p + "linear1.bias", H);
    t.l2w = ps.add(p + "linear2.weight", D * H); t.l2b = ps.add(p + "linear2.bias", D);
    d->tl.push_back(t);
    if (l >= 3 && l <= 5) {
      const std::string q = "Transformer_layers.instr_attention_" + std::to_string(l) + ".";
      BInstr i;
      i.in_w = ps.add(q + "self_attn.in_proj_weight", 3 * D * D); i.in_b = ps.add(q + "self_attn.in_proj_bias", 3 * D);
      i.out_w = ps.add(q + "self_attn.out_proj.weight", D * D); i.out_b = ps.add(q + "self_attn.out_proj.bias", D);
      i.n1w = ps.add(q + "norm1.weight", D); i.n1b = ps.add(q + "norm1.bias", D); i.n2w = ps.add(q + "norm2.weight", D); i.n2b = ps.add(q + "norm2.bias", D);
      i.l1w = ps.add(q + "linear1.weight", H * D); i.l1b = ps.add(q + "linear1.bias", H);
      i.l2w = ps.add(q + "linear2.weight", D * H); i.l2b = ps.add(q + "linear2.bias", D);
      d->il.push_back(i);
    }
  }
  d->ow = ps.add("out_linear.weight", (size_t)c.ntoken * D); d->ob = ps.add("out_linear.bias", c.ntoken);
  d->tw = ps.add("out_linear_t.weight", (size_t)BT_TEMPO * D); d->tb = ps.add("out_linear_t.bias", BT_TEMPO);
  // host image of the parameters, checked before the device is touched
  WeightTable wt(names, host_ptrs, numels, n);
  if (wt.null_name >= 0) { g_etd_err = "etd_btrain_create: null name " + std::to_string(wt.null_name); return fail(ETD_EINVAL); }
  ps.n_train = ps.n_total;
  std::vector<float> host(ps.n_total, 0.f);
  if (ps.fill(wt, host.data()) != ETD_OK) { g_etd_err = "etd_btrain_create: " + g_etd_err; return fail(ETD_EINVAL); }
  // ---- device
  DevPool& pl = d->pool;
  ETD_TRY_OR(fail, ps.upload(pl, host.data(), ps.n_total));
  ETD_TRY_OR(fail, pl.alloc(&d->w2p, (size_t)64 * BEAT_K2)); ETD_TRY_OR(fail, pl.alloc(&d->dw2p, (size_t)64 * BEAT_K2));
  ETD_TRY_OR(fail, pl.alloc(&d->w3p, D * BEAT_K3)); ETD_TRY_OR(fail, pl.alloc(&d->dw3p, D * BEAT_K3));
  ETD_TRY_OR(fail, pl.alloc(&ps.partial, (size_t)TN_BLOCKS));
  const size_t R = (size_t)c.max_rows, ns = (size_t)c.max_seqs, nt = (size_t)c.ntoken;
  const size_t before = pl.mark();
  ETD_TRY_OR(fail, pl.alloc(&d->c1, R * BEAT_W1 * BEAT_C1)); ETD_TRY_OR(fail, pl.alloc(&d->x2, R * BEAT_C2_COLS * BEAT_K2)); ETD_TRY_OR(fail, pl.alloc(&d->c2o, R * BEAT_C2_COLS * BEAT_C2));
  ETD_TRY_OR(fail, pl.alloc(&d->x3, R * 3 * BEAT_K3)); ETD_TRY_OR(fail, pl.alloc(&d->c3o, R * 3 * D)); ETD_TRY_OR(fail, pl.alloc(&d->xL, R * D));
  ETD_TRY_OR(fail, pl.alloc(&d->tacc, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->hm, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->tm, ns * D));
  ETD_TRY_OR(fail, pl.alloc(&d->logits, R * nt)); ETD_TRY_OR(fail, pl.alloc(&d->tlog, ns * BT_TEMPO));
  for (int l = 0; l < c.nlayers; ++l) {
    BSavedT s;
    ETD_TRY_OR(fail, pl.alloc(&s.xin, R * D)); ETD_TRY_OR(fail, pl.alloc(&s.qkv, R * 768)); ETD_TRY_OR(fail, pl.alloc(&s.prob, R * 40)); ETD_TRY_OR(fail, pl.alloc(&s.xat, R * D));
    ETD_TRY_OR(fail, pl.alloc(&s.pre, R * H)); ETD_TRY_OR(fail, pl.alloc(&s.m1, R)); ETD_TRY_OR(fail, pl.alloc(&s.r1, R)); ETD_TRY_OR(fail, pl.alloc(&s.m2, R)); ETD_TRY_OR(fail, pl.alloc(&s.r2, R));
    d->st.push_back(s);
  }
  for (size_t l = 0; l < d->il.size(); ++l) {
    BSavedI s;
    ETD_TRY_OR(fail, pl.alloc(&s.xin, R * D)); ETD_TRY_OR(fail, pl.alloc(&s.qkv, R * 768)); ETD_TRY_OR(fail, pl.alloc(&s.ao, R * D)); ETD_TRY_OR(fail, pl.alloc(&s.xat, R * D));
    ETD_TRY_OR(fail, pl.alloc(&s.pre, R * H)); ETD_TRY_OR(fail, pl.alloc(&s.m1, R)); ETD_TRY_OR(fail, pl.alloc(&s.r1, R)); ETD_TRY_OR(fail, pl.alloc(&s.m2, R)); ETD_TRY_OR(fail, pl.alloc(&s.r2, R));
    d->si.push_back(s);
  }
  ETD_TRY_OR(fail, pl.alloc(&d->wI, R * H)); ETD_TRY_OR(fail, pl.alloc(&d->tx, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->dxn, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->dx, R * D));
  ETD_TRY_OR(fail, pl.alloc(&d->dsk, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->dqkv, R * 768)); ETD_TRY_OR(fail, pl.alloc(&d->dl, R * 40));
  ETD_TRY_OR(fail, pl.alloc(&d->big, R * BEAT_C2_COLS * BEAT_K2));      // dx3 [3 R][1152], then conv2's dpatch [24 R][384], then dc1 [R][42][32]: each is dead when the next is written
  ETD_TRY_OR(fail, pl.alloc(&d->part, std::max((R + BT_C1_ROWS - 1) / BT_C1_ROWS * 512, (R + BT_ER_ROWS - 1) / BT_ER_ROWS * 1280)));
  ETD_TRY_OR(fail, pl.alloc(&d->seg, std::max((3 * R + BT_SEG_ROWS - 1) / BT_SEG_ROWS * (D * BEAT_K3 + D), (BEAT_C2_COLS * R + BT_SEG_ROWS - 1) / BT_SEG_ROWS * (size_t)(64 * BEAT_K2 + 64))));
  ETD_TRY_OR(fail, pl.alloc(&d->cpart, (size_t)btrain_cpart_floats(c)));
  ETD_TRY_OR(fail, pl.alloc(&d->dtf, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->dhm, R * D)); ETD_TRY_OR(fail, pl.alloc(&d->dtm, ns * D));
  ETD_TRY_OR(fail, pl.alloc(&d->dz, R * nt)); ETD_TRY_OR(fail, pl.alloc(&d->cell, R * nt)); ETD_TRY_OR(fail, pl.alloc(&d->ytgt, R * nt));
  ETD_TRY_OR(fail, pl.alloc(&d->dt, ns * BT_TEMPO)); ETD_TRY_OR(fail, pl.alloc(&d->ttgt, ns * BT_TEMPO)); ETD_TRY_OR(fail, pl.alloc(&d->trow, ns)); ETD_TRY_OR(fail, pl.alloc(&d->fl, 2 * nt));
  ETD_TRY_OR(fail, pl.alloc(&d->ints, 3 * (ns + 1)));
  for (size_t i = before; i < pl.bytes.size(); ++i) d->workspace_bytes += pl.bytes[i];
  *out = d;
  return ETD_OK;
}

extern "C" void etd_btrain_destroy(etd_btrain* d) {
  if (!d) return;
  (void)hipDeviceSynchronize();
  d->pool.free_all();
  delete d;
}

extern "C" long long etd_btrain_bytes(const etd_btrain* d, int what) {
  if (!d) return ETD_EINVAL;
  return what == 0 ? (long long)d->workspace_bytes : (long long)(4 * d->ps.n_total * sizeof(float));
}

// HOST ONLY: the argument checks of etd_btrain_loss_backward.  n_scored [ntoken] (may be NULL): scored cells per class; *n_tempo: songs with a tempo target
extern "C" int etd_btrain_check_batch(const etd_btrain_cfg* cfg, int n_seq, const int64_t* T_host, const float* beat_targets, const float* tempo_targets,
                                      const int32_t* has_tempo, int32_t* n_scored, int32_t* n_tempo) {
  ETD_TRY(btrain_check_cfg(cfg));
  if (!T_host || !beat_targets || n_seq < 1) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: null argument or n_seq < 1");
  if (n_seq > cfg->max_seqs) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: %d songs, the workspace was sized for %d", n_seq, cfg->max_seqs);
  long long rows = 0, frames = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (T_host[s] < 1) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: song %d has T = %lld (need >= 1)", s, (long long)T_host[s]);
    rows += T_host[s] * cfg->instr; frames += T_host[s];
    if (rows > cfg->max_rows) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: more than max_rows = %d rows (instr x frames); the workspace was sized for that many", cfg->max_rows);
  }
  const int nt = cfg->ntoken;
  std::vector<int32_t> cnt(nt, 0);
  for (long long i = 0; i < frames * nt; ++i) {
    const float y = beat_targets[i];
    if (y == -1.f) continue;
    if (!(y >= 0.f && y <= 1.f)) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: beat target %g at frame %lld, class %d is neither in [0, 1] nor -1", (double)y, i / nt, (int)(i % nt));
    ++cnt[i % nt];
  }
  int ntempo = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (!has_tempo || !has_tempo[s]) continue;
    if (!tempo_targets) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: has_tempo without tempo targets");
    double sum = 0.0;
    for (int k = 0; k < BT_TEMPO; ++k) {
      const float p = tempo_targets[(size_t)s * BT_TEMPO + k];
      if (!(p >= 0.f) || !std::isfinite(p)) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: tempo target of song %d holds %g at %d (need finite, >= 0)", s, (double)p, k);
      sum += (double)p;
    }
    if (!(fabs(sum - 1.0) <= 1e-5)) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: tempo target of song %d sums to %.9g, not to 1 within 1e-5", s, sum);
    ++ntempo;
  }
  if (n_scored) for (int k = 0; k < nt; ++k) n_scored[k] = cnt[k];
  if (n_tempo) *n_tempo = ntempo;
  return ETD_OK;
}

#define BT_GEMM(...) ETD_TRY(launch_tgemm(__VA_ARGS__))

// one feed-forward sublayer's backward (act 0: GELU, 1: ReLU): dx is the gradient of the sublayer's output x + W2 act(W1 LN(x) + b1) + b2 on entry, of x on exit
// P / G: the buffers the six offsets (LayerNorm gain, bias, linear1, linear2) index -- the engine's flat parameters and accumulated gradients, or a tap's own
static int ffn_backward(etd_btrain* d, int R, int act, const float* x, const float* mean, const float* rstd, const float* pre, const float* P, float* G, float* dx, size_t nw,
                        size_t nb, size_t l1w, size_t l1b, size_t l2w, size_t l2b, hipStream_t st) {
  const int H = d->cfg.d_hid;
  const long long RH = (long long)R * H;
  if (act == 0) launch_tgelu(pre, d->wI, RH, st);
  else ETD_TRY(launch_bt_relu(pre, d->wI, RH, st));
  BT_GEMM(ETD_TG_TN, 256, H, R, dx, 256, d->wI, H, nullptr, G + l2w, H, true, st);
  ETD_TRY(launch_bt_colsum(dx, 256, R, 256, d->cpart, G + l2b, st));
  BT_GEMM(ETD_TG_NN, R, H, 256, dx, 256, P + l2w, H, nullptr, d->wI, H, false, st);
  if (act == 0) launch_tgelu_bwd(pre, d->wI, RH, st);
  else ETD_TRY(launch_bt_relu_bwd(pre, d->wI, RH, st));
  launch_tln_fwd(x, R, 256, 1e-5f, nullptr, nullptr, P + nw, P + nb, d->tx, nullptr, nullptr, nullptr, st);
  BT_GEMM(ETD_TG_TN, H, 256, R, d->wI, H, d->tx, 256, nullptr, G + l1w, 256, true, st);
  ETD_TRY(launch_bt_colsum(d->wI, H, R, H, d->cpart, G + l1b, st));
  BT_GEMM(ETD_TG_NN, R, 256, H, d->wI, H, P + l1w, 256, nullptr, d->dxn, 256, false, st);
  launch_tcolred(1, d->dxn, 256, R, 256, x, mean, rstd, G + nb, G + nw, st);
  launch_tln_bwd(d->dxn, x, mean, rstd, P + nw, R, 256, dx, st);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
// a fused q | k | v projection's backward from dqkv: its weight and bias, the LayerNorm in front of it, and dx += the LayerNorm's input gradient
static int proj_backward(etd_btrain* d, int R, const float* x, const float* mean, const float* rstd, const float* dqkv, const float* P, float* G, float* dx, size_t nw,
                         size_t nb, size_t w, size_t b, hipStream_t st) {
  launch_tln_fwd(x, R, 256, 1e-5f, nullptr, nullptr, P + nw, P + nb, d->tx, nullptr, nullptr, nullptr, st);
  BT_GEMM(ETD_TG_TN, 768, 256, R, dqkv, 768, d->tx, 256, nullptr, G + w, 256, true, st);
  // The query and value biases only.  A key bias (a time layer's or an instrument layer's) adds the same q . b to every logit of a query, which the softmax cancels: its
  // gradient is identically zero, and summing dk over the rows would only leave rounding residue there (which AdamW's normalisation would turn into steps of the size of
  // lr).  It is left at exactly zero (tests/test_gpu_beat_train.py::test_key_bias_gradients_are_exactly_zero).
  ETD_TRY(launch_bt_colsum(dqkv, 768, R, 256, d->cpart, G + b, st));
  ETD_TRY(launch_bt_colsum(dqkv + 512, 768, R, 256, d->cpart, G + b + 512, st));
  BT_GEMM(ETD_TG_NN, R, 256, 768, dqkv, 768, P + w, 256, nullptr, d->dxn, 256, false, st);
  launch_tcolred(1, d->dxn, 256, R, 256, x, mean, rstd, G + nb, G + nw, st);
  launch_tln_bwd(d->dxn, x, mean, rstd, P + nw, R, 256, dx, st);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// A conv layer's weight gradient: the reduction runs over 3 (conv3) or 24 (conv2) rows per token, too long for one fp32 chain per element at the bound of
// DESIGN.md 4s.  It runs in segments of BT_SEG_ROWS rows: each segment's dY^T X goes to a slice of `seg` of their own, k_bt_slice_sum adds the slices
// in order.  dw [M][N] is overwritten (the packed weight's gradient of this call).
int launch_bt_conv_wgrad(int M, int N, int K, const float* dY, const float* X, float* seg, float* dw, hipStream_t st) {
  const int ns = (K + BT_SEG_ROWS - 1) / BT_SEG_ROWS;
  const long long width = (long long)M * N;
  for (int q = 0; q < ns; ++q) {
    const int k0 = q * BT_SEG_ROWS, kn = K - k0 < BT_SEG_ROWS ? K - k0 : BT_SEG_ROWS;
    BT_GEMM(ETD_TG_TN, M, N, kn, dY + (long long)k0 * M, M, X + (long long)k0 * N, N, nullptr, seg + q * width, N, false, st);
  }
  HIP_TRY(hipMemsetAsync(dw, 0, (size_t)width * 4, st));
  return launch_bt_slice_sum(seg, ns, (int)width, dw, st);
}

extern "C" int etd_btrain_loss_backward(etd_btrain* d, const float* feat_dev, int n_seq, const int64_t* T_host, const float* beat_targets, const float* tempo_targets,
                                        const int32_t* has_tempo, float loss_scale, float* loss_out, int32_t* n_scored_out, int32_t* skipped_out, void* stream) {
  if (!d || !feat_dev || !loss_out || !n_scored_out || !skipped_out) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: null argument");
  if (!std::isfinite(loss_scale)) ETD_FAIL(ETD_EINVAL, "etd_btrain_loss_backward: loss_scale is not finite");
  const etd_btrain_cfg& c = d->cfg;
  const int nt = c.ntoken, ni = c.instr, H = c.d_hid, L = c.nlayers;
  std::vector<int32_t> cnt(nt, 0);
  int32_t ntempo = 0;
  ETD_TRY(etd_btrain_check_batch(&c, n_seq, T_host, beat_targets, tempo_targets, has_tempo, cnt.data(), &ntempo));
  long long scored = 0;
  for (int k = 0; k < nt; ++k) scored += cnt[k];
  *n_scored_out = (int32_t)scored;
  *skipped_out = 0;
  if (scored == 0 && ntempo == 0) {                    // nothing to learn from: nothing is launched, the accumulated gradients keep every bit
    *loss_out = NAN; *skipped_out = 1;
    return ETD_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  // ---- the call's tables
  std::vector<int> tab(3 * (size_t)(n_seq + 1), 0);     // row0 | frame0 | has_tempo
  long long rows = 0, frames = 0;
  for (int s = 0; s < n_seq; ++s) {
    tab[s] = (int)rows; tab[n_seq + 1 + s] = (int)frames; tab[2 * (n_seq + 1) + s] = has_tempo && has_tempo[s] ? 1 : 0;
    rows += T_host[s] * ni; frames += T_host[s];
  }
  tab[n_seq] = (int)rows; tab[2 * n_seq + 1] = (int)frames;
  const int R = (int)rows, F = (int)frames;
  d->last_rows = R; d->last_frames = F;
  std::vector<float> fl(2 * (size_t)nt);                // pos_weight | coef = loss_scale / n_c (0 for a class with no scored cell)
  for (int k = 0; k < nt; ++k) { fl[k] = d->pos_weight[k]; fl[nt + k] = cnt[k] ? (float)((double)loss_scale / (double)cnt[k]) : 0.f; }
  const float tcoef = ntempo ? (float)((double)c.tempo_weight * (double)loss_scale / (double)ntempo) : 0.f;
  HIP_TRY(hipMemcpyAsync(d->ints, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d->fl, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d->ytgt, beat_targets, (size_t)F * nt * 4, hipMemcpyHostToDevice, st));
  if (ntempo) HIP_TRY(hipMemcpyAsync(d->ttgt, tempo_targets, (size_t)n_seq * BT_TEMPO * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));                    // (the host tables are this call's memory)
  const BeatChunk S = beat_whole_call(d->ints, d->ints + n_seq + 1, n_seq, R, F, ni);
  const int* d_has = d->ints + 2 * (n_seq + 1);
  float *P = d->ps.P, *G = d->ps.G;
  const long long RD = (long long)R * 256, RH = (long long)R * H;
  auto copy = [&](float* dst, const float* src, long long nfl) -> int {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)nfl * 4, hipMemcpyDeviceToDevice, st));
    return ETD_OK;
  };
  // ================================================================ forward
  {
    ProfScope ps("btrain_forward", st);
    ETD_TRY(launch_bt_repack(P + d->c2w, d->w2p, 64, 32, 12, 0, st));
    ETD_TRY(launch_bt_repack(P + d->c3w, d->w3p, 256, 64, 18, 0, st));
    ETD_TRY(launch_beat_conv1(feat_dev, S, P + d->c1w, P + d->c1b, d->c1, st));
    ETD_TRY(launch_bt_patch2(d->c1, R, d->x2, st));
    BT_GEMM(ETD_TG_NT, R * BEAT_C2_COLS, 64, BEAT_K2, d->x2, BEAT_K2, d->w2p, BEAT_K2, P + d->c2b, d->c2o, 64, false, st);
    ETD_TRY(launch_beat_patch3(d->c2o, BEAT_C2_COLS, S, d->x3, st));
    BT_GEMM(ETD_TG_NT, R * 3, 256, BEAT_K3, d->x3, BEAT_K3, d->w3p, BEAT_K3, P + d->c3b, d->c3o, 256, false, st);
    float* x0 = d->st[0].xin;
    ETD_TRY(launch_beat_pool3(d->c3o, R, x0, st));
    HIP_TRY(hipGetLastError());
    int il = 0;
    for (int l = 0; l < L; ++l) {
      const BTime& y = d->tl[l];
      const BSavedT& a = d->st[l];
      const bool has_i = l >= 3 && l <= 5;
      float* xnext = has_i ? d->si[il].xin : l + 1 < L ? d->st[l + 1].xin : d->xL;
      launch_tln_fwd(a.xin, R, 256, 1e-5f, a.m1, a.r1, P + y.n1w, P + y.n1b, d->tx, nullptr, nullptr, nullptr, st);
      BT_GEMM(ETD_TG_NT, R, 768, 256, d->tx, 256, P + y.qkv_w, 256, P + y.qkv_b, a.qkv, 768, false, st);
      ETD_TRY(launch_beat_dattn_train(a.qkv, S, P + y.Er, 1 << l, a.xin, a.prob, d->dsk, a.xat, st));
      ETD_TRY(launch_beat_skipacc(d->dsk, S, l == 0 ? 1 : 0, d->tacc, st));
      launch_tln_fwd(a.xat, R, 256, 1e-5f, a.m2, a.r2, P + y.n2w, P + y.n2b, d->tx, nullptr, nullptr, nullptr, st);
      BT_GEMM(ETD_TG_NT, R, H, 256, d->tx, 256, P + y.l1w, 256, P + y.l1b, a.pre, H, false, st);
      launch_tgelu(a.pre, d->wI, RH, st);
      ETD_TRY(copy(xnext, a.xat, RD));
      BT_GEMM(ETD_TG_NT, R, 256, H, d->wI, H, P + y.l2w, H, P + y.l2b, xnext, 256, true, st);
      if (has_i) {
        const BInstr& z = d->il[il];
        const BSavedI& b = d->si[il];
        float* xn2 = l + 1 < L ? d->st[l + 1].xin : d->xL;
        launch_tln_fwd(b.xin, R, 256, 1e-5f, b.m1, b.r1, P + z.n1w, P + z.n1b, d->tx, nullptr, nullptr, nullptr, st);
        BT_GEMM(ETD_TG_NT, R, 768, 256, d->tx, 256, P + z.in_w, 256, P + z.in_b, b.qkv, 768, false, st);
        ETD_TRY(launch_beat_iattn(b.qkv, S, b.ao, st));
        ETD_TRY(copy(b.xat, b.xin, RD));
        BT_GEMM(ETD_TG_NT, R, 256, 256, b.ao, 256, P + z.out_w, 256, P + z.out_b, b.xat, 256, true, st);
        launch_tln_fwd(b.xat, R, 256, 1e-5f, b.m2, b.r2, P + z.n2w, P + z.n2b, d->tx, nullptr, nullptr, nullptr, st);
        BT_GEMM(ETD_TG_NT, R, H, 256, d->tx, 256, P + z.l1w, 256, P + z.l1b, b.pre, H, false, st);
        ETD_TRY(launch_bt_relu(b.pre, d->wI, RH, st));
        ETD_TRY(copy(xn2, b.xat, RD));
        BT_GEMM(ETD_TG_NT, R, 256, H, d->wI, H, P + z.l2w, H, P + z.l2b, xn2, 256, true, st);
        ++il;
      }
    }
    ETD_TRY(launch_bt_hmean(d->xL, S, d->hm, st));
    BT_GEMM(ETD_TG_NT, F, nt, 256, d->hm, 256, P + d->ow, 256, P + d->ob, d->logits, nt, false, st);
    ETD_TRY(launch_bt_tmean(d->tacc, S, d->tm, st));
    BT_GEMM(ETD_TG_NT, n_seq, BT_TEMPO, 256, d->tm, 256, P + d->tw, 256, P + d->tb, d->tlog, BT_TEMPO, false, st);
    ETD_TRY(launch_bt_bce(d->logits, d->ytgt, d->fl, d->fl + nt, F, nt, d->cell, d->dz, st));
    if (ntempo) ETD_TRY(launch_bt_tempo_ce(d->tlog, d->ttgt, d_has, tcoef, n_seq, BT_TEMPO, d->trow, d->dt, st));
    HIP_TRY(hipGetLastError());
  }
  // ================================================================ backward
  {
    ProfScope ps("btrain_backward", st);
    // ---- tempo head: dtf = the gradient every time layer's skip receives (zeros without a tempo target)
    if (ntempo) {
      BT_GEMM(ETD_TG_TN, BT_TEMPO, 256, n_seq, d->dt, BT_TEMPO, d->tm, 256, nullptr, G + d->tw, 256, true, st);
      ETD_TRY(launch_bt_colsum(d->dt, BT_TEMPO, n_seq, BT_TEMPO, d->cpart, G + d->tb, st));
      BT_GEMM(ETD_TG_NN, n_seq, 256, BT_TEMPO, d->dt, BT_TEMPO, P + d->tw, 256, nullptr, d->dtm, 256, false, st);
      ETD_TRY(launch_bt_tmean_bwd(d->tacc, d->dtm, S, d->dtf, st));
    } else {
      HIP_TRY(hipMemsetAsync(d->dtf, 0, (size_t)F * 256 * 4, st));
    }
    // ---- beat head
    BT_GEMM(ETD_TG_TN, nt, 256, F, d->dz, nt, d->hm, 256, nullptr, G + d->ow, 256, true, st);
    ETD_TRY(launch_bt_colsum(d->dz, nt, F, nt, d->cpart, G + d->ob, st));
    BT_GEMM(ETD_TG_NN, F, 256, nt, d->dz, nt, P + d->ow, 256, nullptr, d->dhm, 256, false, st);
    ETD_TRY(launch_bt_hmean_bwd(d->xL, d->dhm, S, d->dx, st));
    HIP_TRY(hipGetLastError());
    int il = (int)d->il.size();
    for (int l = L - 1; l >= 0; --l) {
      if (l >= 3 && l <= 5) {
        --il;
        const BInstr& z = d->il[il];
        const BSavedI& b = d->si[il];
        ETD_TRY(ffn_backward(d, R, 1, b.xat, b.m2, b.r2, b.pre, P, G, d->dx, z.n2w, z.n2b, z.l1w, z.l1b, z.l2w, z.l2b, st));
        BT_GEMM(ETD_TG_TN, 256, 256, R, d->dx, 256, b.ao, 256, nullptr, G + z.out_w, 256, true, st);
        ETD_TRY(launch_bt_colsum(d->dx, 256, R, 256, d->cpart, G + z.out_b, st));
        BT_GEMM(ETD_TG_NN, R, 256, 256, d->dx, 256, P + z.out_w, 256, nullptr, d->dsk, 256, false, st);
        ETD_TRY(launch_bt_iattn_bwd(b.qkv, d->dsk, S, d->dqkv, st));
        ETD_TRY(proj_backward(d, R, b.xin, b.m1, b.r1, d->dqkv, P, G, d->dx, z.n1w, z.n1b, z.in_w, z.in_b, st));
      }
      const BTime& y = d->tl[l];
      const BSavedT& a = d->st[l];
      ETD_TRY(ffn_backward(d, R, 0, a.xat, a.m2, a.r2, a.pre, P, G, d->dx, y.n2w, y.n2b, y.l1w, y.l1b, y.l2w, y.l2b, st));
      ETD_TRY(launch_bt_dskip(d->dx, d->dtf, S, d->dsk, st));
      ETD_TRY(launch_bt_dattn_bwd(a.qkv, a.prob, d->dsk, S, P + y.Er, 1 << l, d->dl, d->dqkv, d->part, G + y.Er, st));
      ETD_TRY(proj_backward(d, R, a.xin, a.m1, a.r1, d->dqkv, P, G, d->dx, y.n1w, y.n1b, y.qkv_w, y.qkv_b, st));
    }
    // ---- conv front end: dx is the gradient of the tokens
    float* dc3 = d->dqkv;                              // [3 R][256] = [R][768]
    ETD_TRY(launch_bt_pool3_bwd(d->c3o, d->dx, R, dc3, st));
    ETD_TRY(launch_bt_conv_wgrad(256, BEAT_K3, 3 * R, dc3, d->x3, d->seg, d->dw3p, st));
    ETD_TRY(launch_bt_colsum(dc3, 256, 3 * R, 256, d->cpart, G + d->c3b, st));
    BT_GEMM(ETD_TG_NN, 3 * R, BEAT_K3, 256, dc3, 256, d->w3p, BEAT_K3, nullptr, d->big, BEAT_K3, false, st);
    ETD_TRY(launch_bt_repack(G + d->c3w, d->dw3p, 256, 64, 18, 1, st));
    float* dc2 = d->x3;                                // [24 R][64]: x3 [3 R][1152] has been read for the last time
    ETD_TRY(launch_bt_patch3_bwd(d->c2o, d->big, S, dc2, st));
    ETD_TRY(launch_bt_conv_wgrad(64, BEAT_K2, BEAT_C2_COLS * R, dc2, d->x2, d->seg, d->dw2p, st));
    ETD_TRY(launch_bt_colsum(dc2, 64, BEAT_C2_COLS * R, 64, d->cpart, G + d->c2b, st));
    BT_GEMM(ETD_TG_NN, BEAT_C2_COLS * R, BEAT_K2, 64, dc2, 64, d->w2p, BEAT_K2, nullptr, d->big, BEAT_K2, false, st);
    ETD_TRY(launch_bt_repack(G + d->c2w, d->dw2p, 64, 32, 12, 1, st));
    float* dc1 = d->x2;                                // [R][42][32]: the patches have been read for the last time
    ETD_TRY(launch_bt_fold2(d->big, d->c1, R, dc1, st));
    ETD_TRY(launch_bt_conv1_bwd(feat_dev, dc1, S, P + d->c1w, P + d->c1b, d->part, G + d->c1w, G + d->c1b, st));
    HIP_TRY(hipGetLastError());
  }
  d->h_cell.resize((size_t)F * nt);
  d->h_trow.assign(n_seq, 0.f);
  HIP_TRY(hipMemcpyAsync(d->h_cell.data(), d->cell, (size_t)F * nt * 4, hipMemcpyDeviceToHost, st));
  if (ntempo) HIP_TRY(hipMemcpyAsync(d->h_trow.data(), d->trow, (size_t)n_seq * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double tot = 0.0;
  for (int k = 0; k < nt; ++k) {                        // cells in frame order, class after class
    if (!cnt[k]) continue;
    double a = 0.0;
    for (int f = 0; f < F; ++f) a += (double)d->h_cell[(size_t)f * nt + k];
    tot += a / (double)cnt[k];
  }
  if (ntempo) {
    double a = 0.0;
    for (int s = 0; s < n_seq; ++s) a += (double)d->h_trow[s];
    tot += (double)c.tempo_weight * a / (double)ntempo;
  }
  *loss_out = (float)(tot * (double)loss_scale);
  return ETD_OK;
}

extern "C" int etd_btrain_zero_grad(etd_btrain* d, void* stream) {
  if (!d) ETD_FAIL(ETD_EINVAL, "etd_btrain_zero_grad: null handle");
  return d->ps.zero_grad(d->ps.n_total, (hipStream_t)stream);
}

extern "C" int etd_btrain_grad_norm(etd_btrain* d, double* norm, void* stream) {
  if (!d || !norm) ETD_FAIL(ETD_EINVAL, "etd_btrain_grad_norm: null argument");
  return d->ps.grad_norm(d->ps.n_total, (hipStream_t)stream, norm);
}

extern "C" int etd_btrain_step(etd_btrain* d, double max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, double* norm_out, void* stream) {
  if (!d) ETD_FAIL(ETD_EINVAL, "etd_btrain_step: null handle");
  return adamw_step(d->ps, d->ps.n_total, "etd_btrain_step", "btrain_optimizer", max_norm, lr, beta1, beta2, eps, weight_decay, norm_out, (hipStream_t)stream);
}

extern "C" int etd_btrain_set_step(etd_btrain* d, long long step) {
  if (!d || step < 0) ETD_FAIL(ETD_EINVAL, "etd_btrain_set_step: null handle or negative step");
  d->ps.step = step;
  return ETD_OK;
}
extern "C" long long etd_btrain_get_step(const etd_btrain* d) { return d ? d->ps.step : ETD_EINVAL; }

// which: 0 parameter, 1 gradient, 2 exp_avg, 3 exp_avg_sq
extern "C" int etd_btrain_read(etd_btrain* d, const char* name, int which, float* out_host, long long numel, void* stream) {
  if (!d || !name || !out_host || which < 0 || which > 3) ETD_FAIL(ETD_EINVAL, "etd_btrain: null argument or unknown buffer");
  return train_io(&d->ps, "etd_btrain", name, which, out_host, nullptr, numel, (hipStream_t)stream);
}
extern "C" int etd_btrain_write(etd_btrain* d, const char* name, int which, const float* in_host, long long numel, void* stream) {
  if (!d || !name || !in_host || which < 0 || which > 3) ETD_FAIL(ETD_EINVAL, "etd_btrain: null argument or unknown buffer");
  return train_io(&d->ps, "etd_btrain", name, which, nullptr, in_host, numel, (hipStream_t)stream);
}

// ================================================================================================
// debug entries (include/etude_hip_debug.h): every kernel and the two host pipelines on a caller's inputs, through the engine's own launchers
// ================================================================================================
namespace {
// the song tables of a tap: checked on the host, then uploaded to a block of its own (freed by the tap after its stream has drained)
struct TapSongs {
  BeatChunk S;
  int* dev = nullptr;
  int make(const char* who, int n_seq, const int64_t* T_host, int instr, hipStream_t st) {
    if (n_seq < 1 || n_seq > 65535 || !T_host) ETD_FAIL(ETD_EINVAL, "%s: n_seq = %d or no lengths", who, n_seq);
    if (instr < 1 || instr > 8) ETD_FAIL(ETD_EINVAL, "%s: instr = %d (1 .. 8)", who, instr);
    std::vector<int> tab(2 * (size_t)(n_seq + 1));
    long long rows = 0, frames = 0;
    for (int s = 0; s < n_seq; ++s) {
      if (T_host[s] < 1) ETD_FAIL(ETD_EINVAL, "%s: song %d has T = %lld", who, s, (long long)T_host[s]);
      tab[s] = (int)rows; tab[n_seq + 1 + s] = (int)frames;
      rows += T_host[s] * instr; frames += T_host[s];
      if (rows > (1 << 17)) ETD_FAIL(ETD_EINVAL, "%s: more than 2^17 rows", who);
    }
    tab[n_seq] = (int)rows; tab[2 * n_seq + 1] = (int)frames;
    HIP_TRY(hipMalloc((void**)&dev, tab.size() * 4));
    HIP_TRY(hipMemcpyAsync(dev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    S = beat_whole_call(dev, dev + n_seq + 1, n_seq, (int)rows, (int)frames, instr);
    return ETD_OK;
  }
  int done(int rc, hipStream_t st) {
    if (dev) { (void)hipStreamSynchronize(st); (void)hipFree(dev); dev = nullptr; }
    return rc;
  }
};
}  // namespace

extern "C" int etd_debug_btrain_dattn(int n_seq, const int64_t* T_host, int instr, int layer, const float* qkv_dev, const float* Er_dev, const float* xin_dev,
                                      const float* dO_dev, float* prob_dev, float* skip_dev, float* xout_dev, float* dl_dev, float* dqkv_dev, float* part_dev,
                                      float* dEr_dev, void* stream) {
  if (!qkv_dev || !Er_dev || !xin_dev || !prob_dev || !skip_dev || !xout_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_dattn: null forward argument");
  if (dO_dev && (!dl_dev || !dqkv_dev || !part_dev || !dEr_dev)) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_dattn: dO without dl, dqkv, part or dEr");
  if (layer < 0 || layer > 15) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_dattn: layer = %d (0 .. 15)", layer);
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_dattn", n_seq, T_host, instr, st));
  int rc = launch_beat_dattn_train(qkv_dev, t.S, Er_dev, 1 << layer, xin_dev, prob_dev, skip_dev, xout_dev, st);
  if (rc == ETD_OK && dO_dev) rc = launch_bt_dattn_bwd(qkv_dev, prob_dev, dO_dev, t.S, Er_dev, 1 << layer, dl_dev, dqkv_dev, part_dev, dEr_dev, st);
  return t.done(rc, st);
}

extern "C" int etd_debug_btrain_iattn(int n_seq, const int64_t* T_host, int instr, const float* qkv_dev, const float* dao_dev, float* ao_dev, float* dqkv_dev, void* stream) {
  if (!qkv_dev || !ao_dev || (dao_dev && !dqkv_dev)) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_iattn: null argument");
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_iattn", n_seq, T_host, instr, st));
  int rc = launch_beat_iattn(qkv_dev, t.S, ao_dev, st);
  if (rc == ETD_OK && dao_dev) rc = launch_bt_iattn_bwd(qkv_dev, dao_dev, t.S, dqkv_dev, st);
  return t.done(rc, st);
}

extern "C" int etd_debug_btrain_fold2(int rows, const float* dpatch_dev, const float* c1_dev, float* dc1_dev, void* stream) {
  if (rows < 1 || rows > (1 << 17) || !dpatch_dev || !c1_dev || !dc1_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_fold2: rows = %d (1 .. 2^17) or a null argument", rows);
  return launch_bt_fold2(dpatch_dev, c1_dev, rows, dc1_dev, (hipStream_t)stream);
}

extern "C" int etd_debug_btrain_conv1_bwd(int n_seq, const int64_t* T_host, int instr, const float* feat_dev, const float* dc1_dev, const float* w_dev, const float* b_dev,
                                          float* part_dev, float* dw_dev, float* db_dev, void* stream) {
  if (!feat_dev || !dc1_dev || !w_dev || !b_dev || !part_dev || !dw_dev || !db_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_conv1_bwd: null argument");
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_conv1_bwd", n_seq, T_host, instr, st));
  return t.done(launch_bt_conv1_bwd(feat_dev, dc1_dev, t.S, w_dev, b_dev, part_dev, dw_dev, db_dev, st), st);
}

extern "C" int etd_debug_btrain_bce(const float* z_dev, const float* y_dev, const float* pos_weight_dev, const float* coef_dev, int frames, int ntoken, float* cell_dev,
                                    float* dz_dev, void* stream) {
  if (frames < 1 || ntoken < 1 || ntoken > 64 || !z_dev || !y_dev || !pos_weight_dev || !coef_dev || !cell_dev || !dz_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_bce: frames = %d, ntoken = %d (1 .. 64) or a null argument", frames, ntoken);
  return launch_bt_bce(z_dev, y_dev, pos_weight_dev, coef_dev, frames, ntoken, cell_dev, dz_dev, (hipStream_t)stream);
}

extern "C" int etd_debug_btrain_tempo_ce(const float* t_dev, const float* p_dev, const int32_t* has_dev, float coef, int n, float* row_dev, float* dt_dev, void* stream) {
  if (n < 1 || n > 65535 || !t_dev || !p_dev || !has_dev || !row_dev || !dt_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_tempo_ce: n = %d (1 .. 65535) or a null argument", n);
  return launch_bt_tempo_ce(t_dev, p_dev, has_dev, coef, n, BT_TEMPO, row_dev, dt_dev, (hipStream_t)stream);
}

// what 0: the gradient of the front end's tokens [rows][256]; 1: the logits [frames][ntoken]; 2: the gradient of conv1's pooled output [rows][42][32] -- of the last call that ran
extern "C" int etd_debug_btrain_read_rows(etd_btrain* d, int what, float* out_host, long long numel, void* stream) {
  if (!d || !out_host || what < 0 || what > 2) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_read_rows: null argument or what = %d (0 .. 2)", what);
  if (d->last_rows < 1) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_read_rows: no call has run");
  const long long n = what == 0 ? (long long)d->last_rows * 256 : what == 1 ? (long long)d->last_frames * d->cfg.ntoken : (long long)d->last_rows * BEAT_W1 * BEAT_C1;
  if (numel != n) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_read_rows: the buffer holds %lld floats, the last call left %lld", numel, n);
  const float* src = what == 0 ? d->dx : what == 1 ? d->logits : d->x2;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(out_host, src, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}

// which 0: conv1 (in = feat, w, b); 1: conv2's patches (in = c1); 2: conv3's patches (in = c2); 3: pool3 (in = c3)
extern "C" int etd_debug_btrain_front_fwd(int which, int n_seq, const int64_t* T_host, int instr, const float* in_dev, const float* w_dev, const float* b_dev, float* out_dev,
                                          void* stream) {
  if (which < 0 || which > 3 || !in_dev || !out_dev || (which == 0 && (!w_dev || !b_dev))) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_front_fwd: which = %d (0 .. 3) or a null argument", which);
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_front_fwd", n_seq, T_host, instr, st));
  const int rc = which == 0 ? launch_beat_conv1(in_dev, t.S, w_dev, b_dev, out_dev, st) : which == 1 ? launch_bt_patch2(in_dev, t.S.rows, out_dev, st)
               : which == 2 ? launch_beat_patch3(in_dev, BEAT_C2_COLS, t.S, out_dev, st) : launch_beat_pool3(in_dev, t.S.rows, out_dev, st);
  return t.done(rc, st);
}

// which 0: pool3 backward (c = c3, g = dx -> dc3); 1: patch3 backward (c = c2, g = dx3 -> dc2)
extern "C" int etd_debug_btrain_front_bwd(int which, int n_seq, const int64_t* T_host, int instr, const float* c_dev, const float* g_dev, float* out_dev, void* stream) {
  if (which < 0 || which > 1 || !c_dev || !g_dev || !out_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_front_bwd: which = %d (0 .. 1) or a null argument", which);
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_front_bwd", n_seq, T_host, instr, st));
  return t.done(which == 0 ? launch_bt_pool3_bwd(c_dev, g_dev, t.S.rows, out_dev, st) : launch_bt_patch3_bwd(c_dev, g_dev, t.S, out_dev, st), st);
}

extern "C" int etd_debug_btrain_repack(int dir, int co, int ci, int kk, float* native_dev, float* packed_dev, void* stream) {
  if (dir < 0 || dir > 1 || co < 1 || ci < 1 || kk < 1 || (long long)co * ci * kk > (1 << 24) || !native_dev || !packed_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_repack: dir = %d (0, 1), co x ci x kk = %d x %d x %d (each >= 1, at most 2^24 elements) or a null argument", dir, co, ci, kk);
  return launch_bt_repack(native_dev, packed_dev, co, ci, kk, dir, (hipStream_t)stream);
}

extern "C" int etd_debug_btrain_colsum(const float* dy_dev, int ld, int M, int N, float* part_dev, float* out_dev, void* stream) {
  if (M < 1 || M > BEAT_C2_COLS * (1 << 17) || N < 1 || N > 8192 || ld < N || !dy_dev || !part_dev || !out_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_colsum: M = %d (1 .. 24 x 2^17), N = %d (1 .. 8192), ld = %d (>= N) or a null argument", M, N, ld);
  return launch_bt_colsum(dy_dev, ld, M, N, part_dev, out_dev, (hipStream_t)stream);
}

extern "C" int etd_debug_btrain_slice_sum(const float* part_dev, int n_slices, int width, float* out_dev, void* stream) {
  if (n_slices < 1 || n_slices > (1 << 17) || width < 1 || width > (1 << 24) || !part_dev || !out_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_slice_sum: n_slices = %d (1 .. 2^17), width = %d (1 .. 2^24) or a null argument", n_slices, width);
  return launch_bt_slice_sum(part_dev, n_slices, width, out_dev, (hipStream_t)stream);
}

// which 0: skipacc (a = skip -> tacc, first_layer 0 / 1); 1: dskip (a = dx, b = dtf -> dsk); 2: hmean (a = x -> hm); 3: hmean_bwd (a = x, b = dhm -> dx);
// 4: tmean (a = tacc -> tm); 5: tmean_bwd (a = tacc, b = dtm -> dtf)
extern "C" int etd_debug_btrain_means(int which, int n_seq, const int64_t* T_host, int instr, const float* a_dev, const float* b_dev, int first_layer, float* out_dev,
                                      void* stream) {
  const bool two = which == 1 || which == 3 || which == 5;
  if (which < 0 || which > 5 || !a_dev || !out_dev || (two && !b_dev) || first_layer < 0 || first_layer > 1)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_means: which = %d (0 .. 5), first_layer = %d (0, 1) or a null argument", which, first_layer);
  hipStream_t st = (hipStream_t)stream;
  TapSongs t;
  ETD_TRY(t.make("etd_debug_btrain_means", n_seq, T_host, instr, st));
  int rc;
  switch (which) {
    case 0: rc = launch_beat_skipacc(a_dev, t.S, first_layer, out_dev, st); break;
    case 1: rc = launch_bt_dskip(a_dev, b_dev, t.S, out_dev, st); break;
    case 2: rc = launch_bt_hmean(a_dev, t.S, out_dev, st); break;
    case 3: rc = launch_bt_hmean_bwd(a_dev, b_dev, t.S, out_dev, st); break;
    case 4: rc = launch_bt_tmean(a_dev, t.S, out_dev, st); break;
    default: rc = launch_bt_tmean_bwd(a_dev, b_dev, t.S, out_dev, st); break;
  }
  return t.done(rc, st);
}

// y = relu(x) (y may be NULL); then dy = x > 0 ? dy : 0 in place (dy may be NULL); at least one of them
extern "C" int etd_debug_btrain_relu(const float* x_dev, long long n, float* y_dev, float* dy_dev, void* stream) {
  if (n < 1 || n > (1LL << 31) || !x_dev || (!y_dev && !dy_dev)) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_relu: n = %lld (1 .. 2^31) or a null argument", n);
  hipStream_t st = (hipStream_t)stream;
  if (y_dev) ETD_TRY(launch_bt_relu(x_dev, y_dev, n, st));
  if (dy_dev) ETD_TRY(launch_bt_relu_bwd(x_dev, dy_dev, n, st));
  return ETD_OK;
}

extern "C" int etd_debug_btrain_conv_wgrad(int M, int N, int K, const float* dY_dev, const float* X_dev, float* seg_dev, float* dw_dev, void* stream) {
  if (M < 1 || N < 1 || K < 1 || K > BEAT_C2_COLS * (1 << 17) || (long long)M * N > (1 << 24) || !dY_dev || !X_dev || !seg_dev || !dw_dev)
    ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_conv_wgrad: M x N = %d x %d (each >= 1, at most 2^24 elements), K = %d (1 .. 24 x 2^17) or a null argument", M, N, K);
  return launch_bt_conv_wgrad(M, N, K, dY_dev, X_dev, seg_dev, dw_dev, (hipStream_t)stream);
}

// P_dev / G_dev: gain [256] | bias [256] | linear1.weight [H][256] | linear1.bias [H] | linear2.weight [256][H] | linear2.bias [256], H = the handle's d_hid
extern "C" int etd_debug_btrain_ffn_bwd(etd_btrain* d, int R, int act, const float* x_dev, const float* mean_dev, const float* rstd_dev, const float* pre_dev, const float* P_dev,
                                        float* G_dev, float* dx_dev, void* stream) {
  if (!d || !x_dev || !mean_dev || !rstd_dev || !pre_dev || !P_dev || !G_dev || !dx_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_ffn_bwd: null argument");
  if (R < 1 || R > d->cfg.max_rows || act < 0 || act > 1) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_ffn_bwd: R = %d (1 .. max_rows = %d) or act = %d (0, 1)", R, d->cfg.max_rows, act);
  const size_t H = (size_t)d->cfg.d_hid, l1w = 512, l1b = l1w + H * 256, l2w = l1b + H, l2b = l2w + 256 * H;
  return ffn_backward(d, R, act, x_dev, mean_dev, rstd_dev, pre_dev, P_dev, G_dev, dx_dev, 0, 256, l1w, l1b, l2w, l2b, (hipStream_t)stream);
}

// P_dev / G_dev: gain [256] | bias [256] | weight [768][256] | bias [768]
extern "C" int etd_debug_btrain_proj_bwd(etd_btrain* d, int R, const float* x_dev, const float* mean_dev, const float* rstd_dev, const float* dqkv_dev, const float* P_dev,
                                         float* G_dev, float* dx_dev, void* stream) {
  if (!d || !x_dev || !mean_dev || !rstd_dev || !dqkv_dev || !P_dev || !G_dev || !dx_dev) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_proj_bwd: null argument");
  if (R < 1 || R > d->cfg.max_rows) ETD_FAIL(ETD_EINVAL, "etd_debug_btrain_proj_bwd: R = %d (1 .. max_rows = %d)", R, d->cfg.max_rows);
  return proj_backward(d, R, x_dev, mean_dev, rstd_dev, dqkv_dev, P_dev, G_dev, dx_dev, 0, 256, 512, 512 + 768 * 256, (hipStream_t)stream);
}
