// Beat-Transformer engine: Demixed_DilatedTransformerModel.forward (etude/models/beat_transformer.py:56-106, layers/dilated_transformer_layer.py:37-180) in the
// exact-parity arithmetic of csrc/gemm3.h.  Rows are (song, instr, t): song s owns the row block [row0_s, row0_s + instr T_s) laid out [instr][T_s], as its features
// [instr][T_s][128] arrive; frames are (song, t).  Every kernel computes a row (or a frame, or a song) from that row's own inputs in a fixed order, and every GEMM is
// k_gemm3 (one path for every row count: its per-row arithmetic does not depend on M or on the tile a row falls in), so a song's outputs are bit-identical alone, inside
// any ragged batch and across chunks.  DESIGN.md "Beat-Transformer engine" has the bounds, the layout and the FLOP formula.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "beat.h"
#include "etude_hip.h"
#include "etude_hip_debug.h"
#include "prof.h"

// ================================================================================================ conv1 + maxpool(1,3) + ReLU
// c1[r][p][co] = relu(max_{u<3} (b[co] + sum_{kt<5,kw<3} w[co][kt][kw] x[t+kt-2][3p+u+kw])), x = 0 outside the song (padding (2, 0)).  Channel-last, so that the
// conv2 patch of pooled column c is the 384 contiguous floats at (r 42 + c) 32.  One thread per (row, p, co).
// (feat points at the chunk's first row)
// The chain is written out here and once more as beat_conv1_at (beat.h), which the trainer's k_bt_conv1_bwd calls to find the maximum this kernel took: the same
// fmaf order, bias first, kt then kw ascending.  Calling the helper from here folds the row offsets differently (3 more instructions), so this body stays as written.
__global__ __launch_bounds__(256) void k_beat_conv1(const float* __restrict__ feat, BeatChunk c, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ c1) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)c.rows * BEAT_W1 * BEAT_C1) return;
  const int r = (int)(gid / (BEAT_W1 * BEAT_C1)), rem = (int)(gid - (long long)r * (BEAT_W1 * BEAT_C1)), p = rem / BEAT_C1, co = rem - p * BEAT_C1;
  const int g = r + c.row_base, s = beat_song_of(c.row0, c.first, c.count, g);
  const int T = (c.frame0[s + 1] - c.frame0[s]), q = g - c.row0[s], t = q % T;
  float wr[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) wr[k] = w[co * 15 + k];
  float m = -INFINITY;
#pragma unroll 1
  for (int u = 0; u < 3; ++u) {            // one serial fmaf chain at a time (three unrolled chains become packed-FP32 FMAs: tests/test_isa_guard.py)
    float acc = b[co];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
      const int tt = t + kt - 2;
      if (tt < 0 || tt >= T) continue;
      const float* xr = feat + (long long)(r + kt - 2) * BEAT_MELS + 3 * p + u;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc = fmaf(wr[kt * 3 + kw], xr[kw], acc);
    }
    m = fmaxf(m, acc);
  }
  c1[gid] = fmaxf(m, 0.f);
}

// ================================================================================================ conv2 maxpool + ReLU -> conv3 patches
// c2 = conv2 + bias over COLS columns of every row ([r COLS + col][64]: the engine's GEMM forms all 42, the trainer's the 24 that are read);
// X3[r 3 + c][kt 384 + kw 64 + ci] = relu(max_{u<3} c2[(r+kt-1) COLS + 3 (c+kw) + u][ci]), 0 where the row r+kt-1 is outside the song (conv3 padding (1, 0)).
// One thread per X3 element.
template <int COLS>
__global__ __launch_bounds__(256) void k_beat_patch3(const float* __restrict__ c2, BeatChunk c, float* __restrict__ x3) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)c.rows * 3 * BEAT_K3) return;
  const int rc = (int)(gid / BEAT_K3), k = (int)(gid - (long long)rc * BEAT_K3);
  const int r = rc / 3, col = rc - r * 3, kt = k / 384, kw = (k - kt * 384) / 64, ci = k & 63;
  int s, T, t;
  beat_row_at(c, r, s, T, t);
  const int tt = t + kt - 1;
  float v = 0.f;
  if (tt >= 0 && tt < T) {
    const float* p = c2 + ((long long)(r + kt - 1) * COLS + 3 * (col + kw)) * BEAT_C2 + ci;
    v = beat_pool3_relu(p[0], p[BEAT_C2], p[2 * BEAT_C2]);
  }
  x3[gid] = v;
}

// conv3 maxpool + ReLU: x[r][co] = relu(max_{c<3} c3[r 3 + c][co])
__global__ __launch_bounds__(256) void k_beat_pool3(const float* __restrict__ c3, int rows, float* __restrict__ x) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)rows * BEAT_DMODEL) return;
  const int r = (int)(gid >> 8), co = (int)(gid & 255);
  const float* p = c3 + (long long)r * 3 * BEAT_DMODEL + co;
  x[gid] = beat_pool3_relu(p[0], p[BEAT_DMODEL], p[2 * BEAT_DMODEL]);
}

// ================================================================================================ dilated 5-tap attention (dilated_transformer_layer.py:37-95)
// One thread per (row, head).  Tap j of head h reads the row at time t + o_h(j) 2^layer of the same (song, instr): o = j-2 (heads 0-3), j-4 (4), j-3 (5), j-1 (6), j (7);
// head 7 takes its KEYS from head 6's projection (:51) and its values from its own.  logit = (q.k_j + q.Er[h][:, j]) / sqrt(32); a tap outside the song is masked
// (the reference masks qk == 0 of its zero-padded keys).  out = sum_j p_j v_j is the layer's skip; x += out.
// One body, two instances.  The engine's (TRAIN = false) updates x in place through the one restrict pointer x.  The trainer's reads the layer's input from keep.xin,
// writes x = xin + out out of place and keeps the probabilities in keep.prob [rows][8][5] (0 for a masked tap).  What only the trainer passes travels in `keep`, which
// is empty for the engine, so that the engine's arguments and code are what they were before the trainer shared the kernel.
template <bool TRAIN> struct BeatDattnKeep {};
template <> struct BeatDattnKeep<true> { const float* xin; float* prob; };
template <bool TRAIN>
__global__ __launch_bounds__(256) void k_beat_dattn(const float* __restrict__ qkv, BeatChunk c, const float* __restrict__ Er, int dil, float* __restrict__ skip, float* __restrict__ x,
                                                    BeatDattnKeep<TRAIN> keep) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)c.rows * BEAT_HEADS) return;
  const int r = (int)(gid >> 3), h = (int)(gid & 7), kh = h == 7 ? 6 : h;
  const int g = r + c.row_base, s = beat_song_of(c.row0, c.first, c.count, g);
  const int T = (c.frame0[s + 1] - c.frame0[s]), t = (g - c.row0[s]) % T;
  const float* qp = qkv + (long long)r * 768 + h * BEAT_HEAD_DIM;
  float q[BEAT_HEAD_DIM];
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; d += 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(qp + d); q[d] = v[0]; q[d + 1] = v[1]; q[d + 2] = v[2]; q[d + 3] = v[3]; }
  const float* er = Er + h * BEAT_HEAD_DIM * BEAT_TAPS;        // [32][5]
  float lg[BEAT_TAPS];
  bool ok[BEAT_TAPS];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) {
    const int o = beat_tap_off(h, j) * dil, tt = t + o;
    ok[j] = tt >= 0 && tt < T;
    float qk = 0.f, qe = 0.f;
#pragma unroll
    for (int d = 0; d < BEAT_HEAD_DIM; ++d) qe = fmaf(q[d], er[d * BEAT_TAPS + j], qe);
    if (ok[j]) {
      const float* kp = qkv + (long long)(r + o) * 768 + 256 + kh * BEAT_HEAD_DIM;
#pragma unroll
      for (int d = 0; d < BEAT_HEAD_DIM; d += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(kp + d);
        qk = fmaf(q[d], v[0], qk); qk = fmaf(q[d + 1], v[1], qk); qk = fmaf(q[d + 2], v[2], qk); qk = fmaf(q[d + 3], v[3], qk);
      }
    }
    lg[j] = (qk + qe) / 5.656854249492380195f;
    if (ok[j]) mx = fmaxf(mx, lg[j]);
  }
  float den = 0.f;
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) { lg[j] = ok[j] ? expf(lg[j] - mx) : 0.f; den += lg[j]; }
  float o[BEAT_HEAD_DIM];
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < BEAT_TAPS; ++j) {
    if constexpr (TRAIN) keep.prob[gid * BEAT_TAPS + j] = ok[j] ? lg[j] / den : 0.f;
    if (!ok[j]) continue;
    const float p = lg[j] / den;
    const float* vp = qkv + (long long)(r + beat_tap_off(h, j) * dil) * 768 + 512 + h * BEAT_HEAD_DIM;
#pragma unroll
    for (int d = 0; d < BEAT_HEAD_DIM; d += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(vp + d);
      o[d] = fmaf(p, v[0], o[d]); o[d + 1] = fmaf(p, v[1], o[d + 1]); o[d + 2] = fmaf(p, v[2], o[d + 2]); o[d + 3] = fmaf(p, v[3], o[d + 3]);
    }
  }
  float* sp = skip + (long long)r * BEAT_DMODEL + h * BEAT_HEAD_DIM;
  float* xp = x + (long long)r * BEAT_DMODEL + h * BEAT_HEAD_DIM;
  const float* xi = xp;
  if constexpr (TRAIN) xi = keep.xin + (long long)r * BEAT_DMODEL + h * BEAT_HEAD_DIM;
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; d += 4) {
    const f32x4 ov = {o[d], o[d + 1], o[d + 2], o[d + 3]};
    *reinterpret_cast<f32x4*>(sp + d) = ov;
    f32x4 xv = *reinterpret_cast<const f32x4*>(xi + d);
    xv[0] = xv[0] + ov[0]; xv[1] = xv[1] + ov[1]; xv[2] = xv[2] + ov[2]; xv[3] = xv[3] + ov[3];
    *reinterpret_cast<f32x4*>(xp + d) = xv;
  }
}
// per-layer skip into the tempo accumulator: tacc[f][d] (+)= (sum_i skip[row(i, f)][d]) / instr   (beat_transformer.py:82-84, 101), layers added in order
__global__ __launch_bounds__(256) void k_beat_skipacc(const float* __restrict__ skip, BeatChunk c, int first_layer, float* __restrict__ tacc) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)c.frames * BEAT_DMODEL) return;
  const int fl = (int)(gid >> 8), d = (int)(gid & 255);
  int s, T, rb;
  beat_frame_at(c, fl, s, T, rb);
  float sum = 0.f;
  for (int i = 0; i < c.instr; ++i) sum += skip[(long long)(rb + i * T) * BEAT_DMODEL + d];
  const float m = sum / (float)c.instr;
  tacc[gid] = first_layer ? m : tacc[gid] + m;
}

// ================================================================================================ instrument attention (torch TransformerEncoderLayer self-attention)
// 8-head attention over the instr rows of one frame, no mask; one thread per (frame, head, query instr); qkv = in_proj output [row][q|k|v].
// (Loads, dots and axpys are written out, as in k_beat_dattn: on beat.h's helpers the compiler schedules both kernels differently.  The order of operations per
// query is that of beat_dot32 / beat_axpy32, which the trainer's k_bt_iattn_bwd uses to recompute this softmax.)
__global__ __launch_bounds__(256) void k_beat_iattn(const float* __restrict__ qkv, BeatChunk c, float* __restrict__ ao) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int ni = c.instr;
  if (gid >= (long long)c.frames * BEAT_HEADS * ni) return;
  const int fl = (int)(gid / (BEAT_HEADS * ni)), rem = (int)(gid - (long long)fl * (BEAT_HEADS * ni)), h = rem / ni, iq = rem - h * ni;
  const int gf = fl + c.frame_base, s = beat_song_of(c.frame0, c.first, c.count, gf);
  const int T = c.frame0[s + 1] - c.frame0[s], t = gf - c.frame0[s], rb = c.row0[s] - c.row_base + t;
  const float* qp = qkv + (long long)(rb + iq * T) * 768 + h * BEAT_HEAD_DIM;
  float q[BEAT_HEAD_DIM];
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; d += 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(qp + d); q[d] = v[0]; q[d + 1] = v[1]; q[d + 2] = v[2]; q[d + 3] = v[3]; }
  float lg[8];
  float mx = -INFINITY;
  for (int j = 0; j < ni; ++j) {
    const float* kp = qkv + (long long)(rb + j * T) * 768 + 256 + h * BEAT_HEAD_DIM;
    float qk = 0.f;
#pragma unroll
    for (int d = 0; d < BEAT_HEAD_DIM; d += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(kp + d);
      qk = fmaf(q[d], v[0], qk); qk = fmaf(q[d + 1], v[1], qk); qk = fmaf(q[d + 2], v[2], qk); qk = fmaf(q[d + 3], v[3], qk);
    }
    lg[j] = qk / 5.656854249492380195f;
    mx = fmaxf(mx, lg[j]);
  }
  float den = 0.f;
  for (int j = 0; j < ni; ++j) { lg[j] = expf(lg[j] - mx); den += lg[j]; }
  float o[BEAT_HEAD_DIM];
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; ++d) o[d] = 0.f;
  for (int j = 0; j < ni; ++j) {
    const float p = lg[j] / den;
    const float* vp = qkv + (long long)(rb + j * T) * 768 + 512 + h * BEAT_HEAD_DIM;
#pragma unroll
    for (int d = 0; d < BEAT_HEAD_DIM; d += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(vp + d);
      o[d] = fmaf(p, v[0], o[d]); o[d + 1] = fmaf(p, v[1], o[d + 1]); o[d + 2] = fmaf(p, v[2], o[d + 2]); o[d + 3] = fmaf(p, v[3], o[d + 3]);
    }
  }
  float* op = ao + (long long)(rb + iq * T) * BEAT_DMODEL + h * BEAT_HEAD_DIM;
#pragma unroll
  for (int d = 0; d < BEAT_HEAD_DIM; d += 4) { const f32x4 ov = {o[d], o[d + 1], o[d + 2], o[d + 3]}; *reinterpret_cast<f32x4*>(op + d) = ov; }
}

// ================================================================================================ heads (beat_transformer.py:99-106)
// beat: logits[f][k] = b[k] + W[k] . mean_i relu(x[row(i, f)]); one wave per frame, 4 features per lane, fixed-order wave sums
__global__ __launch_bounds__(256) void k_beat_head(const float* __restrict__ x, BeatChunk c, const float* __restrict__ W, const float* __restrict__ b, int ntoken, float* __restrict__ logits) {
  const int fl = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (fl >= c.frames) return;
  const int gf = fl + c.frame_base, s = beat_song_of(c.frame0, c.first, c.count, gf);
  const int T = c.frame0[s + 1] - c.frame0[s], t = gf - c.frame0[s], rb = c.row0[s] - c.row_base + t;
  float hm[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < c.instr; ++i) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + (long long)(rb + i * T) * BEAT_DMODEL + lane * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) hm[e] += fmaxf(v[e], 0.f);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) hm[e] = hm[e] / (float)c.instr;
  for (int k = 0; k < ntoken; ++k) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(W + k * BEAT_DMODEL + lane * 4);
    float a = w[0] * hm[0];
    a = fmaf(w[1], hm[1], a); a = fmaf(w[2], hm[2], a); a = fmaf(w[3], hm[3], a);
    a = wave_sum(a);
    if (lane == 0) logits[(long long)gf * ntoken + k] = a + b[k];
  }
}

// tempo, stage 1: part[seg0[s] - seg0[first] + seg][d] = sum over the song's frames [seg 128, + 128) of relu(tacc[f][d]) in frame order
__global__ __launch_bounds__(256) void k_beat_tempo_part(const float* __restrict__ tacc, BeatChunk c, float* __restrict__ part) {
  const int seg = blockIdx.x, sl = blockIdx.y, s = c.first + sl, d = threadIdx.x;
  const int T = c.frame0[s + 1] - c.frame0[s], f0 = seg * BEAT_SEG;
  if (f0 >= T) return;
  const int f1 = f0 + BEAT_SEG < T ? f0 + BEAT_SEG : T;
  const float* p = tacc + (long long)(c.frame0[s] - c.frame_base) * BEAT_DMODEL + d;
  float sum = 0.f;
  for (int f = f0; f < f1; ++f) sum += fmaxf(p[(long long)f * BEAT_DMODEL], 0.f);
  part[((long long)(c.seg0[s] - c.seg0[c.first]) + seg) * BEAT_DMODEL + d] = sum;
}
// tempo, stage 2: m = (sum of the song's parts in order) / T; out[s][j] = bt[j] + Wt[j] . m   (one workgroup per song)
__global__ __launch_bounds__(256) void k_beat_tempo(const float* __restrict__ part, BeatChunk c, const float* __restrict__ Wt, const float* __restrict__ bt, int n_out,
                                                    float* __restrict__ tempo) {
  __shared__ float m[BEAT_DMODEL];
  const int sl = blockIdx.x, s = c.first + sl, d = threadIdx.x;
  const int T = c.frame0[s + 1] - c.frame0[s], nseg = (T + BEAT_SEG - 1) / BEAT_SEG;
  float sum = 0.f;
  const float* pp = part + (long long)(c.seg0[s] - c.seg0[c.first]) * BEAT_DMODEL + d;
  for (int g = 0; g < nseg; ++g) sum += pp[(long long)g * BEAT_DMODEL];
  m[d] = sum / (float)T;
  __syncthreads();
  for (int j = d; j < n_out; j += 256) {
    const float* w = Wt + (long long)j * BEAT_DMODEL;
    float a = 0.f;
    for (int k = 0; k < BEAT_DMODEL; ++k) a = fmaf(w[k], m[k], a);
    tempo[(long long)s * n_out + j] = a + bt[j];
  }
}

// ================================================================================================ launchers of the stages shared with the trainer (beat.h)
static inline unsigned nblk(long long threads) { return (unsigned)((threads + 255) / 256); }

int launch_beat_conv1(const float* feat, const BeatChunk& c, const float* w, const float* b, float* c1, hipStream_t st) {
  ProfScope ps("k_beat_conv1", st, (double)c.rows * BEAT_W1 * BEAT_C1 * 3 * 15 * 2, (double)c.rows * (BEAT_MELS * 4 + BEAT_W1 * BEAT_C1 * 4));
  hipLaunchKernelGGL(k_beat_conv1, dim3(nblk((long long)c.rows * BEAT_W1 * BEAT_C1)), dim3(256), 0, st, feat, c, w, b, c1);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_beat_patch3(const float* c2, int c2_cols, const BeatChunk& c, float* x3, hipStream_t st) {
  if (c2_cols != BEAT_W1 && c2_cols != BEAT_C2_COLS) ETD_FAIL(ETD_EINVAL, "launch_beat_patch3: c2 of %d columns (%d or %d)", c2_cols, BEAT_W1, BEAT_C2_COLS);
  ProfScope ps("k_beat_patch3", st, 0.0, (double)c.rows * 3 * BEAT_K3 * 4 * 2);
  const dim3 grid(nblk((long long)c.rows * 3 * BEAT_K3));
  if (c2_cols == BEAT_W1) hipLaunchKernelGGL(k_beat_patch3<BEAT_W1>, grid, dim3(256), 0, st, c2, c, x3);
  else hipLaunchKernelGGL(k_beat_patch3<BEAT_C2_COLS>, grid, dim3(256), 0, st, c2, c, x3);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_beat_pool3(const float* c3, int rows, float* x, hipStream_t st) {
  ProfScope ps("k_beat_pool3", st, 0.0, (double)rows * 4 * 256 * 4);
  hipLaunchKernelGGL(k_beat_pool3, dim3(nblk((long long)rows * 256)), dim3(256), 0, st, c3, rows, x);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
#define BEAT_DATTN_SCOPE ProfScope ps("k_beat_dattn", st, (double)c.rows * BEAT_HEADS * BEAT_TAPS * BEAT_HEAD_DIM * 6, (double)c.rows * (768 * 4 * 3 + 256 * 4 * 3))
int launch_beat_dattn(const float* qkv, const BeatChunk& c, const float* Er, int dil, float* skip, float* x, hipStream_t st) {
  BEAT_DATTN_SCOPE;
  hipLaunchKernelGGL(k_beat_dattn<false>, dim3(nblk((long long)c.rows * BEAT_HEADS)), dim3(256), 0, st, qkv, c, Er, dil, skip, x, BeatDattnKeep<false>{});
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_beat_dattn_train(const float* qkv, const BeatChunk& c, const float* Er, int dil, const float* xin, float* prob, float* skip, float* xout, hipStream_t st) {
  BEAT_DATTN_SCOPE;
  hipLaunchKernelGGL(k_beat_dattn<true>, dim3(nblk((long long)c.rows * BEAT_HEADS)), dim3(256), 0, st, qkv, c, Er, dil, skip, xout, BeatDattnKeep<true>{xin, prob});
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_beat_skipacc(const float* skip, const BeatChunk& c, int first_layer, float* tacc, hipStream_t st) {
  ProfScope ps("k_beat_skipacc", st, (double)c.rows * 256, (double)c.rows * 256 * 4 + (double)c.frames * 256 * 8);
  hipLaunchKernelGGL(k_beat_skipacc, dim3(nblk((long long)c.frames * 256)), dim3(256), 0, st, skip, c, first_layer, tacc);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}
int launch_beat_iattn(const float* qkv, const BeatChunk& c, float* ao, hipStream_t st) {
  ProfScope ps("k_beat_iattn", st, (double)c.rows * BEAT_HEADS * c.instr * BEAT_HEAD_DIM * 4, (double)c.rows * (768 * 4 * (1 + 2 * c.instr) / 1.0 + 256 * 4));
  hipLaunchKernelGGL(k_beat_iattn, dim3(nblk((long long)c.frames * BEAT_HEADS * c.instr)), dim3(256), 0, st, qkv, c, ao);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// ================================================================================================ host: the engine
namespace {

struct TimeLayer { float *ln1g, *ln1b, *ln2g, *ln2b, *Er; G3Lin qkv, l1, l2; };
struct InstrLayer { float *ln1g, *ln1b, *ln2g, *ln2b; G3Lin inp, outp, l1, l2; };
// the checkpoint's tensors of one layer (host pointers into the caller's arrays)
struct TimeHostW { const float *Wq[3], *bq[3], *Er, *W1, *c1, *W2, *c2, *g1, *b1, *g2, *b2; };
struct InstrHostW { const float *Wi, *bi, *Wo, *bo, *W1, *c1, *W2, *c2, *g1, *b1, *g2, *b2; };

}  // namespace

struct etd_beat {
  etd_beat_cfg cfg;
  DevPool pool;                            // weights (freed in destroy)
  float *c1w = nullptr, *c1b = nullptr;
  G3Lin c2, c3;
  std::vector<TimeLayer> tl;
  std::vector<InstrLayer> il;              // for time layers 3 .. 5 (those below nlayers)
  float *ow = nullptr, *ob = nullptr, *tw = nullptr, *tb = nullptr;
  // workspace, sized for `cap_rows` rows (grown when one song alone needs more)
  long long cap_rows = 0;
  void* ws = nullptr;
  float *x = nullptr, *xa = nullptr, *qkv = nullptr, *skip = nullptr, *hid = nullptr, *c1 = nullptr, *c2o = nullptr, *x3 = nullptr, *c3o = nullptr, *tacc = nullptr, *part = nullptr;
  int* tab = nullptr; int tab_cap = 0;
  float *tap_front = nullptr, *tap_l0 = nullptr;     // etd_beat_debug_taps
  etd_debug_beat_taps st = {}; bool st_on = false;   // etd_beat_debug_stage_taps
};

namespace {

// launch_gemm3 at every row count, on purpose: the outputs are then bit-identical across batch layouts
int gemm(const G3Lin& L, const float* X, int M, int epi, float* Y, float* resid, hipStream_t st, int ldx = 0) {
  DGemmArgs a = g3_lin_args(L, X, ldx ? ldx : L.K, M);
  a.Y = Y; a.ldy = L.N;
  if (epi == DEPI_RESID) { a.hin = resid; a.hout = resid; a.add = nullptr; }
  return launch_gemm3(a, epi, st);
}

// per-row floats of the workspace: x, xa, skip (256 each), qkv 768, hid d_hid, conv1 42 x 32, conv2 42 x 64, conv3 patches 3 x 1152, conv3 out 3 x 256
size_t ws_row_floats(int d_hid) { return 3 * 256 + 768 + (size_t)d_hid + BEAT_W1 * BEAT_C1 + BEAT_W1 * BEAT_C2 + 3 * BEAT_K3 + 3 * 256; }

int ensure_ws(etd_beat* e, long long rows, int n_seq, hipStream_t st) {
  if (rows > e->cap_rows) {
    HIP_TRY(hipStreamSynchronize(st));
    if (e->ws) { (void)hipFree(e->ws); e->ws = nullptr; e->cap_rows = 0; }
    const size_t per = ws_row_floats(e->cfg.d_hid);
    // + frames (tacc: <= rows / instr frames, but a chunk of short songs can hold rows / instr rounded up per song: take rows) + tempo partial sums + slack for the
    // conv2 GEMM's overlapping rows (the last row reads 384 floats from its start)
    const long long maxseg = rows / e->cfg.instr / BEAT_SEG + rows / e->cfg.instr + 2;      // sum over a chunk's songs of ceil(T_s / 128) <= frames / 128 + songs
    const size_t floats = per * rows + 256 * (size_t)rows + 256 * (size_t)maxseg + 64 * 1024;
    HIP_TRY(hipMalloc(&e->ws, floats * 4));
    HIP_TRY(hipMemset(e->ws, 0, floats * 4));
    float* p = (float*)e->ws;
    auto take = [&](size_t n) { float* q = p; p += (n + 63) / 64 * 64; return q; };
    e->x = take(256 * rows); e->xa = take(256 * rows); e->skip = take(256 * rows); e->qkv = take(768 * rows); e->hid = take((size_t)e->cfg.d_hid * rows);
    e->c1 = take((size_t)BEAT_W1 * BEAT_C1 * rows + 1024); e->c2o = take((size_t)BEAT_W1 * BEAT_C2 * rows); e->x3 = take((size_t)3 * BEAT_K3 * rows);
    e->c3o = take((size_t)3 * 256 * rows); e->tacc = take(256 * (size_t)rows); e->part = take(256 * (size_t)maxseg);
    e->cap_rows = rows;
  }
  if (3 * (n_seq + 1) > e->tab_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    if (e->tab) (void)hipFree(e->tab);
    e->tab = nullptr;
    HIP_TRY(hipMalloc((void**)&e->tab, (size_t)3 * (n_seq + 1) * 4));
    e->tab_cap = 3 * (n_seq + 1);
  }
  return ETD_OK;
}

// the model on one chunk of whole songs
// (seg_base, segs: the chunk's first tempo partial sum in the call's order and their number -- only the stage taps need them on the host)
int run_chunk(etd_beat* e, const float* feat_dev, const BeatChunk& c, int max_seg, int seg_base, int segs, float* logits_dev, float* tempo_dev, hipStream_t st) {
  const etd_beat_cfg& k = e->cfg;
  const int R = c.rows, F = c.frames;
  const double fR = R;
  // ---- stage taps (etd_beat_debug_stage_taps): every copy follows the launch that produced its source, on the same stream, into slice `sl` of a buffer of `total`
  // units per slice at the chunk's global offset `base`; a NULL member is off.  With taps off none of this runs.
  const etd_debug_beat_taps& tp = e->st;
  const bool ton = e->st_on;
  auto tap = [&](float* dst, int sl, long long total, long long base, const float* src, long long n, long long width) -> int {
    if (!dst) return ETD_OK;
    HIP_TRY(hipMemcpyAsync(dst + ((long long)sl * total + base) * width, src, (size_t)(n * width) * 4, hipMemcpyDeviceToDevice, st));
    return ETD_OK;
  };
  auto rtap = [&](float* dst, int sl, const float* src, long long width) { return tap(dst, sl, tp.rows, c.row_base, src, R, width); };
  ETD_TRY(launch_beat_conv1(feat_dev + (long long)c.row_base * BEAT_MELS, c, e->c1w, e->c1b, e->c1, st));      // conv front end
  if (ton) ETD_TRY(rtap(tp.c1, 0, e->c1, BEAT_W1 * BEAT_C1));
  ETD_TRY(gemm(e->c2, e->c1, R * BEAT_W1, DEPI_BIAS, e->c2o, nullptr, st, BEAT_C1));      // row r 42 + col = the patch at (r 42 + col) 32
  if (ton) ETD_TRY(rtap(tp.c2, 0, e->c2o, BEAT_W1 * BEAT_C2));
  ETD_TRY(launch_beat_patch3(e->c2o, BEAT_W1, c, e->x3, st));
  if (ton) ETD_TRY(rtap(tp.x3, 0, e->x3, 3 * BEAT_K3));
  ETD_TRY(gemm(e->c3, e->x3, R * 3, DEPI_BIAS, e->c3o, nullptr, st));
  if (ton) ETD_TRY(rtap(tp.c3, 0, e->c3o, 3 * 256));
  ETD_TRY(launch_beat_pool3(e->c3o, R, e->x, st));
  if (e->tap_front) HIP_TRY(hipMemcpyAsync(e->tap_front + (long long)c.row_base * 256, e->x, (size_t)R * 256 * 4, hipMemcpyDeviceToDevice, st));
  if (ton) ETD_TRY(rtap(tp.front, 0, e->x, 256));
  for (int l = 0; l < k.nlayers; ++l) {
    const TimeLayer& L = e->tl[l];
    const bool tl = ton && ((tp.layer_mask >> l) & 1u);
    const int sl = __builtin_popcount(tp.layer_mask & ((1u << l) - 1u)), isl = __builtin_popcount(tp.layer_mask & 0x38u & ((1u << l) - 1u));
    ETD_TRY(launch_ln_rows_f32(e->x, R, 256, L.ln1g, L.ln1b, nullptr, nullptr, 1e-5f, e->xa, nullptr, st));
    if (tl) ETD_TRY(rtap(tp.ln1, sl, e->xa, 256));
    ETD_TRY(gemm(L.qkv, e->xa, R, DEPI_BIAS, e->qkv, nullptr, st));
    if (tl) ETD_TRY(rtap(tp.qkv, sl, e->qkv, 768));
    ETD_TRY(launch_beat_dattn(e->qkv, c, L.Er, 1 << l, e->skip, e->x, st));
    if (tl) { ETD_TRY(rtap(tp.skip, sl, e->skip, 256)); ETD_TRY(rtap(tp.x_attn, sl, e->x, 256)); }
    ETD_TRY(launch_beat_skipacc(e->skip, c, l == 0 ? 1 : 0, e->tacc, st));
    if (tl) ETD_TRY(tap(tp.tacc, sl, tp.frames, c.frame_base, e->tacc, F, 256));
    ETD_TRY(launch_ln_rows_f32(e->x, R, 256, L.ln2g, L.ln2b, nullptr, nullptr, 1e-5f, e->xa, nullptr, st));
    if (tl) ETD_TRY(rtap(tp.ln2, sl, e->xa, 256));
    ETD_TRY(gemm(L.l1, e->xa, R, DEPI_GELU, e->hid, nullptr, st));
    if (tl) ETD_TRY(rtap(tp.hid, sl, e->hid, k.d_hid));
    ETD_TRY(gemm(L.l2, e->hid, R, DEPI_RESID, nullptr, e->x, st));
    if (tl) ETD_TRY(rtap(tp.x_ffn, sl, e->x, 256));
    if (l == 0 && e->tap_l0) HIP_TRY(hipMemcpyAsync(e->tap_l0 + (long long)c.row_base * 256, e->x, (size_t)R * 256 * 4, hipMemcpyDeviceToDevice, st));
    if (l >= 3 && l <= 5) {
      const InstrLayer& I = e->il[l - 3];
      ETD_TRY(launch_ln_rows_f32(e->x, R, 256, I.ln1g, I.ln1b, nullptr, nullptr, 1e-5f, e->xa, nullptr, st));
      if (tl) ETD_TRY(rtap(tp.iln1, isl, e->xa, 256));
      ETD_TRY(gemm(I.inp, e->xa, R, DEPI_BIAS, e->qkv, nullptr, st));
      if (tl) ETD_TRY(rtap(tp.iqkv, isl, e->qkv, 768));
      ETD_TRY(launch_beat_iattn(e->qkv, c, e->skip, st));
      if (tl) ETD_TRY(rtap(tp.iao, isl, e->skip, 256));
      ETD_TRY(gemm(I.outp, e->skip, R, DEPI_RESID, nullptr, e->x, st));
      if (tl) ETD_TRY(rtap(tp.ix_attn, isl, e->x, 256));
      ETD_TRY(launch_ln_rows_f32(e->x, R, 256, I.ln2g, I.ln2b, nullptr, nullptr, 1e-5f, e->xa, nullptr, st));
      if (tl) ETD_TRY(rtap(tp.iln2, isl, e->xa, 256));
      ETD_TRY(gemm(I.l1, e->xa, R, DEPI_RELU, e->hid, nullptr, st));
      if (tl) ETD_TRY(rtap(tp.ihid, isl, e->hid, k.d_hid));
      ETD_TRY(gemm(I.l2, e->hid, R, DEPI_RESID, nullptr, e->x, st));
      if (tl) ETD_TRY(rtap(tp.ix_ffn, isl, e->x, 256));
    }
  }
  {
    ProfScope ps("k_beat_head", st, fR * 256 + (double)F * 256 * 2 * k.ntoken, fR * 256 * 4);
    hipLaunchKernelGGL(k_beat_head, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, st, e->x, c, e->ow, e->ob, k.ntoken, logits_dev);
    HIP_TRY(hipGetLastError());
  }
  if (tempo_dev) {
    ProfScope ps("k_beat_tempo", st, (double)F * 256 + (double)c.count * 256 * 2 * k.tempo_out, (double)F * 256 * 4 + (double)k.tempo_out * 256 * 4);
    hipLaunchKernelGGL(k_beat_tempo_part, dim3((unsigned)max_seg, (unsigned)c.count), dim3(256), 0, st, e->tacc, c, e->part);
    HIP_TRY(hipGetLastError());
    if (ton) ETD_TRY(tap(tp.part, 0, tp.segs, seg_base, e->part, segs, 256));
    hipLaunchKernelGGL(k_beat_tempo, dim3((unsigned)c.count), dim3(256), 0, st, e->part, c, e->tw, e->tb, k.tempo_out, tempo_dev);
    HIP_TRY(hipGetLastError());
  }
  return ETD_OK;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int etd_beat_create(const etd_beat_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n, etd_beat** out) {
  if (!cfg || !out || (n > 0 && (!names || !host_ptrs || !numels)) || n < 0) ETD_FAIL(ETD_EINVAL, "beat_create: null argument");
  *out = nullptr;
  if (cfg->struct_bytes != (int)sizeof(etd_beat_cfg))
    ETD_FAIL(ETD_EINVAL, "beat_create: etd_beat_cfg of %d bytes, this library (ABI %d) expects %d -- caller built against another etude_hip.h", cfg->struct_bytes, ETD_ABI_VERSION,
             (int)sizeof(etd_beat_cfg));
  const etd_beat_cfg& c = *cfg;
  if (c.nhead != 8) ETD_FAIL(ETD_EINVAL, "beat_create: nhead = %d; the reference's dilated head table (dilated_transformer_layer.py:45-63) is written for 8 heads", c.nhead);
  if (c.attn_len != 5) ETD_FAIL(ETD_EINVAL, "beat_create: attn_len = %d; the reference's dilated head table is written for 5 taps", c.attn_len);
  if (c.dmodel % 256 != 0 || c.dmodel != 256) ETD_FAIL(ETD_EINVAL, "beat_create: dmodel = %d; this engine takes dmodel = 256 (head_dim 32)", c.dmodel);
  if (!c.norm_first) ETD_FAIL(ETD_EINVAL, "beat_create: norm_first = 0 (post-norm layers) is not supported");
  if (c.n_mels != 128) ETD_FAIL(ETD_EINVAL, "beat_create: n_mels = %d; the conv front end pools 128 mel bins to one token", c.n_mels);
  if (c.instr < 1 || c.instr > 8) ETD_FAIL(ETD_EINVAL, "beat_create: instr = %d (1 .. 8)", c.instr);
  if (c.d_hid < 256 || c.d_hid % 256 || c.d_hid > 8192) ETD_FAIL(ETD_EINVAL, "beat_create: d_hid = %d (a multiple of 256, <= 8192)", c.d_hid);
  if (c.nlayers < 1 || c.nlayers > 16) ETD_FAIL(ETD_EINVAL, "beat_create: nlayers = %d (1 .. 16)", c.nlayers);
  if (c.ntoken < 1 || c.ntoken > 64) ETD_FAIL(ETD_EINVAL, "beat_create: ntoken = %d (1 .. 64)", c.ntoken);
  if (c.tempo_out < 1 || c.tempo_out > 65536) ETD_FAIL(ETD_EINVAL, "beat_create: tempo_out = %d", c.tempo_out);
  if (c.max_rows < 1 || c.max_rows > (1 << 24)) ETD_FAIL(ETD_EINVAL, "beat_create: max_rows = %d (1 .. 2^24)", c.max_rows);
  const WeightTable T(names, host_ptrs, numels, n);
  if (T.null_name >= 0) ETD_FAIL(ETD_EINVAL, "beat_create: null name %d", T.null_name);
  const int D = 256, H = c.d_hid;
  // every tensor the model reads, fetched with its element count before anything touches the GPU; the first failure is the one reported
  bool ok = true;
  auto get = [&](const std::string& k, int64_t numel) {
    const float* p = ok ? T.get(k, numel) : nullptr;
    if (ok && !p) { ok = false; g_etd_err = "beat_create: " + g_etd_err; }
    return p;
  };
  const float *w1 = get("conv1.weight", 32 * 15), *b1 = get("conv1.bias", 32), *w2 = get("conv2.weight", 64 * 32 * 12), *b2 = get("conv2.bias", 64);
  const float *w3 = get("conv3.weight", (int64_t)D * 64 * 18), *b3 = get("conv3.bias", D);
  const float *ow = get("out_linear.weight", (int64_t)c.ntoken * D), *ob = get("out_linear.bias", c.ntoken);
  const float *tw = get("out_linear_t.weight", (int64_t)c.tempo_out * D), *tb = get("out_linear_t.bias", c.tempo_out);
  std::vector<TimeHostW> tlw(c.nlayers);
  std::vector<InstrHostW> ilw;
  for (int l = 0; l < c.nlayers; ++l) {
    const std::string p = "Transformer_layers.time_attention_" + std::to_string(l) + ".";
    TimeHostW& t = tlw[l];
    const char* parts[3] = {"query", "key", "value"};
    for (int j = 0; j < 3; ++j) { t.Wq[j] = get(p + "self_attn." + parts[j] + ".weight", (int64_t)D * D); t.bq[j] = get(p + "self_attn." + parts[j] + ".bias", D); }
    t.Er = get(p + "self_attn.Er", 8 * 32 * 5);
    t.W1 = get(p + "linear1.weight", (int64_t)H * D); t.c1 = get(p + "linear1.bias", H);
    t.W2 = get(p + "linear2.weight", (int64_t)D * H); t.c2 = get(p + "linear2.bias", D);
    t.g1 = get(p + "norm1.weight", D); t.b1 = get(p + "norm1.bias", D); t.g2 = get(p + "norm2.weight", D); t.b2 = get(p + "norm2.bias", D);
    if (l >= 3 && l <= 5) {
      const std::string q = "Transformer_layers.instr_attention_" + std::to_string(l) + ".";
      ilw.emplace_back();
      InstrHostW& i = ilw.back();
      i.Wi = get(q + "self_attn.in_proj_weight", (int64_t)3 * D * D); i.bi = get(q + "self_attn.in_proj_bias", 3 * D);
      i.Wo = get(q + "self_attn.out_proj.weight", (int64_t)D * D); i.bo = get(q + "self_attn.out_proj.bias", D);
      i.W1 = get(q + "linear1.weight", (int64_t)H * D); i.c1 = get(q + "linear1.bias", H);
      i.W2 = get(q + "linear2.weight", (int64_t)D * H); i.c2 = get(q + "linear2.bias", D);
      i.g1 = get(q + "norm1.weight", D); i.b1 = get(q + "norm1.bias", D); i.g2 = get(q + "norm2.weight", D); i.b2 = get(q + "norm2.bias", D);
    }
  }
  if (!ok) return ETD_EINVAL;

  etd_beat* e = new etd_beat();
  e->cfg = c;
  DevPool& P = e->pool;
  auto fail = [&](int rc) { P.free_all(); delete e; return rc; };
  // conv1 as [co][kt * 3 + kw]; its output bound: |b| + 80 ||w||_1 (features |x| <= 80, the precondition)
  ETD_TRY_OR(fail, P.upload(&e->c1w, w1, 32 * 15)); ETD_TRY_OR(fail, P.upload(&e->c1b, b1, 32));
  const float bx1 = g3_bound_linear(w1, b1, 32, 15, 80.f);
  {  // conv2: [co][ci][0][kw] -> [co][kw * 32 + ci]
    std::vector<float> p((size_t)64 * BEAT_K2);
    for (int co = 0; co < 64; ++co) for (int ci = 0; ci < 32; ++ci) for (int kw = 0; kw < 12; ++kw) p[(size_t)co * BEAT_K2 + kw * 32 + ci] = w2[(co * 32 + ci) * 12 + kw];
    ETD_TRY_OR(fail, g3_lin_upload(P, p.data(), b2, 64, BEAT_K2, bx1, &e->c2));
    const float bx2 = g3_bound_linear(p.data(), b2, 64, BEAT_K2, bx1);
    // conv3: [co][ci][kt][kw] -> [co][kt * 384 + kw * 64 + ci]
    std::vector<float> p3((size_t)D * BEAT_K3);
    for (int co = 0; co < D; ++co) for (int ci = 0; ci < 64; ++ci) for (int kt = 0; kt < 3; ++kt) for (int kw = 0; kw < 6; ++kw)
      p3[(size_t)co * BEAT_K3 + kt * 384 + kw * 64 + ci] = w3[((co * 64 + ci) * 3 + kt) * 6 + kw];
    ETD_TRY_OR(fail, g3_lin_upload(P, p3.data(), b3, D, BEAT_K3, bx2, &e->c3));
  }
  e->tl.resize(c.nlayers);
  for (int l = 0; l < c.nlayers; ++l) {
    const TimeHostW& t = tlw[l];
    TimeLayer& L = e->tl[l];
    ETD_TRY_OR(fail, P.upload(&L.ln1g, t.g1, D)); ETD_TRY_OR(fail, P.upload(&L.ln1b, t.b1, D)); ETD_TRY_OR(fail, P.upload(&L.ln2g, t.g2, D)); ETD_TRY_OR(fail, P.upload(&L.ln2b, t.b2, D));
    ETD_TRY_OR(fail, P.upload(&L.Er, t.Er, 8 * 32 * 5));
    std::vector<float> wq((size_t)3 * D * D), bq(3 * D);
    for (int j = 0; j < 3; ++j) {
      memcpy(wq.data() + (size_t)j * D * D, t.Wq[j], (size_t)D * D * 4);
      memcpy(bq.data() + j * D, t.bq[j], D * 4);
    }
    ETD_TRY_OR(fail, g3_lin_upload(P, wq.data(), bq.data(), 3 * D, D, g3_bound_ln(t.g1, t.b1, D), &L.qkv));
    ETD_TRY_OR(fail, g3_lin_upload(P, t.W1, t.c1, H, D, g3_bound_ln(t.g2, t.b2, D), &L.l1));
    ETD_TRY_OR(fail, g3_lin_upload(P, t.W2, t.c2, D, H, g3_bound_linear_of_ln(t.W1, t.c1, H, D, t.g2, t.b2), &L.l2));      // |gelu(y)| <= |y|
  }
  for (const InstrHostW& i : ilw) {
    e->il.emplace_back();
    InstrLayer& I = e->il.back();
    ETD_TRY_OR(fail, P.upload(&I.ln1g, i.g1, D)); ETD_TRY_OR(fail, P.upload(&I.ln1b, i.b1, D)); ETD_TRY_OR(fail, P.upload(&I.ln2g, i.g2, D)); ETD_TRY_OR(fail, P.upload(&I.ln2b, i.b2, D));
    ETD_TRY_OR(fail, g3_lin_upload(P, i.Wi, i.bi, 3 * D, D, g3_bound_ln(i.g1, i.b1, D), &I.inp));
    std::vector<float> rb(3 * D);
    g3_row_bounds_of_ln(i.Wi, i.bi, 3 * D, D, i.g1, i.b1, rb.data());
    float bv = 0.f;
    for (int j = 2 * D; j < 3 * D; ++j) bv = fmaxf(bv, rb[j]);        // attention output: a convex combination of value rows
    ETD_TRY_OR(fail, g3_lin_upload(P, i.Wo, i.bo, D, D, bv, &I.outp));
    ETD_TRY_OR(fail, g3_lin_upload(P, i.W1, i.c1, H, D, g3_bound_ln(i.g2, i.b2, D), &I.l1));
    ETD_TRY_OR(fail, g3_lin_upload(P, i.W2, i.c2, D, H, g3_bound_linear_of_ln(i.W1, i.c1, H, D, i.g2, i.b2), &I.l2));      // |relu(y)| <= |y|
  }
  ETD_TRY_OR(fail, P.upload(&e->ow, ow, (size_t)c.ntoken * D)); ETD_TRY_OR(fail, P.upload(&e->ob, ob, c.ntoken));
  ETD_TRY_OR(fail, P.upload(&e->tw, tw, (size_t)c.tempo_out * D)); ETD_TRY_OR(fail, P.upload(&e->tb, tb, c.tempo_out));
  *out = e;
  return ETD_OK;
}

extern "C" void etd_beat_destroy(etd_beat* e) {
  if (!e) return;
  (void)hipDeviceSynchronize();
  e->pool.free_all();
  if (e->ws) (void)hipFree(e->ws);
  if (e->tab) (void)hipFree(e->tab);
  delete e;
}

extern "C" int etd_beat_forward(etd_beat* e, const float* feat_dev, int n_seq, const int64_t* T_host, float* logits_dev, float* tempo_dev, void* stream) {
  if (!e || !feat_dev || !T_host || !logits_dev || n_seq < 1) ETD_FAIL(ETD_EINVAL, "beat_forward: null argument or n_seq < 1");
  hipStream_t st = (hipStream_t)stream;
  const int ni = e->cfg.instr;
  std::vector<int> tab(3 * (size_t)(n_seq + 1));        // row0 [n_seq + 1] | frame0 [n_seq + 1] | seg0 [n_seq + 1]
  long long rows = 0, frames = 0, segs = 0, big = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (T_host[s] < 1) ETD_FAIL(ETD_EINVAL, "beat_forward: song %d has T = %lld (need >= 1)", s, (long long)T_host[s]);
    tab[s] = (int)rows; tab[n_seq + 1 + s] = (int)frames; tab[2 * (n_seq + 1) + s] = (int)segs;
    rows += T_host[s] * ni; frames += T_host[s]; segs += (T_host[s] + BEAT_SEG - 1) / BEAT_SEG;
    big = T_host[s] * ni > big ? T_host[s] * ni : big;
    if (rows > (1LL << 30)) ETD_FAIL(ETD_EINVAL, "beat_forward: more than 2^30 rows in one call");
  }
  tab[n_seq] = (int)rows; tab[2 * n_seq + 1] = (int)frames; tab[3 * n_seq + 2] = (int)segs;
  if (e->st_on && (rows > e->st.rows || frames > e->st.frames || segs > e->st.segs))       // checked before anything is launched
    ETD_FAIL(ETD_EINVAL, "beat_forward: stage taps registered for %d rows, %d frames, %d segments; this call has %lld, %lld, %lld", e->st.rows, e->st.frames, e->st.segs, rows,
             frames, segs);
  const long long cap = big > e->cfg.max_rows ? big : e->cfg.max_rows;        // a song longer than max_rows gets a workspace of its own size
  ETD_TRY(ensure_ws(e, cap, n_seq, st));
  ETD_TRY(upload_table(st, e->tab, tab));
  const int* row0 = e->tab; const int* frame0 = e->tab + n_seq + 1; const int* seg0 = e->tab + 2 * (n_seq + 1);
  int s = 0;
  while (s < n_seq) {      // chunks of whole songs, in order, up to cap rows each
    int s1 = s;
    long long r = 0, maxT = 0;
    while (s1 < n_seq && (s1 == s || r + T_host[s1] * ni <= cap)) { r += T_host[s1] * ni; maxT = T_host[s1] > maxT ? T_host[s1] : maxT; ++s1; }
    BeatChunk c;
    c.row0 = row0; c.frame0 = frame0; c.seg0 = seg0; c.first = s; c.count = s1 - s; c.row_base = tab[s]; c.frame_base = tab[n_seq + 1 + s];
    c.rows = (int)r; c.frames = (int)(r / ni); c.instr = ni;
    const int max_seg = (int)((maxT + BEAT_SEG - 1) / BEAT_SEG);
    const int seg_base = tab[2 * (n_seq + 1) + s];
    ETD_TRY(run_chunk(e, feat_dev, c, max_seg, seg_base, tab[2 * (n_seq + 1) + s1] - seg_base, logits_dev, tempo_dev, st));
    s = s1;
  }
  return ETD_OK;
}

extern "C" double etd_beat_flops(etd_beat* e, long long T) {
  if (!e || T < 1) return 0.0;
  const etd_beat_cfg& c = e->cfg;
  const double R = (double)T * c.instr, D = 256, H = c.d_hid;
  const double conv = R * (32.0 * 126 * 15 + 64.0 * 31 * 384 + D * 5 * 1152) * 2;
  const double time_l = R * (2 * D * 3 * D + 2 * 2 * D * H + 8.0 * 5 * 32 * 2 * 3);
  const int n_instr = c.nlayers > 6 ? 3 : c.nlayers > 3 ? c.nlayers - 3 : 0;
  const double instr_l = R * (2 * D * 3 * D + 2 * D * D + 2 * 2 * D * H + 8.0 * c.instr * 32 * 2 * 2);
  const double heads = (double)T * 2 * D * c.ntoken + 2 * D * c.tempo_out;
  return conv + c.nlayers * time_l + n_instr * instr_l + heads;
}

extern "C" int etd_beat_debug_taps(etd_beat* e, float* front_dev, float* layer0_dev) {
  if (!e) ETD_FAIL(ETD_EINVAL, "beat_debug_taps: null handle");
  e->tap_front = front_dev; e->tap_l0 = layer0_dev;
  return ETD_OK;
}

extern "C" int etd_beat_debug_stage_taps(etd_beat* e, const etd_debug_beat_taps* t) {
  if (!e) ETD_FAIL(ETD_EINVAL, "beat_debug_stage_taps: null handle");
  if (t && t->struct_bytes != (int)sizeof(etd_debug_beat_taps))      // first: no other member of a struct of another size is read
    ETD_FAIL(ETD_EINVAL, "beat_debug_stage_taps: etd_debug_beat_taps of %d bytes, this library expects %d", t->struct_bytes, (int)sizeof(etd_debug_beat_taps));
  if (t && t->layer_mask == 0 && !t->c1 && !t->c2 && !t->x3 && !t->c3 && !t->front && !t->part) t = nullptr;      // nothing to tap: off
  if (t) {
    const int L = e->cfg.nlayers;
    if (t->layer_mask >> L) ETD_FAIL(ETD_EINVAL, "beat_debug_stage_taps: layer_mask %#x names a layer beyond the model's %d", t->layer_mask, L);
    if (t->rows < 1 || t->frames < 1 || t->segs < 1 || t->d_hid != e->cfg.d_hid)
      ETD_FAIL(ETD_EINVAL, "beat_debug_stage_taps: buffers stated for rows %d, frames %d, segs %d, d_hid %d; the model has d_hid %d", t->rows, t->frames, t->segs, t->d_hid, e->cfg.d_hid);
    const int need = __builtin_popcount(t->layer_mask), ineed = __builtin_popcount(t->layer_mask & 0x38u);
    if (t->slices < need || t->islices < ineed)
      ETD_FAIL(ETD_EINVAL, "beat_debug_stage_taps: layer_mask %#x needs %d time and %d instrument slices, the buffers are stated to hold %d and %d", t->layer_mask, need, ineed,
               t->slices, t->islices);
  }
  e->st = t ? *t : etd_debug_beat_taps{};
  e->st_on = t != nullptr;
  return ETD_OK;
}
