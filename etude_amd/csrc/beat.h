// Beat-Transformer engine (Demixed_DilatedTransformerModel, etude/models/beat_transformer.py:23-106): the exact-parity (fp32-grade) forward pass of beat / downbeat
// logits and the tempo head.  Dense contractions on csrc/gemm3.h; the conv front end's pooling, the dilated 5-tap attention, the 5-token instrument attention, the
// skip accumulation and the two heads are the kernels of beat.hip.  The C entry points are etd_beat_* (include/etude_hip.h).
//
// The trainer (beat_train.hip) runs the same model: the song table, the device helpers and the launchers below are what the two share, so that a stage exists once.
#pragma once
#include "gemm3.h"

#define BEAT_HEADS 8
#define BEAT_HEAD_DIM 32
#define BEAT_DMODEL 256
#define BEAT_TAPS 5
#define BEAT_MELS 128
#define BEAT_C1 32            // conv1 channels; pooled width 42 (126 / 3)
#define BEAT_W1 42
#define BEAT_C2 64            // conv2 channels; the conv2 GEMM runs over all 42 pooled conv1 columns (overlapping rows of the [row][42][32] buffer), 0 .. 23 are used
#define BEAT_C2_COLS 24       // conv2 columns the model reads (8 pooled columns x 3); the trainer forms only these
#define BEAT_K2 384           // 12 x 32
#define BEAT_K3 1152          // 3 x 6 x 64
#define BEAT_SEG 128          // frames per partial sum of the tempo head's time mean
#define BEAT_SCALE 5.656854249492380195f      // sqrt(head_dim)

// ================================================================================================ song tables
// The chunk's songs: global row / frame offsets of every song of the call (one table, uploaded once per call) and the chunk's slice of it.
struct BeatChunk {
  const int* row0;      // [n_seq + 1] global row offset of song s (row0[n_seq] = total rows)
  const int* frame0;    // [n_seq + 1] global frame offset
  const int* seg0;      // [n_seq + 1] global offset of song s's first tempo partial sum (ceil(T / 128) per song); only the engine's tempo head reads it
  int first, count;     // songs [first, first + count) form this chunk
  int row_base, frame_base;     // row0[first], frame0[first]: chunk-local row r = global row - row_base
  int rows, frames;
  int instr;
};
// a whole call as one chunk (the trainer: its rows must fit the workspace sized at create)
inline BeatChunk beat_whole_call(const int* row0, const int* frame0, int n_seq, int rows, int frames, int instr) {
  return BeatChunk{row0, frame0, nullptr, 0, n_seq, 0, 0, rows, frames, instr};
}

// ================================================================================================ the stages the engine and the trainer both run
// Each is one kernel of beat.hip (feat, c2, qkv, ... point at the chunk's first row).  patch3 reads c2 as [row][c2_cols][64], c2_cols = BEAT_W1 or BEAT_C2_COLS.  dattn
// updates x in place; dattn_train also keeps the probabilities prob [rows][8][5] and writes xout = xin + skip out of place.
int launch_beat_conv1(const float* feat, const BeatChunk& c, const float* w, const float* b, float* c1, hipStream_t st);
int launch_beat_patch3(const float* c2, int c2_cols, const BeatChunk& c, float* x3, hipStream_t st);
int launch_beat_pool3(const float* c3, int rows, float* x, hipStream_t st);
int launch_beat_dattn(const float* qkv, const BeatChunk& c, const float* Er, int dil, float* skip, float* x, hipStream_t st);
int launch_beat_dattn_train(const float* qkv, const BeatChunk& c, const float* Er, int dil, const float* xin, float* prob, float* skip, float* xout, hipStream_t st);
int launch_beat_skipacc(const float* skip, const BeatChunk& c, int first_layer, float* tacc, hipStream_t st);
int launch_beat_iattn(const float* qkv, const BeatChunk& c, float* ao, hipStream_t st);

// ================================================================================================ device helpers
// The source-level order of the floating-point operations is the contract: a forward kernel and the backward kernel that recomputes its maximum or its softmax call
// the same function.
#ifdef __HIPCC__
__device__ __forceinline__ int beat_song_of(const int* off, int first, int count, int g) {       // largest s in the chunk with off[s] <= g
  int lo = first, hi = first + count - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= g) lo = mid; else hi = mid - 1; }
  return lo;
}
// chunk-local row r -> its song s, the song's frame count T and the row's frame t
__device__ __forceinline__ void beat_row_at(const BeatChunk& c, int r, int& s, int& T, int& t) {
  const int g = r + c.row_base;
  s = beat_song_of(c.row0, c.first, c.count, g);
  T = c.frame0[s + 1] - c.frame0[s]; t = (g - c.row0[s]) % T;
}
// chunk-local frame fl -> its song s, T and the chunk-local row rb of its instrument 0 (instrument i is row rb + i T)
__device__ __forceinline__ void beat_frame_at(const BeatChunk& c, int fl, int& s, int& T, int& rb) {
  const int gf = fl + c.frame_base;
  s = beat_song_of(c.frame0, c.first, c.count, gf);
  T = c.frame0[s + 1] - c.frame0[s];
  const int t = gf - c.frame0[s];
  rb = c.row0[s] - c.row_base + t;
}
// tap j of head h of the dilated attention reads the row at time t + beat_tap_off(h, j) 2^layer
__device__ __forceinline__ int beat_tap_off(int h, int j) { return h < 4 ? j - 2 : h == 4 ? j - 4 : h == 5 ? j - 3 : h == 6 ? j - 1 : j; }

__device__ __forceinline__ void beat_load32(float (&a)[32], const float* p) {
#pragma unroll
  for (int d = 0; d < 32; d += 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(p + d); a[d] = v[0]; a[d + 1] = v[1]; a[d + 2] = v[2]; a[d + 3] = v[3]; }
}
__device__ __forceinline__ void beat_store32(float* p, const float (&a)[32]) {
#pragma unroll
  for (int d = 0; d < 32; d += 4) { const f32x4 v = {a[d], a[d + 1], a[d + 2], a[d + 3]}; *reinterpret_cast<f32x4*>(p + d) = v; }
}
__device__ __forceinline__ float beat_dot32(const float (&a)[32], const float* p) {      // one fmaf chain, d ascending
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 32; d += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + d);
    s = fmaf(a[d], v[0], s); s = fmaf(a[d + 1], v[1], s); s = fmaf(a[d + 2], v[2], s); s = fmaf(a[d + 3], v[3], s);
  }
  return s;
}
__device__ __forceinline__ void beat_axpy32(float (&acc)[32], float s, const float* p) {
#pragma unroll
  for (int d = 0; d < 32; d += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + d);
    acc[d] = fmaf(s, v[0], acc[d]); acc[d + 1] = fmaf(s, v[1], acc[d + 1]); acc[d + 2] = fmaf(s, v[2], acc[d + 2]); acc[d + 3] = fmaf(s, v[3], acc[d + 3]);
  }
}
// one conv1 output before pooling, column 3 p + u: b + sum_{kt<5,kw<3} w[kt][kw] x[t + kt - 2][3 p + u + kw], x = 0 outside the song (padding (2, 0)); one serial fmaf chain
__device__ __forceinline__ float beat_conv1_at(const float* feat, int r, int t, int T, int p, int u, const float (&wr)[15], float b) {
  float acc = b;
#pragma unroll
  for (int kt = 0; kt < 5; ++kt) {
    const int tt = t + kt - 2;
    if (tt < 0 || tt >= T) continue;
    const float* xr = feat + (long long)(r + kt - 2) * BEAT_MELS + 3 * p + u;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) acc = fmaf(wr[kt * 3 + kw], xr[kw], acc);
  }
  return acc;
}
// max-pool over 3 + ReLU
__device__ __forceinline__ float beat_pool3_relu(float v0, float v1, float v2) { return fmaxf(fmaxf(fmaxf(v0, v1), v2), 0.f); }
#endif
