// Source separator (csrc/separator.hip) and its training (csrc/separator_train.hip): the layout constants, the one-launch descriptor of the gather convolution, the
// launch both engines call, the MFMA tile step their GEMM kernels share, and the U-Net's geometry.
#pragma once
#include "host_util.h"
#include "lds_rfft.h"
#include "../../include/etude_hip.h"

#define SEP_THREADS 256
// dynamic LDS of the two FFT kernels in floats, M complex points: the two buffer pairs of the plan of lds_rfft.h
#define SEP_FFT_LDS_FLOATS(M) (4 * RFFT_PM(M))
// the implicit-GEMM tile: 64 output positions x 64 output channels, 32 of K per step (k_tgemm's shape and LDS images)
#define SEP_BM 64
#define SEP_BN 64
#define SEP_BK 32
#define SEP_LD 65
// a layer whose K = taps * Cin is below this (the first convolution with up to 2 channels), or whose Cout is 1, runs on the VALU (k_sep_conv_valu); so does the head
#define SEP_MFMA_MIN_K 64

// One launch of a gather convolution over n units: position (jt, jf) of the Hj x Wj grid of a unit reads input rows S jt + o0t + d a, a < nt (columns alike) of
// the channels [x0 | x1], multiplies by W [nt nf (C0 + C1)][N] and writes output position (oS jt + opt, oS jf + opf) of a Hout x Wout image.
//   encoder conv       S = 2, o0 = -1, d = +1, 5 x 5 taps, oS = 1
//   transposed conv    one launch per output parity (pt, pf): S = 1, o0 = p, d = -1, 2 (p = 0: kernel taps 1, 3) or 3 (p = 1: taps 0, 2, 4) taps, oS = 2, op = p
//   head               S = 1, o0 = -3, d = +2, 4 x 4 taps, oS = 1
// The epilogue of an output element v = the sum + bias:
//   CONV    pre = v, act = ELU(bn_a v + bn_s) (either may be null)          DECONV  act = bn_a ELU(v) + bn_s          HEAD  pre = v
//   PLAIN   (training: every forward convolution and every input gradient) v, with no bias when `bias` is null; columns < N0 go to `pre` [..][N0], the rest to
//           `out1` [..][N - N0]
enum { SEP_EPI_CONV = 0, SEP_EPI_DECONV = 1, SEP_EPI_HEAD = 2, SEP_EPI_PLAIN = 3 };
struct SepLaunch {                                              // (the leading fields arrive in SGPRs, build.py's kernarg preload: new fields go to the end)
  const float* x0; long long x0_us; int x0_u0, x0_div, C0;      // unit u reads x0 + ((x0_u0 + u) / x0_div) * x0_us
  const float* x1; long long x1_us; int C1;                     // ... and x1 + u * x1_us (C1 = 0: no second input)
  int Hin, Win, Hj, Wj, S, o0t, o0f, d, nt, nf;
  const float* W; long long w_is;                               // + instrument * w_is
  const float* bias; const float* bn_a; const float* bn_s;      // [instr][N]
  int N;
  float* pre; float* act; long long out_us;                     // unit u writes at + u * out_us; either may be null
  int Wout, oS, opt, opf, epi;
  int u0, I;                                                    // instrument of unit u = (u0 + u) % I
  int N0; float* out1; long long out1_us;                       // PLAIN only: the column split and the second output tensor
};

// The launch of both engines (separator.hip; the kernels are compiled there, once: one body each, the epilogue a template parameter the launch picks by `epi`): the
// VALU kernel for K < SEP_MFMA_MIN_K, N = 1, the head and `force_valu`, the MFMA kernel otherwise.  `name`: the profile scope, or null for none.
int sep_launch(const SepLaunch& a, int n_units, bool force_valu, const char* name, hipStream_t st);

// kernel taps of a transposed convolution that reach output parity p, in the order the packed weights hold them (a = 0, 1, (2)): p = 0: 1, 3; p = 1: 0, 2, 4
__host__ __device__ inline int sep_dec_taps(int p) { return p ? 3 : 2; }
__host__ __device__ inline int sep_dec_tap(int p, int a) { return p ? 2 * a : 1 + 2 * a; }

// ---- the U-Net's shapes: what both engines derive from the config
struct SepNet {
  int T, F, C, I;
  int Cenc[ETD_SEP_LEVELS + 1];             // Cenc[0] = n_channels, Cenc[l] = filters[l - 1]
  int Cdout[ETD_SEP_LEVELS + 1];            // decoder j's output channels: filters[5 - j], 1 for j = 6
  long long szE[ETD_SEP_LEVELS + 1];        // floats of one unit's conv_l output [T >> l][F >> l][Cenc l]
  long long szD[ETD_SEP_LEVELS + 1];        // ... of decoder j's output [T >> (6 - j)][F >> (6 - j)][Cdout j]
  long long posE(int l) const { return (long long)(T >> l) * (F >> l); }
  long long posD(int j) const { return (long long)(T >> (ETD_SEP_LEVELS - j)) * (F >> (ETD_SEP_LEVELS - j)); }
};
inline void sep_net_init(SepNet* n, const etd_sep_cfg& c) {
  n->T = c.T; n->F = c.F; n->C = c.n_channels; n->I = c.n_instr;
  n->Cenc[0] = c.n_channels; n->Cdout[0] = 0; n->szE[0] = n->szD[0] = 0;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) n->Cenc[l] = c.filters[l - 1];
  for (int j = 1; j < ETD_SEP_LEVELS; ++j) n->Cdout[j] = c.filters[ETD_SEP_LEVELS - 1 - j];
  n->Cdout[ETD_SEP_LEVELS] = 1;
  for (int l = 1; l <= ETD_SEP_LEVELS; ++l) { n->szE[l] = n->posE(l) * n->Cenc[l]; n->szD[l] = n->posD(l) * n->Cdout[l]; }
}

// ---- the geometry of the three layer kinds: sizes, stride, first offset, dilation, taps, output stride and parity, channel counts.  Pointers, unit strides, weights
// and the epilogue are the caller's.  The trainer's gradients run on the same geometries with their own channel counts: a convolution's input gradient is the
// transposed convolution's, a transposed convolution's input and weight gradients are the convolution's at the doubled size, the head's input gradient is the head's
// with offset and dilation negated.
inline void sep_geom_encoder(const SepNet& n, int l, SepLaunch* a) {      // l = 1 .. 6
  a->C0 = n.Cenc[l - 1]; a->C1 = 0; a->N = n.Cenc[l];
  a->Hin = n.T >> (l - 1); a->Win = n.F >> (l - 1); a->Hj = n.T >> l; a->Wj = n.F >> l;
  a->S = 2; a->o0t = -1; a->o0f = -1; a->d = 1; a->nt = 5; a->nf = 5;
  a->Wout = a->Wj; a->oS = 1; a->opt = 0; a->opf = 0;
}
inline void sep_geom_deconv(const SepNet& n, int j, int pt, int pf, SepLaunch* a) {      // j = 1 .. 6 on [skip | up], output parity (pt, pf)
  a->C0 = n.Cenc[7 - j]; a->C1 = j > 1 ? n.Cdout[j - 1] : 0; a->N = n.Cdout[j];
  a->Hin = n.T >> (7 - j); a->Win = n.F >> (7 - j); a->Hj = a->Hin; a->Wj = a->Win;
  a->S = 1; a->o0t = pt; a->o0f = pf; a->d = -1; a->nt = sep_dec_taps(pt); a->nf = sep_dec_taps(pf);
  a->Wout = 2 * a->Win; a->oS = 2; a->opt = pt; a->opf = pf;
}
inline void sep_geom_head(const SepNet& n, SepLaunch* a) {
  a->C0 = 1; a->C1 = 0; a->N = n.C;
  a->Hin = n.T; a->Win = n.F; a->Hj = a->Hin; a->Wj = a->Win;
  a->S = 1; a->o0t = -3; a->o0f = -3; a->d = 2; a->nt = 4; a->nf = 4;
  a->Wout = a->Win; a->oS = 1; a->opt = 0; a->opf = 0;
}

// ---- the MFMA tile step of the 64 x 64 x 32 GEMM kernels (k_sep_conv_mfma, k_st_dw).  As [k][m] and Bs [k][n] hold one step of 32 of K; a wave owns the 32 x 32
// block at rows m = arow - l31 .., columns n = bcol - l31 .. (arow = wr * 32 + l31, bcol = wc * 32 + l31, half = lane >> 5).
// The summation order of an output element, which is part of both engines' contract (the same call gives the same bits; a weight gradient's slice sums as the
// forward does): every step runs as two chains of 8 v_mfma_f32_32x32x2_f32 (16 terms each) that are added and join one of four running totals (step s -> total
// s % 4); the totals are added pairwise at the end.  No chain is longer than K / 128 + 16 terms, in an order the shape fixes.
__device__ __forceinline__ void sep_tile_zero(f32x16 (&tot)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[c][r] = 0.f;
}
__device__ __forceinline__ void sep_tile_step(const float (&As)[SEP_BK][SEP_LD], const float (&Bs)[SEP_BK][SEP_LD], int arow, int bcol, int half, int step,
                                              f32x16 (&tot)[4]) {
  f32x16 p0, p1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { p0[r] = 0.f; p1[r] = 0.f; }
#pragma unroll
  for (int kk = 0; kk < SEP_BK; kk += 4) {
    p0 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + half][arow], Bs[kk + half][bcol], p0, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + 2 + half][arow], Bs[kk + 2 + half][bcol], p1, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) p0[r] += p1[r];
  switch (step & 3) {                                // (uniform)
    case 0: for (int r = 0; r < 16; ++r) tot[0][r] += p0[r]; break;
    case 1: for (int r = 0; r < 16; ++r) tot[1][r] += p0[r]; break;
    case 2: for (int r = 0; r < 16; ++r) tot[2][r] += p0[r]; break;
    default: for (int r = 0; r < 16; ++r) tot[3][r] += p0[r]; break;
  }
}
__device__ __forceinline__ float sep_tile_total(const f32x16 (&tot)[4], int r) { return (tot[0][r] + tot[1][r]) + (tot[2][r] + tot[3][r]); }

// ---- multichannel Wiener filtering of one song's masked spectra (separator_mwf.hip): `iterations` (1 .. SEP_MWF_MAX_ITER) passes in place on
// Y [I][C][Tf][F] with the mixture X [C][Tf][F], C = 1 or 2, in `scratch` (sep_mwf_scratch_bytes of it, 256-byte aligned, the caller's: etd_sep_run lends the work
// region, idle between the mask pass and the inverse STFT).  Reads nothing but the song's own X and Y, sums in an order Tf alone fixes.
#define SEP_MWF_MAX_ITER 8
#define SEP_MWF_MAX_CHANNELS 2
#define SEP_MWF_CHUNK 64                   // frames per partial sum of the source model
long long sep_mwf_scratch_bytes(int I, int C, int F, long long Tf);
int sep_mwf_run(const float2* X, float2* Y, long long Tf, int I, int C, int F, int iterations, void* scratch, hipStream_t st);
