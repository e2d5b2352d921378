// Source separator (csrc/separator.hip): the layout constants and the one-launch descriptor the kernels and the host side share.
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
enum { SEP_EPI_CONV = 0, SEP_EPI_DECONV = 1, SEP_EPI_HEAD = 2 };
struct SepLaunch {
  const float* x0; long long x0_us; int x0_u0, x0_div, C0;      // unit u reads x0 + ((x0_u0 + u) / x0_div) * x0_us
  const float* x1; long long x1_us; int C1;                     // ... and x1 + u * x1_us (C1 = 0: no second input)
  int Hin, Win, Hj, Wj, S, o0t, o0f, d, nt, nf;
  const float* W; long long w_is;                               // + instrument * w_is
  const float* bias; const float* bn_a; const float* bn_s;      // [instr][N]
  int N;
  float* pre; float* act; long long out_us;                     // unit u writes at + u * out_us; either may be null
  int Wout, oS, opt, opf, epi;
  int u0, I;                                                    // instrument of unit u = (u0 + u) % I
};
