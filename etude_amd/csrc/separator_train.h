// Separator training (csrc/separator_train.hip): the launch descriptors its kernels and its host side share.  DESIGN.md 4n is the contract.
#pragma once
#include "separator.h"

// dW: the K axis (unit, position) of one instrument is cut into slices of this many rows, whatever the device and the batch
#define ST_DW_SLICE 4096
// column reductions: a workgroup sums this many rows of its columns
#define ST_COL_ROWS 1024
// running statistics: r <- m r + (1 - m) batch
#define ST_BN_MOMENTUM 0.99

// (The convolutions -- every forward one and every input gradient -- are launches of separator.h's SepLaunch with the PLAIN epilogue; unit u = b * I + instrument.)

// One weight gradient: part[inst][slice][m][n] = sum over the slice's rows k = b * P + pos of g(pos, tap(m), cg(m)) y[pos][n]; m = tap * Cg + cg, y = [y0 | y1]
struct StDw {
  const float* g; long long g_us; int g_div, Cg, Hg, Wg;
  int S, o0t, o0f, d, nt, nf;
  const float* y0; long long y0_us; int N0; const float* y1; long long y1_us; int N1;
  int Hj, Wj, B, I, slices;
  float* part;
};

// column reductions over the rows (b, pos) of one instrument; what is summed:
enum { ST_COL_X = 0, ST_COL_ELU = 1, ST_COL_VAR = 2, ST_COL_VAR_ELU = 3, ST_COL_BWD_ENC = 4, ST_COL_BWD_DEC = 5 };
struct StCol {
  const float* x; const float* x2; long long us; int P, C, B, I, mode, chunks, CT;
  const double* mean; const double* rstd; const float* gamma; const float* beta;    // [I][C]; the statistics are kept in fp64
  float* part;                                                                     // [2][I][chunks][C]
};
enum { ST_FIN_MEAN = 0, ST_FIN_VAR = 1, ST_FIN_BWD = 2, ST_FIN_BIAS = 3 };

// elementwise passes
enum { ST_EW_ENC = 0, ST_EW_DEC = 1, ST_EW_ENC_BWD = 2, ST_EW_DEC_BWD = 3 };
struct StEw {
  const float* x; const float* dy; const float* add; float* out;
  long long total, unit; int C, I, mode;
  const double* mean; const double* rstd; const float* gamma; const float* beta; const double* m1; const double* m2;
};
