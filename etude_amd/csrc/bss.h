// BSS Eval on the device (csrc/bss.hip): the constants of the source and the kernels' argument blocks.  DESIGN.md 4p is the contract.
#pragma once
#include "common.h"

#define BSS_SLICE 32768          // samples of one correlation slice: a constant of the source, whatever the device or N (the partials are joined in slice order)
#define BSS_CHUNK 512            // samples a workgroup holds in LDS at a time
#define BSS_LAGS_PER_WG 256      // four waves x 64 lags
#define BSS_ROWS_PER_WG 256      // projection: four waves x 64 output samples
#define BSS_MAX_SOURCES 8
#define BSS_MAX_CHANNELS 2
#define BSS_MAX_SIGNALS 16       // = the matrix core's tile width: the lag-0 signals are one column tile, the right-hand sides one block
#define BSS_MAX_ORDER 8192       // S L
#define BSS_MAX_L 512
#define BSS_NB 16                // Cholesky panel width = the tile

struct BssTrack {
  const float* ref;              // [J][C][N]
  const float* est;
  int J, C, S, L;
  long long N;
  int window, hop, nwin;
};
