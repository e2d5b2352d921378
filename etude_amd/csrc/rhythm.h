// Rhythm metrics (csrc/rhythm.hip): the constants the kernel and the host side share.  DESIGN.md 4h is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"
#include "../../include/etude_hip_debug.h"

#define RH_THREADS 256
#define RH_MAX_ONSETS 8192          // onsets per cover: 8 191 IOIs; the cover's working set is 17 bytes per slot of LDS, 136 KB at the limit
#define RH_IDX_BITS 13              // an IOI's index inside its cover
#define RH_MAX_COVERS (1 << 20)     // covers per call
#define RH_MAX_TOPK 64
#define RH_MAX_DIGITS 9             // rint(ioi * 10^digits) must stay below 2^50 (a 64-bit sort key holds it above the 13 index bits)
#define RH_MAX_NGRAM 16             // 3-bit symbols: 48 bits of a 64-bit key
#define RH_MAX_CLUSTERS 8
#define RH_N_RANDOM 29              // 1 + 7 x (2 + int(log 8)) doubles of RandomState(42).random_sample
#define RH_MAX_ITER 300
#define RH_LDS_PER_SLOT 17          // fp64 + 64-bit key + label

// status word of a cover (etude_hip.h)
#define RH_BAD_INPUT 5

struct RhArgs {
  const double* onsets; const int64_t* offsets; int n_covers;
  double* out; int32_t* status;
  int top_k, n_gram, n_clusters, slots;          // slots: LDS slots of this launch, a power of two >= the longest cover's IOIs
  double scale, min_ioi, max_ioi;
  double rnd[RH_N_RANDOM];
  double* tap_x; signed char* tap_lab; double* tap_c;
};
