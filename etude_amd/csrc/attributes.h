// Bar attributes (csrc/attributes.hip): the constants the kernel and the host side share.  DESIGN.md 4i is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"

#define AT_WAVES 4                  // pairs per workgroup: one wavefront each
#define AT_THREADS (64 * AT_WAVES)
#define AT_MAX_TOKENS 4096          // tokens per bar: a position's target and overlap counts share one 32-bit word, 16 bits each
#define AT_MAX_PAIRS (1 << 20)      // pairs (and bars per side) per call
#define AT_MAX_POS_RANGE 4096       // distinct Pos values a vocabulary may span: 8 bytes of LDS per value and wavefront, 128 KB per workgroup at the limit
#define AT_MAX_EDGES 2              // bin edges per attribute (three bins)

// status word of a pair (etude_hip.h)
#define AT_BAD_ID 1
#define AT_BAD_INDEX 2
#define AT_NPOS_SHIFT 8

struct AtArgs {
  const int32_t* src_ids; const int64_t* src_off; const int32_t* src_idx; int n_src;
  const int32_t* tgt_ids; const int64_t* tgt_off; const int32_t* tgt_idx; int n_tgt;
  const int2* table; int V, pos_min, npos, n_pairs;
  int ty_pos, ty_note, ty_dur;
  int32_t* feat; double* attr; int32_t* bins; int32_t* status;
  int n_edges[4]; double edges[4][AT_MAX_EDGES];
};
