// DBN beat / downbeat tracking (madmom 0.16's DBNBeatTrackingProcessor / DBNDownBeatTrackingProcessor restated): the host tables of one HMM.
// dbn_host.cpp builds them (plain C++, no GPU: etd_dbn_describe / etd_dbn_workspace_bytes), dbn.hip uploads them and runs the Viterbi kernels.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/etude_hip.h"

constexpr int DBN_MAX_STATES = 8192;      // largest HMM a handle accepts (Viterbi vector in LDS: 64 KiB of fp64)
constexpr int DBN_MAX_INTERVALS = 255;    // backpointers are one byte: the predecessor's interval index

struct DbnHmm {
  int num_beats = 1;                      // 1 = the beat HMM, B = a bar of B beats
  int n_int = 0;                          // intervals (tempi) per beat
  int per_beat = 0;                       // states per beat = sum(intervals)
  int S = 0;                              // states = num_beats * per_beat
  int K = 2;                              // densities per frame: 2 (beat HMM) or 3 (bar HMM)
  double init = 0.0;                      // log(1 / S)
  std::vector<int32_t> ivl;               // [n_int] interval lengths in frames, ascending
  std::vector<int32_t> first;             // [n_int] first state of interval j inside one beat
  std::vector<double> lt;                 // [to][from] log transition last state of `from` -> first state of `to`; -inf = no edge
  std::vector<int32_t> flo, fhi;          // [to] lowest / highest `from` with an edge
  std::vector<uint8_t> ptr;               // [S] density index of a state
  std::vector<uint8_t> beatno;            // [S] int(position) + 1
  std::vector<uint16_t> chain;            // [S] beat * n_int + interval index
};

// validate cfg (ETD_EINVAL + message otherwise) and build the beat HMM followed by one bar HMM per beats_per_bar entry; device_limits: also refuse what the
// device engine cannot hold (DBN_MAX_STATES, DBN_MAX_INTERVALS)
int dbn_build(const etd_dbn_cfg* cfg, std::vector<DbnHmm>& out, bool device_limits);

// device workspace of one (song of T frames, HMM): what the Viterbi kernel writes besides its LDS
struct DbnWs {
  long long bp, seg, rr, bn, out, dens, total;   // byte offsets inside the block, and its size
  long long out_cap;                              // (frame, number) pairs the result list can hold
};
DbnWs dbn_ws_layout(const DbnHmm& h, long long T);
