// Note renderer (csrc/render.hip): the constants and records the kernels and the host side share.  DESIGN.md 4l is the contract.
#pragma once
#include "host_util.h"
#include "alignfeat.h"
#include "../../include/etude_hip.h"

#define RN_THREADS 256
#define RN_PER_THREAD 4                          // consecutive samples of a thread: one 16-byte store
#define RN_BLOCK (RN_THREADS * RN_PER_THREAD)    // samples a workgroup owns
#define RN_MAX_PARTIALS 16
#define RN_MAX_NOTES (1 << 16)                   // notes per cover
#define RN_MAX_SAMPLES AF_MAX_N                  // samples per cover: what etd_alignfeat takes
#define RN_MAX_COVERS 4096                       // covers per call
#define RN_MAX_LAUNCH_BLOCKS (1 << 23)           // workgroups per launch (2^31 threads); a call above it takes several launches
#define RN_ALIGN 64                              // a cover's first sample in the flat buffer: a multiple of this many floats

struct RnCover {          // one per cover of a call (host -> device)
  long long blk0;         // its first workgroup among the call's
  long long out_off;      // its first sample in the flat buffer
  long long N;            // its samples
  int note0, n_notes;     // its notes among the call's
};

struct RnHead {           // one per note (host -> device): the note, its cover's tuning, and the samples it sounds on -- decided once, on the host, by the
  double onset, offset;   // restatement's own fp64 predicates: n_first = the first n with n / sr >= onset, n_end = the first n with n / sr - offset >= R
  double cents;
  long long n_first, n_end;
  int pitch, velocity;
};

struct RnNote {           // one per note (prep kernel -> render kernel), everything derived in fp64
  long long n_first, n_end;
  double d0;              // n_first / sr - onset: the time since the onset at the first sample, 0 <= d0 < 1 / sr
  double dur;             // offset - onset
  int K, pad;             // surviving partials
  double fsr[RN_MAX_PARTIALS];     // f_k / sr: revolutions per sample
  double ph0[RN_MAX_PARTIALS];     // f_k * d0: revolutions at the first sample
  float amp[RN_MAX_PARTIALS];      // A_k
  float dec[RN_MAX_PARTIALS];      // -log2(e) / T_k (0: no decay)
};

struct RnVoice {          // the kernel's view of etd_render_cfg
  double sr, inv_sr;
  double inharmonicity, inharmonicity_step, partial_rolloff, velocity_power, decay_base, decay_halving, decay_partial, nyquist_hz;
  float inv_attack, rel_c, inv_rel_len, gain;      // 1 / attack, -log2(e) / release_tau, 1 / release_len
  int partials, decay_on, release_on;
};
