// Audio loading (csrc/resample.hip): the constants and per-call tables the kernel and the host side share.  DESIGN.md 4q is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"
#include "../../include/etude_hip_debug.h"

#define RS_TILE 256                 // consecutive outputs of one (song, channel) a workgroup produces; one thread per output
#define RS_THREADS 256
#define RS_MAX_TABLE (1LL << 22)    // entries up x K of a handle's table (16 MB of fp32)
#define RS_MAX_CH 8
#define RS_MAX_SONGS 4096
#define RS_MAX_RATE (1 << 30)
#define RS_MAX_N (1LL << 32)        // frames per song

// one song of a call (device table at the head of the workspace, built per call)
struct RsSong {
  const unsigned char* src;         // the raw samples
  float* dst;                       // [C][Nout], or [Nout] when mono
  long long N, Nout;
  int C, fmt, mono;
  float inv_c;                      // 1.f / C
};
// one workgroup of the launch: outputs n0 .. n0 + RS_TILE - 1 (cut at Nout) of channel ch of a song; ch = 0 for a mono song
struct RsTile {
  int song, ch;
  long long n0;
};
