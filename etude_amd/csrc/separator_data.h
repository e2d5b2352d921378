// Training data of the source separator (csrc/separator_data.hip): what the gather kernel and its host side share.  DESIGN.md 4o is the contract.
#pragma once
#include "host_util.h"
#include "../../include/etude_hip.h"

#define SD_THREADS 256

// One unit of a batch: its track's magnitudes S [1 + I][frames][F][C] (ks floats per source), the track's Tf, the start frame and the stretched sizes
// T' = floor(T a), F' = floor(F q), formed on the host in double.
struct SdUnit {
  const float* S; long long ks;
  int Tf, t0, Tp, Fp;
};

// the stems of etd_sepdata_sum_stems, by value
struct SdStems { const float* p[ETD_SEP_MAX_INSTR]; };
