// fp32 PARITY MODE of the Extract stage (etd_ext_cfg.precision == 1): the same model as api_ext.hip / ext_kernels.hip runs,
// with fp32 weights, fp32 activations and exact-fp32 products (v_mfma_f32_32x32x2_f32 for the GEMMs, fmaf elsewhere).
// It exists to pin the arithmetic: the default mode computes in bf16 (fp32 accumulate) and sits within ~6e-2 of the
// reference's probabilities, which moves borderline notes; this mode sits within ~1e-4 and is what the note-level parity test
// runs on.  Simple kernels, no fusion -- ~20x slower than the bf16 path, still seconds per 3-minute clip.
#pragma once
#include <cstdint>
#include "../../include/etude_hip.h"
#include "ext_kernels.h"
#include "host_util.h"

struct Ext32;
struct Outs32 { float *on, *off, *mpe; int8_t* vel; };

int ext32_create(const etd_ext_cfg& cfg, const WeightTable& w, Ext32** out);
void ext32_destroy(Ext32* e);
// windows [0, n_windows) of `src` (EmbedArgs source description: feat_mode / strides as in the bf16 path); one window at a time
int ext32_run(Ext32* e, const EmbedArgs& src, int n_windows, Outs32 B, Outs32 A, void* const* tap, float* dbg_vel, hipStream_t st);
