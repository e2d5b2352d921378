// Beat-Transformer engine (Demixed_DilatedTransformerModel, etude/models/beat_transformer.py:23-106): the exact-parity (fp32-grade) forward pass of beat / downbeat
// logits and the tempo head.  Dense contractions on csrc/gemm3.h; the conv front end's pooling, the dilated 5-tap attention, the 5-token instrument attention, the
// skip accumulation and the two heads are the kernels of beat.hip.  The C entry points are etd_beat_* (include/etude_hip.h).
#pragma once
#include "gemm3.h"

#define BEAT_HEADS 8
#define BEAT_HEAD_DIM 32
#define BEAT_DMODEL 256
#define BEAT_TAPS 5
#define BEAT_MELS 128
#define BEAT_C1 32            // conv1 channels; pooled width 42 (126 / 3)
#define BEAT_W1 42
#define BEAT_C2 64            // conv2 channels; the conv2 GEMM runs over all 42 pooled conv1 columns (overlapping rows of the [row][42][32] buffer), 0 .. 23 are used
#define BEAT_K2 384           // 12 x 32
#define BEAT_K3 1152          // 3 x 6 x 64
#define BEAT_SEG 128          // frames per partial sum of the tempo head's time mean
