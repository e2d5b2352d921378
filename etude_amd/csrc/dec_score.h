// Teacher-forced scoring of the EtudeDecoder: per-row log-probabilities of given labels and their per-sequence sums
// (etd_decoder_score, etd_decoder_score_jobs).  The logits come from the model's own LM head (api_dec.hip: head_logits).
// Reference: F.cross_entropy(logits.view(-1, V), labels.view(-1)) of etude/models/etude_decoder.py:196-198 (ignore index -100).
#pragma once
#include "common.h"

#define ETD_IGNORE_LABEL (-100)

// One wave per logits row j < n (row stride ldl, V entries): lse = max + log(sum exp(l - max)) in fp32, the argmax with
// launch_dargmax's tie rule (lowest index, torch.argmax), lp = l[label] - lse (0 for label -100).  Row j's results and label
// live at row out_row[j] of the row arrays: lp[], lse[], amax[] are written there, labels[] is read there.
int launch_row_logprob(const float* logits, int ldl, int V, int n, const int* out_row, const int* labels,
                       float* lp, float* lse, int* amax, hipStream_t st);

// One workgroup per sequence s < n_seq (rows [row0[s], + len[s]) of the row arrays): in a fixed order, the double sum of lp over the
// rows whose label is not -100, their count, and the count of those whose argmax equals the label.
int launch_seq_reduce(const int* row0, const int* len, int n_seq, const int* labels, const float* lp, const int* amax,
                      double* seq_lp, int* seq_tokens, int* seq_hits, hipStream_t st);
