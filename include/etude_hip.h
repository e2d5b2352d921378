/* etude_hip.h -- C ABI of libetude_hip.so: the MI355X (gfx950) implementation of Etude's two compute
 * hot paths.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (Xiugapurin/Etude) is pure Python and has no FFI; the "interface each entry point
 * replaces" is therefore the Python call it stands in for (file:line under /root/reference):
 *
 *   etd_frontend_*        AMTAPC_Extractor._wav2feature               etude/data/extractor.py:178-197
 *                         (torchaudio Resample + MelSpectrogram + log)
 *   etd_extractor_create  _load_model + _Spec2MIDI construction        etude/data/extractor.py:78-113
 *   etd_transcript        AMTAPC_Extractor._transcript                 etude/data/extractor.py:199-253
 *   etd_transcript_windows  _Spec2MIDI.forward on [B,n_bin,n_frame+2m] etude/data/extractor.py:53-56,
 *                         = Model_SPEC2MIDI.forward                    etude/models/amt_apc.py:29-49
 *   etd_mpe2note, etd_mpe2note_dev  AMTAPC_Extractor._mpe2note (host / device)  etude/data/extractor.py:256-418
 *   etd_decoder_create    load_etude_decoder + EtudeDecoder.__init__   etude/utils/model_loader.py:12-60,
 *                                                                      etude/models/etude_decoder.py:94-123
 *   etd_decoder_begin_bar / etd_decoder_step / etd_decoder_poll / etd_decoder_read_tokens
 *                         the body of EtudeDecoder.generate's token loop: forward (embeddings +
 *                         GPT-NeoX + lm_head) + greedy argmax + KV cache  etude/models/etude_decoder.py:300-343,148-206
 *   etd_decoder_generate_bar  one bar of generate(): prefill + <=limit greedy steps, stop at Bar_EOS
 *                                                                      etude/models/etude_decoder.py:291-343
 *   etd_decoder_score     EtudeDecoder.forward(..., labels=...) -> .loss / .logits    etude/models/etude_decoder.py:148-206
 *   etd_decoder_score_jobs  teacher-forced per-bar log-likelihood of covers under generate()'s prompt rule  :246-354
 *   etd_beat_create       BeatDetector._load_model                      etude/data/beat_detector.py:79-97
 *   etd_beat_forward      Demixed_DilatedTransformerModel.forward      etude/models/beat_transformer.py:56-106,
 *                         (conv front end + 9 dilated layers + 3       etude/models/layers/dilated_transformer_layer.py:37-180
 *                         instrument layers + beat / tempo heads)      (BeatDetector.detect's model call: etude/data/beat_detector.py:121-127)
 *   etd_stemfeat_run      process_stems_to_spectrogram (stft + mel +    scripts/run_separation.py:124-141, 163-183
 *                         power_to_db per separated stem)
 *   etd_dtw_align         AudioAligner._compute_warping_path behind the  etude/data/aligner.py:106-133
 *                         features: CENS, optimal chroma shift, DTW,
 *                         strictly monotonic path, pitch_shift
 *   etd_tuning_run        estimate_tuning(audio, fs) of                  etude/data/aligner.py:100-101
 *                         AudioAligner._compute_alignment
 *   etd_resample_run      librosa.load(path, sr=22050) behind the walk   etude/data/aligner.py:71-72,
 *                         over the WAV's chunks; torchaudio.load          scripts/run_separation.py:89
 *   etd_rhythm_run       RGCCalculator / IPECalculator .calculate       etude/evaluation/metrics/rgc.py, ipe.py
 *   etd_attr_run          EtudeDataset._extract_bar_features,             etude/data/dataset.py:204-270, 335-339
 *                         _compute_musical_attributes, _get_attribute_bin_id
 *
 * Conventions: every function returns 0 on success or a negative errno-style code (ETD_E*); the
 * message is available from etd_last_error() (thread-local).  "dev" pointers are device (HBM)
 * addresses valid in the calling process's HIP context, "host" pointers are ordinary memory.  The
 * caller owns every buffer it passes; the library owns only what *_create allocated and frees it in
 * *_destroy.  `stream` is a hipStream_t (NULL = default stream).  Calls on one handle are not
 * re-entrant; launches are asynchronous on `stream` unless stated otherwise.
 */
#ifndef ETUDE_HIP_H
#define ETUDE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: 1 = rounds 1-2 (etd_ext_cfg without `precision` / etd_sched_cfg without the job keys in its first builds);
 * 2 = round 3: struct_bytes leads every config struct, so a caller compiled against another layout is refused instead of misread;
 * etd_decoder_stats / _stats_reset / _stamp added; the diagnostic hooks moved to etude_hip_debug.h;
 * 3 = round 6 (the change itself is round 5's): the element type of every 16-bit buffer reachable through this API -- KV cache rows, activation taps and peeks of the
 * debug header -- is IEEE half (was bf16; `etd_decoder_operand_type` / `etd_extractor_operand_type` name the type of a given build); `etd_frontend_run(feat = NULL)`
 * sizes its output; no struct layout changed. */
#define ETD_ABI_VERSION 3
#define ETD_OK 0
#define ETD_EINVAL (-22)
#define ETD_ENOMEM (-12)
#define ETD_EHIP (-5)
#define ETD_EIO (-6)      /* host file I/O failed (etd_midi_write) */

int etd_version(void);
const char* etd_last_error(void);
/* Hash of the sources this binary was built from (etude_amd/build.py: src_hash); the Python binding refuses a library whose
 * id differs from the tree it sits in, so a stale in-tree .so cannot stand in for the current kernels. */
const char* etd_build_id(void);

/* ------------------------------------------------------------------ launch profiler (measurement only)
 * When enabled, every kernel launch of the library is bracketed by HIP events on its own stream;
 * etd_prof_collect() synchronises them and accumulates per-kernel totals. */
int etd_prof_enable(int on);
int etd_prof_reset(void);
int etd_prof_collect(void);
int etd_prof_count(void);
int etd_prof_entry(int i, char* name, int name_cap, double* total_ms, long long* launches, double* flops, double* bytes);

/* ------------------------------------------------------------------ audio front end */
typedef struct etd_frontend etd_frontend;
/* Tables are built by the host layer exactly as torchaudio builds them:
 *   kernT_host [K][nw]   polyphase sinc kernel, transposed (k-major); orig/nw = sr_in/gcd, sr_out/gcd
 *   window_host[n_fft]   periodic Hann
 *   mel filterbank in CSR form: filter m covers power-spectrum bins [mel_start[m], +mel_len[m]) with
 *   weights mel_w[sum(mel_len[:m]) ...].
 * The resampler holds 7 * orig + K input samples in LDS: a rate pair whose span exceeds the device's per-workgroup
 * shared-memory limit is refused here with ETD_EINVAL and a message naming the pair; nothing is uploaded or launched.  */
int etd_frontend_create(int sr_in, int sr_out, int orig, int nw, int K, int width, const float* kernT_host,
                        int n_fft, int hop, const float* window_host, int n_mels, const int* mel_start,
                        const int* mel_len, const float* mel_w_host, float log_offset, etd_frontend** out);
void etd_frontend_destroy(etd_frontend*);
/* STFT centre padding: 0 = reflect (AMTAPC_Extractor, torchaudio default), 1 = zeros (HFT_Transformer: pad_mode="constant",
 * etude/models/hft_transformer.py:124-131) */
int etd_frontend_set_pad_mode(etd_frontend*, int constant_zero);
/* frame-wise RMS of a mono device signal: out[t] = sqrt(mean(x[t*hop - frame/2 .. + frame)^2)), zeros outside the signal
 * (librosa.feature.rms, center=True) -- the volume contour of analyze_volume, etude/utils/preprocess.py:116-152 */
int etd_rms_frames(const float* x_dev, long long n, int frame_length, int hop_length, float* out_dev, long long n_frames, void* stream);
long long etd_frontend_resampled_len(const etd_frontend*, long long n_in);
long long etd_frontend_num_frames(const etd_frontend*, long long n_in);
/* wav_dev: planar [channels][n_in] fp32.  resampled_dev: scratch >= resampled_len floats.
 * feat_dev: [T][n_mels] fp32 log-mel, T = 1 + resampled_len / hop (written to *n_frames_out); NULL = channel mean + resample only (what
 * analyze_volume needs of this stage: etude/utils/preprocess.py:135), *n_frames_out = 0. */
int etd_frontend_run(etd_frontend*, const float* wav_dev, int channels, long long n_in, float* resampled_dev,
                     float* feat_dev, long long feat_capacity_frames, long long* n_frames_out, void* stream);

/* ------------------------------------------------------------------ extractor (hFT-Transformer) */
typedef struct etd_ext etd_ext;
typedef struct {
  int struct_bytes;       /* sizeof(etd_ext_cfg) of the caller: a mismatch is ETD_EINVAL */
  int n_margin, n_frame, n_bin, cnn_channel, cnn_kernel, hid_dim, pf_dim, n_heads;
  int n_layers_enc, n_layers_dec, n_note, n_velocity;
  float min_value;        /* -18.0: padding value of _transcript */
  int max_windows;        /* windows processed per internal batch (workspace size) */
  int chunk_frames;       /* frames per encoder/freq-decoder chunk (0 = default) */
  int precision;          /* 0 = the 16-bit serving mode: IEEE-half operands (etd_extractor_operand_type), fp32 accumulate / LayerNorm / softmax /
                             sigmoid (default, the fast path);
                             1 = exact-parity mode: fp32 weights and activations, fp32-grade products (two-plane f16 splits on the matrix cores:
                             csrc/gemm3.h, csrc/ext_fp32.hip), one window at a time -- what the note-level parity tests run on.
                             Architectures (etude/config/schema.py:100-112): mode 0 is built for the reference's default one (hid 256 / 4 heads / pf 512 /
                             256 bins / margin 32 / conv 4 x 5 / 3 + 3 layers / 128 velocities, n_frame % 32 == 0, n_note % 4 == 0 <= 128) and refuses any
                             other; mode 1 takes hid_dim = 64 * n_heads <= 512, pf_dim % 32 == 0, n_bin % 32 == 0, n_margin <= 64,
                             cnn_kernel <= 2 * n_margin + 1, any layer / note / frame counts, n_velocity <= 128 */
} etd_ext_cfg;
/* element type of the 16-bit serving mode's operands and activation buffers (debug taps): 1 = IEEE half (the default build), 0 = bf16 (-DETD_EXT_BF16) */
int etd_extractor_operand_type(void);
/* Weights: n named fp32 host tensors with the reference checkpoint's own keys ("encoder.*",
 * "decoder.*"); every key the model needs must be present with the right element count. */
int etd_extractor_create(const etd_ext_cfg* cfg, const char* const* names, const float* const* host_ptrs,
                         const int64_t* numels, int n, etd_ext** out);
void etd_extractor_destroy(etd_ext*);
/* feat_dev [T][n_bin] fp32 -> outputs over T_pad = ceil(T/n_frame)*n_frame rows of n_note:
 * onset/offset/mpe fp32 probabilities and int8 velocity argmax of the time ("B") heads; the "A"
 * (frequency) head outputs are produced only when all four *_A pointers are non-NULL.
 * PRECONDITION on the input (both entry points, both precisions): log-mel features lie in [-F, F], F = max(|min_value|, 32) -- what
 * log(mel + 1e-8) of audio in [-1, 1] gives (>= -18.4, < 15) and what the wrappers pad with (-18 / -80).  The library's 16-bit operand
 * planes (IEEE half; in the exact-parity mode the two-plane splits of csrc/gemm3.h) are scaled from bounds that assume it; finite features
 * beyond it (a spectrogram of int16-scale samples) can overflow a plane into Inf / NaN probabilities.  Not checked here (the call is
 * asynchronous); the Python mirror checks it (AMTAPC_Extractor.check_feature_range). */
int etd_transcript(etd_ext*, const float* feat_dev, long long T,
                   float* onset_B, float* offset_B, float* mpe_B, int8_t* vel_B,
                   float* onset_A, float* offset_A, float* mpe_A, int8_t* vel_A, void* stream);
/* spec_dev [B][n_bin][n_frame + 2*n_margin] fp32 (the model's own input layout) -> [B*n_frame][n_note]. */
int etd_transcript_windows(etd_ext*, const float* spec_dev, int B,
                           float* onset_B, float* offset_B, float* mpe_B, int8_t* vel_B,
                           float* onset_A, float* offset_A, float* mpe_A, int8_t* vel_A, void* stream);
/* algorithmic FLOPs of one n_frame window (SURVEY.md 8d formula) */
double etd_extractor_window_flops(const etd_ext*);

/* ------------------------------------------------------------------ notes (host) */
typedef struct { double onset, offset; int32_t pitch, velocity; } etd_note;
/* onset/offset/mpe [T][n_note] fp32 host, velocity [T][n_note] int8 host -> notes sorted by (onset, pitch).
 * Keeps the reference's numerics as it runs under numpy>=2 (see oracle/mpe2note.py).  Returns the
 * number of notes in *n_out; fails with ETD_ENOMEM if cap is too small (n_out = needed). */
int etd_mpe2note(const float* onset, const float* offset, const float* mpe, const int8_t* velocity, long long T,
                 int n_note, float thred_onset, float thred_offset, float thred_mpe, int hop_sample, int sr,
                 int note_min, etd_note* out, long long cap, long long* n_out);
/* The same with the reference's two mode switches (extractor.py:256-258): mode_velocity "ignore_zero" (default) drops notes whose
 * velocity argmax is 0, "org" keeps them; mode_offset picks, when both an offset peak and an mpe drop exist, the earlier one
 * ("shorter", default), the later one ("longer") or always the offset peak ("offset") (:386-404).  The device path has the same
 * switches (etd_mpe2note_dev_modes); etd_mpe2note / etd_mpe2note_dev are the defaults, which is all the reference's callers use. */
enum { ETD_M2N_VEL_IGNORE_ZERO = 0, ETD_M2N_VEL_ORG = 1 };
enum { ETD_M2N_SHORTER = 0, ETD_M2N_LONGER = 1, ETD_M2N_OFFSET = 2 };
int etd_mpe2note_modes(const float* onset, const float* offset, const float* mpe, const int8_t* velocity, long long T, int n_note,
                       float thred_onset, float thred_offset, float thred_mpe, int hop_sample, int sr, int note_min,
                       int mode_velocity, int mode_offset, etd_note* out, long long cap, long long* n_out);
/* The same conversion on the DEVICE: the four frame-wise arrays stay in HBM ([T][n_note], as
 * etd_transcript wrote them), only the notes come back, already in the reference's order.  Bit-identical to etd_mpe2note.
 * The handle owns scratch that grows to the largest T seen; calls on one handle are not re-entrant. */
typedef struct etd_m2n etd_m2n;
int etd_mpe2note_dev_create(int n_note, etd_m2n** out);
void etd_mpe2note_dev_destroy(etd_m2n*);
int etd_mpe2note_dev(etd_m2n*, const float* onset_dev, const float* offset_dev, const float* mpe_dev, const int8_t* vel_dev,
                     long long T, float thred_onset, float thred_offset, float thred_mpe, int hop_sample, int sr, int note_min,
                     etd_note* out_host, long long cap, long long* n_out, void* stream);
int etd_mpe2note_dev_modes(etd_m2n*, const float* onset_dev, const float* offset_dev, const float* mpe_dev, const int8_t* vel_dev,
                           long long T, float thred_onset, float thred_offset, float thred_mpe, int hop_sample, int sr, int note_min,
                           int mode_velocity, int mode_offset, etd_note* out_host, long long cap, long long* n_out, void* stream);

/* ------------------------------------------------------------------ decoder (EtudeDecoder / GPT-NeoX) */
typedef struct etd_dec etd_dec;
typedef struct {
  int struct_bytes;       /* sizeof(etd_dec_cfg) of the caller */
  int vocab_size, hidden_size, num_hidden_layers, num_attention_heads, intermediate_size;
  int max_position_embeddings, num_classes, num_attribute_bins, attribute_emb_dim;
  float rotary_pct, rope_theta, layer_norm_eps;
  int max_streams;        /* concurrent token streams (KV slots) */
  int max_ctx;            /* KV positions per stream */
  int precision;          /* 0 = exact-parity mode: fp32 weights, activations and KV cache, fp32-grade products (csrc/gemm3.h) -- the reference's token ids;
                             1 = the 16-bit serving mode: IEEE-half weights, LayerNorm rows and KV cache (etd_decoder_operand_type), fp32 residual stream /
                             accumulators / softmax / logits */
  int max_prefill_rows;   /* prompt rows one etd_decoder_begin_bars call may carry (0 = max(max_ctx, max_streams)) */
} etd_dec_cfg;
int etd_decoder_create(const etd_dec_cfg* cfg, const char* const* names, const float* const* host_ptrs,
                       const int64_t* numels, int n, etd_dec** out);
/* element type of the 16-bit serving mode (weights, KV cache, debug peeks): 1 = IEEE half (the default build), 0 = bf16 (-DETD_DEC_BF16) */
int etd_decoder_operand_type(void);
/* 1 when built with -DETD_EXPERIMENTS (the in-launch row finish and the 8 / 16-wave attention forms compiled in; ETD_ROWFIN, ETD_AD_WAVES, ETD_LAUNCH_LOG and
 * ETD_NO_GRAPH live); the shipped build returns 0 and has one path per precision */
int etd_has_experiments(void);
void etd_decoder_destroy(etd_dec*);
/* A second engine over the SAME weights: own KV cache, workspaces and stream state (same cfg), the weight buffers of `src`
 * (or of the handle `src` was cloned from) are shared, not copied -- concurrent engines then stream one weight set through
 * the caches instead of one copy each.  Handles may be destroyed in any order and from any thread (the family's reference count
 * is kept under a lock); the weights go with the last one.  Using the handles concurrently, one host thread per handle, is what
 * they are for. */
int etd_decoder_clone(etd_dec* src, etd_dec** out);
/* Start one bar on stream `slot` (etude_decoder.py:291-297 + first loop iteration): reset the slot's KV
 * cache and generation state, run the prompt (ids/cls: int32 host [T]; attrs4: int32 host [4][T] in the
 * concat order of etude_decoder.py:171-176 = pitch_overlap, polyphony, note_sustain, rhythm_intensity)
 * through the model and leave the greedy first token in the slot's device-side state.  tgt_attrs4 (same
 * order) condition the generated tokens; generation stops at eos_id or after `limit` tokens.  The bar needs T + limit - 1
 * KV positions: ETD_EINVAL when that exceeds max_ctx (the reference's dynamic cache / on-the-fly rotary has no such bound,
 * etude_decoder.py:285-300; EtudeDecoder sizes max_ctx so that every legal generate() argument set fits). */
/* Sampling branch of generate() (etude_decoder.py:321-331): temperature > 0 -> softmax(logits / T), top-p filter when
 * 0 < top_p < 1, one draw per token; temperature == 0 -> greedy argmax (the default).  Draws are a pure function of (seed, the
 * stream's key, index of the token inside its bar) -- reproducible, independent of slot / engine placement; the reference
 * draws from torch's global generator instead, so parity is distributional (tests/test_gpu_sampling.py).  Keys default to
 * the slot index; etd_decoder_run_jobs sets key = (job index, bar index). */
int etd_decoder_set_sampling(etd_dec*, float temperature, float top_p, unsigned long long seed, void* stream);
int etd_decoder_set_keys(etd_dec*, int n, const int32_t* slots, const unsigned long long* keys);
int etd_decoder_begin_bar(etd_dec*, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                          const int32_t* tgt_attrs4, int eos_id, int limit, void* stream);
/* Batched form: n bars at once (distinct slots).  T[i] = prompt length of bar i; ids/cls hold the prompts back to
 * back (sum(T) rows), attrs4 is [4][sum(T)]; tgt_attrs4 [n][4], eos_ids [n], limits [n].  All prompts go through the
 * model as ONE pass (big-tile MFMA GEMMs over sum(T) rows in bf16 mode). */
int etd_decoder_begin_bars(etd_dec*, int n, const int32_t* slots, const int32_t* T, const int32_t* ids, const int32_t* cls,
                           const int32_t* attrs4, const int32_t* tgt_attrs4, const int32_t* eos_ids, const int32_t* limits, void* stream);
/* n_steps greedy decode steps for the n_active streams listed in `slots` (host array): each step feeds every
 * stream's current token (class TGT=2, its target attrs), appends K/V, and writes the argmax back as the
 * stream's current token and into its output ring -- all on the device: no host sync, no allocation.
 * Streams that already finished (EOS / limit) idle. */
int etd_decoder_step(etd_dec*, const int32_t* slots, int n_active, int n_steps, void* stream);
/* done flag and number of generated tokens of each listed stream (synchronises the stream). */
int etd_decoder_poll(etd_dec*, const int32_t* slots, int n, int32_t* done_out, int32_t* n_out_out, void* stream);
/* Copy out the tokens generated so far by `slot` (synchronises). *n = count. */
int etd_decoder_read_tokens(etd_dec*, int slot, int32_t* out, int cap, int* n, void* stream);
/* The same for n streams with ONE synchronisation: out is [n][cap], counts [n]. */
int etd_decoder_read_many(etd_dec*, int n, const int32_t* slots, int32_t* out, int cap, int32_t* counts, void* stream);
/* The whole bar loop of EtudeDecoder.generate (etude_decoder.py:246-354: prompt assembly, history window, truncation,
 * token budget, Bar_EOS stop) for MANY independent jobs, scheduled natively as concurrent device streams.  A job is
 * one (song, attribute tuple): x_ids = its condition bars back to back, x_offsets [n_bars+1], attrs4 [n_bars][4] in
 * C-ABI attribute order.  Result: out[job_offsets[j] ..] = [n_bars_done, len_0 .., tokens of bar 0 ([Bar_BOS]+generated), ...].
 * `ready` (may be null = ready now) points at a host int another thread sets non-zero once the job's condition bars are
 * valid -- the upstream pipeline stages (infer.py:82-163: extract .. tokenize) of that song have finished; the scheduler
 * admits jobs in list order and never reads x_ids/x_offsets/attrs4 of a job before its flag is set. */
typedef struct { const int32_t* x_ids; const int32_t* x_offsets; int n_bars; const int32_t* attrs4; const int32_t* ready; } etd_job;
typedef struct {
  int struct_bytes;       /* sizeof(etd_sched_cfg) of the caller */
  int bar_bos_id, bar_eos_id, n_ctx_pairs, max_position_embeddings, max_output_tokens, max_bar_token_limit;
  float context_overlap_ratio;
  int force_bar_tokens;   /* >0 (benchmarks): suppress Bar_EOS, every bar is exactly this many tokens */
  int max_streams, max_prefill_rows, steps_per_poll;
  float temperature, top_p;            /* etude_decoder.py:213-214; temperature 0 = greedy */
  unsigned long long seed;
  int job_key_offset, job_key_stride;  /* sampling keys: job k of THIS call is global job job_key_offset + k * max(job_key_stride, 1), so that several
                                          engines sharing one job list (run_engines deals it round-robin) draw independent streams */
} etd_sched_cfg;
int etd_decoder_run_jobs(etd_dec*, const etd_sched_cfg* cfg, const etd_job* jobs, int n_jobs, int32_t* out, long long out_cap,
                         long long* job_offsets, long long* n_steps_out, void* stream);
/* begin_bar + steps until done + read_tokens for one stream.  Synchronous. */
int etd_decoder_generate_bar(etd_dec*, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                             const int32_t* tgt_attrs4, int eos_id, int limit, int32_t* out, int* n_out, void* stream);
/* test hook: full logits [T][vocab] fp32 of a prompt (EtudeDecoder.forward), copied to the host. */
int etd_decoder_prefill_logits(etd_dec*, int slot, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, int T,
                               float* logits_host, void* stream);
/* Teacher-forced scoring (EtudeDecoder.forward with labels, etude_decoder.py:148-206: F.cross_entropy with ignore index -100, labels NOT shifted).
 * n sequences packed as for etd_decoder_begin_bars: T[n] rows each, ids / cls / labels int32 host [M = sum(T)], attrs4 int32 host [4][M] (C-ABI attribute
 * order).  A row's label is the token it should predict, or -100 (not scored).  Per sequence: seq_logprob = sum over its labelled rows of
 * log_softmax(logits)[label] (double), seq_tokens = labelled rows, seq_hits = labelled rows whose argmax (lowest index on ties) is the label.
 * Optional (NULL = not wanted): row_lp [M] (0 on rows not scored) and row_argmax [M] (-1 on rows not scored) host; logits_dev = DEVICE fp32 [M][vocab]:
 * then EVERY row's logits are written there and every row has an argmax.  Sequences are chunked internally (<= max_streams sequences and
 * <= max_prefill_rows rows per pass; a sequence may not exceed max_ctx rows).  Out-of-range ids / classes / attribute bins / labels are ETD_EINVAL
 * before anything runs.  The handle's KV slots serve as scratch: a score call and a generate call (begin_bars / step / run_jobs) on one handle must
 * not overlap, and a stream's state does not survive a score call (etd_decoder_run_jobs starts every bar afresh).  Synchronous. */
int etd_decoder_score(etd_dec*, int n, const int32_t* T, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, const int32_t* labels,
                      double* seq_logprob, int32_t* seq_tokens, int32_t* seq_hits, float* row_lp, int32_t* row_argmax, float* logits_dev, void* stream);
/* Teacher-forced log-likelihood of given covers under generate()'s own context rule.  A job = condition bars as in etd_job (x_ids, x_offsets
 * [n_bars + 1], attrs4 [n_bars][4]) + cover bars y_ids / y_offsets [n_y_bars + 1] as generate returns them ([Bar_BOS] + tokens each; n_y_bars <=
 * n_bars: a budget-stopped cover scores the bars it has).  Bar i is scored as the sequence prompt(history of the given bars 0..i-1, x_i) + y_i[1:-1]
 * with labels -100 on the prompt rows but the last, then y_i[1:] -- the logits generate() saw while producing y_i (same prompt assembly,
 * truncation and history window as etd_decoder_run_jobs, from cfg's bar ids / n_ctx_pairs / max_position_embeddings / max_bar_token_limit /
 * context_overlap_ratio).  Outputs per bar, jobs back to back (sum of n_y_bars entries): bar_logprob, bar_tokens (= len(y_i) - 1), bar_hits.
 * A bar of [Bar_BOS] only scores 0 tokens; a bar of more than max_bar_token_limit tokens, or not led by Bar_BOS, is ETD_EINVAL.
 * All bars of all jobs go through etd_decoder_score in one call (same rules on the handle's slots). */
typedef struct { const int32_t* x_ids; const int32_t* x_offsets; int n_bars; const int32_t* attrs4; const int32_t* y_ids; const int32_t* y_offsets; int n_y_bars; } etd_score_job;
int etd_decoder_score_jobs(etd_dec*, const etd_sched_cfg* cfg, const etd_score_job* jobs, int n_jobs, double* bar_logprob, int32_t* bar_tokens,
                           int32_t* bar_hits, void* stream);
/* algorithmic HBM bytes of one decode step for n_streams at context `ctx` (SURVEY.md 8d formula) */
double etd_decoder_step_bytes(const etd_dec*, int n_streams, int ctx);
/* Exact host-side accounting of the decode steps issued on this handle since the last reset (graph replays included):
 *   out[0] steps, out[1] rows x steps (= tokens generated by steps), out[2] algorithmic K/V bytes the steps' attention read (all layers),
 *   out[3] attention launches, out[4] launches measured by the device stamps, out[5] their summed duration in seconds,
 *   out[6] algorithmic bytes (K/V + streamed weights) of the stamped launches, out[7] weight bytes one step streams (SURVEY 8d "W").
 * etd_decoder_stamp(on, skip_steps): while on, every k_dstep_attn_down launch of this handle records its own span on the device
 * (s_memrealtime of its first workgroup's start and last workgroup's end) -- the kernel's duration in the configuration it
 * actually runs in, other engines included, which HIP events cannot give inside hipGraph replays.  The first `skip_steps` decode
 * steps after switching on are left out (bytes and spans alike), e.g. the bars in which a job's 4-pair history is still filling up.
 * Stamped steps use their own captured graphs; production graphs carry no stamp code path.  All three synchronise `stream`. */
int etd_decoder_stats(etd_dec*, double* out, int n, void* stream);
int etd_decoder_stats_reset(etd_dec*, void* stream);
int etd_decoder_stamp(etd_dec*, int on, int skip_steps, void* stream);
/* (start, end) of every stamped attention launch since the last reset, in 100 MHz ticks of the device's s_memrealtime -- ONE clock for every queue of the chip, so the
 * logs of several engines can be merged into the union of the times an attention launch was running (bench.py: the roofline of concurrent engines is bytes of all
 * launches / that union, not a per-launch fraction).  out_pairs [cap][2]; *n = launches written (the log keeps the first 131 072 per handle). */
int etd_decoder_stamp_log(etd_dec*, unsigned long long* out_pairs, long long cap, long long* n, void* stream);
/* ---- TinyREMITokenizer glue on either side of the decoder (host code, no GPU) ----
 * etd_tok_create      TinyREMITokenizer.__init__ / _create_measures      etude/data/tokenizer.py:24-41,166-229
 * etd_tok_encode      encode (+ _assign_notes, grace-note linking)        :231-252, :78-116, :265-297
 * etd_tok_split_bars  split_sequence_into_bars                            :43-76
 * etd_tok_decode      decode_to_notes (+ glissandos, velocities, sort)    :300-496
 * Results are bit-identical to the reference (same double arithmetic, tie-breaking and summation orders). */
typedef struct { double bpm; int time_sig; double start; const double* downbeats; int n_downbeats; } etd_tempo_region;
enum { ETD_EV_BAR = 0 /* value 1 = BOS, 0 = EOS */, ETD_EV_POS = 1, ETD_EV_NOTE = 2, ETD_EV_DURATION = 3, ETD_EV_GRACE = 4, ETD_EV_OTHER = 5 };
typedef struct { int32_t type; int32_t value; } etd_event;
typedef struct etd_tok etd_tok;
int etd_tok_create(const etd_tempo_region* regions, int n_regions, etd_tok** out);
void etd_tok_destroy(etd_tok*);
int etd_tok_num_measures(const etd_tok*);
int etd_tok_measures(const etd_tok*, double* start, double* end, double* bpm, int32_t* time_sig);
int etd_tok_encode(const etd_tok*, const etd_note* notes, long long n, int with_grace_note, etd_event* out, long long cap, long long* n_out);
int etd_tok_split_bars(const int32_t* ids, long long n, int bar_bos_id, int bar_eos_id, int32_t* out_ids, long long cap_ids,
                       long long* bar_offsets, long long cap_bars, long long* n_bars);
int etd_tok_decode(const etd_tok*, const etd_event* events, long long n, const double* volume /* or NULL */, long long n_volume,
                   etd_note* out, long long cap, long long* n_out);

/* ------------------------------------------------------------------ MIDI output (host)
 * TinyREMITokenizer.note_to_midi, etude/data/tokenizer.py:499-524 (infer.py:207): the notes as a format-1 Standard MIDI
 * File exactly as `pretty_midi.PrettyMIDI()` + one `Instrument(program=0)` + `.write()` lays it out (220 ticks per beat,
 * 120 bpm, tick = round(time * 440)).  pitch / velocity outside 0..127 fail with ETD_EINVAL (mido raises there). */
int etd_midi_write(const etd_note* notes, long long n, const char* path);

/* ------------------------------------------------------------------ Beat-Transformer (beat / downbeat activations; exact-parity fp32-grade arithmetic)
 * Demixed_DilatedTransformerModel (etude/models/beat_transformer.py:23-106) as BeatDetector builds it (etude/data/beat_detector.py:79-97, schema.py:134-158).
 * madmom's DBN trackers that turn the activations into beat times stay with the caller. */
typedef struct etd_beat etd_beat;
typedef struct {
  int struct_bytes;       /* sizeof(etd_beat_cfg) of the caller: a mismatch is ETD_EINVAL */
  int attn_len, instr, ntoken, dmodel, nhead, d_hid, nlayers, norm_first, n_mels, tempo_out;
  int max_rows;           /* rows (instr x frames) per internal chunk: the workspace size (a single longer song gets a workspace of its own size) */
} etd_beat_cfg;
/* Weights: n named fp32 host tensors with the checkpoint's own keys (181 for the default architecture); a missing key or a wrong element count is ETD_EINVAL.
 * Architectures: nhead = 8 and attn_len = 5 (the reference's dilated head table is written for them), dmodel = 256, n_mels = 128, norm_first = 1, instr <= 8,
 * d_hid % 256 == 0; anything else is refused with ETD_EINVAL before any HIP call. */
int etd_beat_create(const etd_beat_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n, etd_beat** out);
void etd_beat_destroy(etd_beat*);
/* feat_dev: the n_seq songs' [instr][T_s][n_mels] fp32 blocks back to back (T_host[s] >= 1 frames each); logits_dev [sum T_s][ntoken]; tempo_dev [n_seq][tempo_out]
 * (NULL: not computed).  A song's outputs do not depend on the other songs of the call or on the chunking.  Synchronises `stream` once at the start (song table upload).
 * PRECONDITION: finite features with |x| <= 80 (power_to_db's top_db floor); the plane scales are bounds derived from it.  Not checked here; the Python mirror checks it. */
int etd_beat_forward(etd_beat*, const float* feat_dev, int n_seq, const int64_t* T_host, float* logits_dev, float* tempo_dev, void* stream);
/* algorithmic FLOPs of one song of T frames (the reference's full convolutions; formula in DESIGN.md) */
double etd_beat_flops(etd_beat*, long long T);

/* ------------------------------------------------------------------ DBN beat / downbeat tracking (activations -> beat frames; fp64 log-space Viterbi on the device)
 * What BeatDetector.detect does with the activations (etude/data/beat_detector.py:133-150): madmom 0.16's DBNBeatTrackingProcessor and DBNDownBeatTrackingProcessor,
 * restated from their published description (DESIGN.md 4c is the contract; parity with madmom itself is unpinned).  HMM 0 is the beat HMM, HMM 1 + i the bar HMM of
 * beats_per_bar[i] beats.  Not implemented: online mode, correct = 0, per-beat transition_lambda lists. */
typedef struct etd_dbn etd_dbn;
typedef struct {
  int struct_bytes;       /* sizeof(etd_dbn_cfg) of the caller: a mismatch is ETD_EINVAL */
  double fps, min_bpm, max_bpm;
  double transition_lambda;   /* 100 */
  double observation_lambda;  /* 16; must be > 1 */
  double threshold;           /* activations below it are trimmed from both ends (compared in fp32); 0 = no trimming */
  int correct;                /* 1: a beat sits on the strongest frame of its beat-state run (the only mode) */
  int num_tempi;              /* 0 = every integer interval; else that many log-spaced ones */
  int n_bars;                 /* bar HMMs: entries of beats_per_bar in use, 0..8 */
  int beats_per_bar[8];       /* each 1..8 */
} etd_dbn_cfg;
/* HOST ONLY (no GPU): the state space of one HMM.  intervals_out [cap] (may be NULL), *n_intervals, *n_states, *num_beats; optional logtrans_out [n][n]
 * (from-major: log probability of last state of interval `from` -> first state of interval `to` of the next beat, -inf = no edge) and pointers_out [n_states]
 * (density index per state).  ETD_EINVAL for a bad config: min_bpm >= max_bpm, non-positive fps, beats_per_bar outside 1..8, observation_lambda <= 1.  Any size is described;
 * etd_dbn_create and etd_dbn_workspace_bytes also refuse (ETD_EINVAL, the message names the count) more than 255 intervals or an HMM of more than 8 192 states. */
int etd_dbn_describe(const etd_dbn_cfg* cfg, int hmm_index, int32_t* intervals_out, int cap, int* n_intervals, int* n_states, int* num_beats,
                     double* logtrans_out, uint8_t* pointers_out);
/* HOST ONLY: device workspace bytes one song of T frames needs for HMM hmm_index (-1: all HMMs of the config).  Backpointers are kept for first states only,
 * [T][num_beats * n_intervals] bytes: there is no [T][n_states] array.  Negative (ETD_EINVAL) for a bad config. */
long long etd_dbn_workspace_bytes(const etd_dbn_cfg* cfg, long long T, int hmm_index);
int etd_dbn_create(const etd_dbn_cfg* cfg, etd_dbn** out);
void etd_dbn_destroy(etd_dbn*);
/* in_dev: [sum T_s][2] fp32 device, the n_seq songs back to back; input_kind says what the two columns are: the (beat, downbeat) activations, the logits
 * etd_beat_forward writes (sigmoid applied inside, fp32) -- in both cases the downbeat tracker sees (max(beat - downbeat, 0), downbeat), as detect() builds it --
 * or that combined pair itself, as madmom's DBNDownBeatTrackingProcessor takes it (the beat tracker then sees column 0).
 * Results on the host, song after song: beat_frames[beat_offsets[s] .. beat_offsets[s + 1]) = the beat tracker's beat frames (time = frame / fps);
 * down_frames / down_numbers [down_offsets[s] ..) = the downbeat tracker's (frame, beat number in the bar) rows of the most likely bar length, bar_choice[s]
 * (may be NULL) = its index in beats_per_bar or -1 (no rows).  needed[0], needed[1] = total beats / rows: when beat_cap or down_cap is short the call fails with
 * ETD_ENOMEM and the offsets and `needed` are valid (the contract of etd_mpe2note).  A song's result depends on that song alone.  Synchronous. */
enum { ETD_DBN_IN_ACTIVATIONS = 0, ETD_DBN_IN_LOGITS = 1, ETD_DBN_IN_COMBINED = 2 };
int etd_dbn_track(etd_dbn*, const float* in_dev, int input_kind, int n_seq, const int64_t* T_host,
                  int32_t* beat_frames, long long beat_cap, int64_t* beat_offsets,
                  int32_t* down_frames, int32_t* down_numbers, long long down_cap, int64_t* down_offsets,
                  int32_t* bar_choice, long long* needed, void* stream);

/* ------------------------------------------------------------------ stem mel-dB features (separated stems -> the input of etd_beat_forward)
 * What scripts/run_separation.py:124-141, 163-183 does on the host per stem: channel mean, librosa.stft(n_fft = 4096, hop_length = 1024), |X|^2, the Slaney mel
 * filterbank, librosa.power_to_db(ref = np.max).  DESIGN.md 4d is the contract (parity with librosa itself is unpinned).  Frame t of a stem covers mono samples
 * [t * hop - lead, + n_fft); T = 1 + (N + 2 * lead - n_fft) / hop. */
typedef struct etd_stemfeat etd_stemfeat;
enum {
  ETD_STEMFEAT_LIBROSA = 0,          /* lead = n_fft / 2, zeros outside the signal (librosa >= 0.10, center = True, pad_mode = "constant"): T = 1 + N / hop */
  ETD_STEMFEAT_LIBROSA_REFLECT = 1,  /* lead = n_fft / 2, reflection without edge repeat (librosa < 0.10); N <= n_fft / 2 is refused */
  ETD_STEMFEAT_SPLEETER = 2          /* lead = n_fft, zeros (Spleeter 2.x Separator._stft: n_fft zeros on both ends, center = False): T = 1 + (N + n_fft) / hop */
};
typedef struct {
  int struct_bytes;       /* sizeof(etd_stemfeat_cfg) of the caller: a mismatch is ETD_EINVAL */
  int n_fft;              /* a power of two in 64 .. 4096 */
  int hop, n_mels;
  int framing;            /* ETD_STEMFEAT_* */
  float amin, top_db;     /* power_to_db: 1e-10, 80 */
} etd_stemfeat_cfg;
/* Tables from the host layer: window_host [n_fft] (periodic Hann) and the mel filterbank in CSR form as for etd_frontend_create: band m covers power-spectrum bins
 * [mel_start[m], + mel_len[m]) with weights mel_w[sum(mel_len[:m]) ...].  A band outside 0 .. n_fft / 2, a negative or non-finite weight, a non-finite window value
 * or a bad config is ETD_EINVAL with a message.  Needs no GPU: the tables go to the device with the first etd_stemfeat_run. */
int etd_stemfeat_create(const etd_stemfeat_cfg* cfg, const float* window_host, const int32_t* mel_start, const int32_t* mel_len, const float* mel_w_host,
                        etd_stemfeat** out);
void etd_stemfeat_destroy(etd_stemfeat*);
/* HOST ONLY: frames of a stem of N >= 1 samples (negative = ETD_EINVAL) */
long long etd_stemfeat_num_frames(const etd_stemfeat*, long long N);
/* HOST ONLY: bytes of device workspace a call with these songs makes the handle hold (per-workgroup and per-stem maxima, the song table); negative = ETD_EINVAL */
long long etd_stemfeat_workspace_bytes(const etd_stemfeat*, int n_songs, int instr, const int64_t* N_host);
/* wav_ptrs: HOST array of n_songs DEVICE pointers, song s = planar [instr][channels][N_host[s]] fp32 (the songs are not concatenated).  feat_dev: the songs'
 * [instr][T_s][n_mels] fp32 blocks back to back -- exactly etd_beat_forward's input.  Three launches whatever n_songs and instr are.  A (song, stem)'s features depend on
 * that stem's samples alone: bit-identical alone, in any batch and in any order.  Every output lies in [-top_db, 0]; a NaN or infinite sample leaves NaN in the
 * frames it reaches (the caller's range check finds it).  Synchronises `stream` once at the start (song table upload). */
int etd_stemfeat_run(etd_stemfeat*, const float* const* wav_ptrs, int n_songs, int instr, int channels, const int64_t* N_host, float* feat_dev, void* stream);

/* ------------------------------------------------------------------ DTW alignment (chroma + DLNCO features of a cover and its origin -> warping path, pitch shift)
 * What AudioAligner._compute_warping_path does behind the feature extraction (etude/data/aligner.py:106-133): quantized_chroma_to_CENS(.., 201, 50, ..),
 * compute_optimal_chroma_shift, shift_chroma_vectors, sync_via_mrmsdtw(step_weights = [1.5, 1.5, 2.0], alpha = 0.5), make_path_strictly_monotonic and the
 * pitch_shift rule.  Where synctoolbox approximates the optimum inside multi-resolution constraint regions, this is the exact full-resolution DTW.  DESIGN.md 4e is
 * the contract (parity with synctoolbox itself is unpinned).  Sequence 1 is the cover, sequence 2 the origin. */
typedef struct etd_dtw etd_dtw;
typedef struct {
  int struct_bytes;          /* sizeof(etd_dtw_cfg) of the caller: a mismatch is ETD_EINVAL */
  int cens_window;           /* 201: points of the Hann window (symmetric, scaled to sum 1) that smooths every pitch row; odd, 1 .. 4095 */
  int cens_decimation;       /* 50: every cens_decimation-th smoothed frame is a CENS frame, starting at 0 */
  int reserved;              /* 0 */
  double step_weights[3];    /* (1.5, 1.5, 2.0): weights of the steps (1,0), (0,1), (1,1) of the final DTW (aligner.py:43) */
  double shift_weights[3];   /* (1, 1, 1): ... of the 12 CENS DTWs of the transposition search (compute_optimal_chroma_shift) */
  float alpha;               /* 0.5: C = alpha (2 - <c1, c2>) + (1 - alpha) ||o1 - o2|| */
  float norm_threshold;      /* 1e-3: a chroma / CENS column with a smaller L2 norm becomes the constant unit vector */
} etd_dtw_cfg;
/* AudioAligner.__init__ (aligner.py:31-45).  Needs no GPU: the window goes to the device with the first call.  A bad config is ETD_EINVAL. */
int etd_dtw_create(const etd_dtw_cfg* cfg, etd_dtw** out);
void etd_dtw_destroy(etd_dtw*);
/* HOST ONLY: the constants of this build: rows of a row block, cells per backpointer word, frames per side and pairs per call it accepts (any may be NULL) */
int etd_dtw_limits(int* row_block, int* cells_per_word, long long* max_frames, int* max_pairs);
/* HOST ONLY: bytes of device workspace a call with these pairs needs (formula in DESIGN.md 4e; dominated by the 2-bit backpointers, N1 * ceil(N2 / 16) * 4 bytes
 * per pair); *result_ints (may be NULL) = int32 elements of its result buffer, result_offsets [n_pairs] (may be NULL) = where each pair's block starts in it.
 * Negative = ETD_EINVAL: n_pairs outside 1 .. 4096, a side of no frames, or one of more than 65 536 frames (the message names the count). */
long long etd_dtw_workspace_bytes(const etd_dtw*, int n_pairs, const int64_t* N1_host, const int64_t* N2_host, long long* result_ints, int64_t* result_offsets);
/* The body of _compute_warping_path for n_pairs pairs in five launches.  feat_ptrs: HOST array [n_pairs][4] of DEVICE pointers: cover quantized chroma, cover DLNCO
 * (both fp32 [12][N1]), origin quantized chroma, origin DLNCO (fp32 [12][N2]); finite, chroma >= 0 (the caller checks).  workspace_dev: 256-byte aligned device
 * memory of >= etd_dtw_workspace_bytes; result_dev: 8-byte aligned device int32 [>= *result_ints].  Pair p's block, at result_offsets[p], with cap = min(N1, N2) + 1:
 *   [0] L = path length  [1] opt = the chroma shift applied to the origin  [2] pitch_shift = (-opt) mod 12, minus 12 above 6  [3] points of the unfiltered path
 *   [4..5] D[-1,-1] of the final DTW (one double)  [6..7] 0     [8 .. 8 + L) wp[0] = cover frames     [8 + cap .. 8 + cap + L) wp[1] = origin frames, increasing.
 * result_host (may be NULL): the whole result copied there, the one copy to the host.  A pair's result depends on that pair alone: bit-identical alone, in any
 * batch and in any order.  Synchronous: returns when `stream` has drained. */
int etd_dtw_align(etd_dtw*, const float* const* feat_ptrs, int n_pairs, const int64_t* N1_host, const int64_t* N2_host, void* workspace_dev, long long workspace_bytes,
                  int32_t* result_dev, long long result_ints, int32_t* result_host, void* stream);

/* ------------------------------------------------------------------ alignment features (mono audio at 22 050 Hz -> quantised chroma + DLNCO, the input of etd_dtw_align)
 * The feature extraction in front of the DTW, modelled on synctoolbox's published pipeline (audio_to_pitch_features, pitch_to_chroma, quantize_chroma,
 * audio_to_pitch_onset_features, pitch_onset_features_to_DLNCO): rate tiers 22 050 / 4 410 / 882 Hz, 88 zero-phase elliptic band-passes (pitches 21 .. 108, an fp64
 * recurrence whose time axis is split exactly into chunks), pitch energy, chroma, onset novelty, peaks, DLNCO.  DESIGN.md 4f is the contract (parity with synctoolbox
 * itself is unpinned); the tuning offset comes from etd_tuning_run or the caller; WAV samples of another rate or layout come through etd_resample_run, decoding other
 * file formats stays the caller's. */
typedef struct etd_alignfeat etd_alignfeat;
typedef struct {
  int struct_bytes;          /* sizeof(etd_alignfeat_cfg) of the caller: a mismatch is ETD_EINVAL */
  int sample_rate;           /* 22050 */
  int hop;                   /* 441: samples per feature frame (50 Hz) */
  int fir_taps;              /* 481: taps of the decimation filter */
  int decimation;            /* 5: between two tiers */
  int chunk;                 /* samples per chunk of the filter's time axis: must equal etd_alignfeat_limits' (apow_host holds that power) */
  int n_banks;               /* filterbanks (one per tuning offset) in the tables below, 1 .. 64 */
  int reserved;              /* 0 */
} etd_alignfeat_cfg;
/* HOST ONLY: the constants of this build: samples per chunk, sections per band, samples per song, songs per call, filterbanks per handle (any may be NULL) */
int etd_alignfeat_limits(int* chunk, int* max_sections, long long* max_samples, int* max_songs, int* max_banks);
/* Tables from the host layer, all host memory: fir_host [481] fp32 (the decimation filter, sum 1); sos_host [n_banks][88][6][6] fp64, band b = pitch 21 + b, section
 * k = (b0, b1, b2, 1, a1, a2) (scipy's layout; sections >= n_sections[b] are ignored); n_sections [n_banks][88], 1 .. 6; apow_host [n_banks][88][12][12] fp64: the
 * `chunk`-th power of the cascade's one-step state matrix (state = z0, z1 of section 0, of section 1, ...; transposed direct form II), zero outside the used block.
 * More than 6 sections, a non-finite value, a0 != 1, a pole on or outside the unit circle or a bad config is ETD_EINVAL with a message.  Needs no GPU: the tables go to
 * the device with the first etd_alignfeat_run. */
int etd_alignfeat_create(const etd_alignfeat_cfg* cfg, const float* fir_host, const double* sos_host, const int32_t* n_sections, const double* apow_host,
                         etd_alignfeat** out);
void etd_alignfeat_destroy(etd_alignfeat*);
/* HOST ONLY: feature frames of a song of N >= 1 samples, ceil(N / 441) (negative = ETD_EINVAL) */
long long etd_alignfeat_num_frames(const etd_alignfeat*, long long N);
/* HOST ONLY: bytes of device workspace a call with these songs needs (formula in DESIGN.md 4f; about 12.5 bytes per band sample, 1.1 GB for three minutes);
 * negative = ETD_EINVAL: n_songs outside 1 .. 4096, N < 1 or N above the limit */
long long etd_alignfeat_workspace_bytes(const etd_alignfeat*, int n_songs, const int64_t* N_host);
/* wav_ptrs: HOST array of n_songs DEVICE pointers, song s = N_host[s] mono fp32 samples, finite (the caller checks); bank_host [n_songs]: the filterbank (tuning) of
 * each song.  chroma_dev / dlnco_dev: the songs' [12][T_s] fp32 blocks back to back.  workspace_dev: 256-byte aligned device memory of workspace_bytes >=
 * etd_alignfeat_workspace_bytes (too small is ETD_EINVAL); afterwards it holds every intermediate stage (etd_alignfeat_debug_layout).  A song's features depend on its
 * samples and its filterbank alone: bit-identical alone, in any batch and in any order.  Synchronises `stream` once at the start (song table upload). */
int etd_alignfeat_run(etd_alignfeat*, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, const int32_t* bank_host, float* chroma_dev, float* dlnco_dev,
                      void* workspace_dev, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------ tuning estimation (mono audio at 22 050 Hz -> cents off 440 Hz equal temperament, the tuning_offset
 * of etd_alignfeat's filterbanks).  estimate_tuning of AudioAligner._compute_alignment (etude/data/aligner.py:100-101), modelled on synctoolbox's routine with its
 * defaults: STFT (n_fft 16 384, hop 8 192, periodic Hann, centred, zero padding), log(1 + 100 |X|^2) summed over time in a fixed order, a not-a-knot cubic spline onto a
 * 1-cent axis from MIDI 24 to 108, minus its 101-point local average, rectified, and a comb of 84 teeth 100 cents apart shifted over theta = -50 .. 49.  DESIGN.md 4g
 * is the contract (parity with synctoolbox or libfmp is unpinned). */
typedef struct etd_tuning etd_tuning;
typedef struct {
  int struct_bytes;          /* sizeof(etd_tuning_cfg) of the caller: a mismatch is ETD_EINVAL */
  int sample_rate;           /* 22050 */
  int n_fft;                 /* 16384 */
  int hop;                   /* 8192 */
} etd_tuning_cfg;
/* HOST ONLY: the constants of this build: fewest and most samples per song, songs per call (any may be NULL) */
int etd_tuning_limits(long long* min_samples, long long* max_samples, int* max_songs);
/* Forms every table on the host in fp64 (window, twiddles, the spline's pivots, the log-frequency axis).  Needs no GPU: the tables go to the device with the first
 * etd_tuning_run.  A config other than the one above is ETD_EINVAL. */
int etd_tuning_create(const etd_tuning_cfg* cfg, etd_tuning** out);
void etd_tuning_destroy(etd_tuning*);
/* HOST ONLY: bytes of device workspace a call with these songs needs (formula in DESIGN.md 4g; 32 KB per 8 frames, 0.5 MB per 3-minute song); negative = ETD_EINVAL:
 * n_songs outside 1 .. 4096, N < 32 768 (two windows) or N above the limit */
long long etd_tuning_workspace_bytes(const etd_tuning*, int n_songs, const int64_t* N_host);
/* wav_ptrs: HOST array of n_songs DEVICE pointers, song s = N_host[s] mono fp32 samples, finite (the caller checks).  tuning_dev: DEVICE int32 [n_songs], cents in
 * -50 .. 49; sim_dev: DEVICE fp64 [n_songs][100], the comb similarity of theta = -50 .. 49 (tuning = -50 + its first maximum).  workspace_dev: 256-byte aligned device
 * memory of workspace_bytes >= etd_tuning_workspace_bytes; afterwards it holds the stages Y, Yi, R and sim of every song (etd_tuning_debug_layout).  Refused with
 * ETD_EINVAL and a message before anything is launched: N < 32 768, too many songs, a workspace that is too small, a NULL output.  Three launches whatever n_songs;
 * a song's numbers depend on its samples alone: bit-identical alone, in any batch and in any order.  Synchronises `stream` once at the start (song table upload). */
int etd_tuning_run(etd_tuning*, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, int32_t* tuning_dev, double* sim_dev, void* workspace_dev,
                   long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------ audio loading (raw WAV samples of any rate, width and channel count -> fp32 at an engine's rate
 * and layout).  librosa.load(path, sr=22050) of etude/data/aligner.py:71-72 and scripts/preprocess.py:135, torchaudio.load of scripts/run_separation.py:89, behind the
 * walk over the file's chunks (etude_amd.audio.read_wav_raw).  The filter is this project's own windowed sinc, modelled on resampy's kaiser_best / kaiser_fast:
 *   up / down = sr_out / sr_in in lowest terms, s = min(1, up / down), half = ceil(Z / s), K = 2 half,
 *   h(t) = s r sinc(s r t) I0(beta sqrt(1 - (s t / Z)^2)) / I0(beta) for |s t| < Z, else 0  (t in input samples; best: Z 64, fast: Z 16),
 *   y[n] = sum_{k < K} tab[p][k] x[i0 - half + 1 + k],  i0 = n down div up,  p = n down mod up,  tab[p][k] = h(k - half + 1 - p / up),  x = 0 outside [0, N),
 *   N' = ceil(N up / down); the sum is one fp32 fmaf chain with k ascending.  Mono is the fp32 sum of the channels in order times 1.f / C, taken before the filter.
 * DESIGN.md 4q is the contract (parity with soxr, resampy or librosa is unpinned).  Decoding anything but RIFF/WAVE stays the caller's. */
typedef struct etd_resample etd_resample;
enum {                       /* sample formats: little-endian, interleaved [N][C] as in a WAV data chunk, except the last */
  ETD_PCM_U8 = 0,            /* (v - 128) / 128 */
  ETD_PCM_S16 = 1,           /* float(v) 2^-15 */
  ETD_PCM_S24 = 2,           /* float(v) 2^-23; three bytes per sample, no alignment */
  ETD_PCM_S32 = 3,           /* float(v) 2^-31 */
  ETD_PCM_F32 = 4,
  ETD_PCM_F64 = 5,           /* (float)v */
  ETD_PCM_F32_PLANAR = 6     /* fp32 [C][N]: tensors already on the device */
};
enum { ETD_RESAMPLE_BEST = 0, ETD_RESAMPLE_FAST = 1 };
typedef struct {
  int struct_bytes;          /* sizeof(etd_resample_cfg) of the caller: a mismatch is ETD_EINVAL */
  int sr_in, sr_out;         /* Hz, 1 .. 2^30 */
  int quality;               /* ETD_RESAMPLE_BEST (Z = 64) or ETD_RESAMPLE_FAST (Z = 16) */
  int up, down;              /* sr_out / sr_in in lowest terms, as the caller's table was designed: anything else is ETD_EINVAL */
  int half;                  /* ceil(Z / s) of that table */
  int reserved;              /* 0 */
} etd_resample_cfg;
/* table_host: fp32 [up][2 half], the filter designed by the host layer in fp64 and rounded once (NULL when sr_in == sr_out: such a handle only decodes).  Needs no
 * GPU: the table goes to the device with the first etd_resample_run.  ETD_EINVAL with a sentence: a cfg that does not match the rates, up x 2 half above 2^22
 * entries (e.g. 44 100 -> 22 051 Hz), a non-finite table. */
int etd_resample_create(const etd_resample_cfg* cfg, const float* table_host, etd_resample** out);
void etd_resample_destroy(etd_resample*);
/* HOST ONLY: N' = ceil(N up / down) in integers; negative = ETD_EINVAL (N < 0 or above 2^32) */
long long etd_resample_out_len(const etd_resample*, long long N);
/* HOST ONLY: bytes of device workspace a call with these songs needs (the song table and one 16-byte record per 256 outputs of every written channel); negative =
 * ETD_EINVAL: n_songs outside 1 .. 4096, channels outside 1 .. 8, frames outside 1 .. 2^32 */
long long etd_resample_workspace_bytes(const etd_resample*, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* mono_host);
/* src_ptrs: HOST array of n_songs DEVICE pointers to the raw samples of song s: frames_host[s] frames of channels_host[s] channels in format_host[s] (ETD_PCM_*),
 * bytes_host[s] bytes in all, aligned to the sample width (S24 and U8: any address).  out_ptrs: HOST array of DEVICE pointers, song s = fp32 [C][N'], or [N'] where
 * mono_host[s] != 0.  workspace_dev: 256-byte aligned device memory of workspace_bytes >= etd_resample_workspace_bytes.  Refused with ETD_EINVAL and a sentence before
 * anything is launched: channels outside 1 .. 8, a byte count other than frames x channels x width, an unknown format, a NULL or misaligned pointer, a workspace that
 * is too small, and a rate ratio whose staged input span (about 256 down / up + 2 half floats) outgrows the LDS the device reports.  One launch whatever n_songs, no
 * atomics: a song's samples depend on its own bytes and the table alone, bit-identical alone, in any batch and in any order.  Synchronises `stream` once at the start
 * (table upload). */
int etd_resample_run(etd_resample*, const void* const* src_ptrs, int n_songs, const int64_t* frames_host, const int32_t* channels_host, const int32_t* format_host,
                     const int32_t* mono_host, const int64_t* bytes_host, float* const* out_ptrs, void* workspace_dev, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------ rhythm metrics (note onsets -> Rhythmic Grid Consistency and IOI Pattern Entropy).
 * RGCCalculator.calculate and IPECalculator.calculate (etude/evaluation/metrics/rgc.py, ipe.py) behind get_onsets_from_file, with the KMeans of scikit-learn the second
 * one fits (n_clusters = min(8, distinct log-IOIs), random_state 42, one k-means++ start, Lloyd, max_iter 300, tol 1e-4) restated in fp64 in a fixed order.  DESIGN.md
 * 4h is the contract. */
typedef struct etd_rhythm etd_rhythm;
typedef struct {
  int struct_bytes;          /* sizeof(etd_rhythm_cfg) of the caller: a mismatch is ETD_EINVAL */
  int top_k;                 /* 8: the most common rounded IOIs the grid is inferred from, 1 .. 64 */
  int precision_digits;      /* 4: decimals the IOIs are rounded to before they are counted, 0 .. 9 */
  int n_gram;                /* 8: symbols per n-gram, 1 .. 16 */
  int n_clusters;            /* 8: most clusters (symbols), 1 .. 8 */
  int n_random;              /* 29: doubles in random_host */
  double min_ioi, max_ioi;   /* 0.0625, 4.0: the IOIs are clipped to this range before the logarithm */
  const double* random_host; /* the first 29 doubles of numpy.random.RandomState(42).random_sample(): the only random numbers KMeans(random_state=42) draws, each in
                              * [0, 1); copied by etd_rhythm_create.  No generator runs on the device. */
} etd_rhythm_cfg;
/* HOST ONLY: the constants of this build: onsets per cover (8 192), covers per call, the largest top_k and n_gram (any may be NULL) */
int etd_rhythm_limits(int* max_onsets, int* max_covers, int* max_top_k, int* max_n_gram);
/* Needs no GPU.  A value outside the ranges above is ETD_EINVAL. */
int etd_rhythm_create(const etd_rhythm_cfg* cfg, etd_rhythm** out);
void etd_rhythm_destroy(etd_rhythm*);
/* A ragged batch: cover b is onsets_dev[offsets[b] .. offsets[b + 1]) (DEVICE fp64, seconds, ascending and unique -- np.unique of the note onsets; fewer than two is
 * a valid cover with an error status); offsets_dev: DEVICE int64 [n_covers + 1], offsets_host: the same numbers on the HOST (offsets[0] = 0).  out_dev: DEVICE fp64
 * [n_covers][3] = rgc_score, inferred_tau, ipe_score (NaN where the metric has none); status_dev: DEVICE int32 [n_covers]:
 *   bits 0 .. 3   RGC: 0 ok, 1 "Not enough onsets for IOI calculation.", 2 "Not enough IOIs to analyze.", 3 "Not enough unique IOIs to determine a grid.",
 *                 4 "Could not infer a valid rhythmic grid period (tau).", 5 the onsets are not ascending, unique, finite and below 2^50 / 10^precision_digits apart
 *   bits 4 .. 7   IPE: 0 ok, 1 as above, 3 "Could not quantize IOI sequence into symbols." (fewer than two distinct clipped log-IOIs), 5 as above
 *   bit 8         relocated: Lloyd's iteration met an empty cluster; the samples that move are picked by distance descending, then lowest index, where scikit-learn's
 *                 argpartition leaves the order of equally far samples open
 *   bits 12 .. 15 the clusters k, bits 16 .. 24 Lloyd's iterations
 * Refused with ETD_EINVAL and a message before anything is launched: a cover above 8 192 onsets, n_covers outside 1 .. 2^20, decreasing offsets, a NULL output.  ONE
 * launch whatever n_covers, one workgroup per cover, the working set in LDS.  A cover's numbers depend on its onsets alone: bit-identical alone, in any batch and
 * from run to run.  Asynchronous on `stream`. */
/* HOST ONLY: what etd_rhythm_run refuses about the shape of a call, with its message, before anything touches the device: n_covers outside 1 .. 2^20,
 * offsets_host[0] != 0, decreasing offsets, a cover above 8 192 onsets */
int etd_rhythm_check(const etd_rhythm*, const int64_t* offsets_host, int n_covers);
int etd_rhythm_run(etd_rhythm*, const double* onsets_dev, const int64_t* offsets_dev, const int64_t* offsets_host, int n_covers, double* out_dev, int32_t* status_dev,
                   void* stream);

/* ------------------------------------------------------------------ bar attributes (token ids of (condition bar, target bar) pairs -> the four attributes the decoder is
 * conditioned on).  EtudeDataset._extract_bar_features, _compute_musical_attributes and _get_attribute_bin_id (etude/data/dataset.py:204-270, 335-339) for a ragged batch
 * of pairs: integer counting plus one fp64 mean per pair, the mean's terms in ascending Pos value and numpy's order.  DESIGN.md 4i is the contract. */
typedef struct etd_attr etd_attr;
typedef struct {
  int struct_bytes;          /* sizeof(etd_attr_cfg) of the caller: a mismatch is ETD_EINVAL */
  int type_pos;              /* 1, 2, 3: the codes the event table uses for Pos, Note and Duration events (TinyREMITokenizer.event_table); every other code is an */
  int type_note;             /* event the attributes ignore */
  int type_duration;
} etd_attr_cfg;
/* HOST ONLY: the constants of this build: tokens per bar (4 096), pairs and bars per call (2^20), the widest range of Pos values a vocabulary may hold (4 096), edges
 * per attribute (2); any may be NULL */
int etd_attr_limits(int* max_bar_tokens, int* max_pairs, int* max_pos_range, int* max_edges);
/* event_table_host: int32 [vocab_size][2] = (type, value) per token id.  The per-pair table in LDS is sized here from the range of the Pos values; a range above 4 096,
 * a Duration value that could overflow the int32 total, or type codes that coincide are ETD_EINVAL.  With a GPU the table is copied to the current device here; without
 * one the handle still serves etd_attr_check, and etd_attr_run refuses it. */
int etd_attr_create(const etd_attr_cfg* cfg, const int32_t* event_table_host, int vocab_size, etd_attr** out);
void etd_attr_destroy(etd_attr*);
/* HOST ONLY: what etd_attr_run refuses about one side's bars, with its message, before anything touches the device: n_bars outside 1 .. 2^20, offsets_host[0] != 0,
 * decreasing offsets, a bar above 4 096 tokens */
int etd_attr_check(const etd_attr*, const int64_t* offsets_host, int n_bars);
/* Source bar b is src_ids_dev[src_offsets[b] .. src_offsets[b + 1]) (DEVICE int32 ids; offsets: DEVICE int64 [n_src_bars + 1] and the same numbers on the HOST), the
 * target side likewise, in the same id buffer or another.  Pair i takes source bar src_index_dev[i] and target bar tgt_index_dev[i] (DEVICE int32 [n_pairs]); a NULL
 * index is the identity and needs n_bars == n_pairs -- the index lets the condition bars of a song be uploaded once for all its attribute tuples.
 * features_dev: DEVICE int32 [n_pairs][6] = note_count, pos_event_count, total_duration_in_16ths of the source, then of the target.  attributes_dev: DEVICE fp64
 * [n_pairs][4] = relative_polyphony, relative_rhythmic_intensity, relative_note_sustain, pitch_overlap_ratio (_MODEL_ATTRIBUTES order).  edges_host: HOST fp64 [4][2]
 * with n_edges_host int32 [4] (0 .. 2 ascending finite edges per attribute, np.unique's output; no edges = bin 1) and bins_dev: DEVICE int32 [n_pairs][4] =
 * np.digitize(value, edges); all three NULL = raw values only.  status_dev: DEVICE int32 [n_pairs]:
 *   bit 0         an id outside [0, vocab_size) in either bar: it counts as an event the attributes ignore, the table is not read
 *   bit 1         a bar index outside its side's bars: that bar counts as empty
 *   bits 8 .. 20  the positions that hold a note in either bar (the terms of the pitch-overlap mean)
 * Refused with ETD_EINVAL and a message before anything is launched: what etd_attr_check refuses, n_pairs outside 1 .. 2^20, edges that are not ascending and finite,
 * a NULL output, a handle created without a GPU.  ONE launch whatever n_pairs, one wavefront per pair, nothing allocated, no synchronisation.  A pair's numbers depend on
 * its two bars alone: bit-identical alone, in any batch and from run to run.  Asynchronous on `stream`. */
int etd_attr_run(etd_attr*, const int32_t* src_ids_dev, const int64_t* src_offsets_dev, const int64_t* src_offsets_host, int n_src_bars, const int32_t* src_index_dev,
                 const int32_t* tgt_ids_dev, const int64_t* tgt_offsets_dev, const int64_t* tgt_offsets_host, int n_tgt_bars, const int32_t* tgt_index_dev, int n_pairs,
                 const double* edges_host, const int32_t* n_edges_host, int32_t* features_dev, double* attributes_dev, int32_t* bins_dev, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------ decoder training (train.py: forward with saved activations, backward of the reference's
 * cross-entropy loss for every parameter, gradient accumulation, clip_grad_norm_ and torch.optim.AdamW), all in fp32.  DESIGN.md 4j is the contract.
 * The model is etd_decoder's in its exact-parity arithmetic (cfg.precision, max_streams, max_ctx and max_prefill_rows are not read); dropout is 0 in the reference's
 * configuration, so train mode computes what eval mode computes.  No floating-point atomics anywhere: the same call on the same inputs gives the same bits. */
typedef struct etd_dtrain etd_dtrain;
/* HOST ONLY: bytes of saved activations and scratch a handle created with these arguments holds; negative = ETD_EINVAL (the limits of etd_dtrain_create) */
long long etd_dtrain_workspace_bytes(const etd_dec_cfg* cfg, int max_rows);
/* The config struct and state-dict names of etd_decoder_create.  Keeps plain fp32 master weights, gradients and AdamW's exp_avg / exp_avg_sq (zero) on the device.
 * The padding_idx rows of the six embedding tables (pad_token_id, pad_class_id, attribute_pad_id) get a zero gradient, as nn.Embedding gives them.
 * transformer.embed_in.weight is part of the state dict but never read: it gets no gradient and is never changed.  max_rows bounds the packed rows of one
 * etd_dtrain_forward_backward call and sizes the workspace.  Limits: head_dim 64, 16 rotary dims, hidden % 256 == 0, intermediate % 128 == 0, any vocabulary, any
 * number of layers; anything else, a missing weight or a wrong element count is ETD_EINVAL with a message before the device is touched. */
int etd_dtrain_create(const etd_dec_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n,
                      int pad_token_id, int pad_class_id, int attribute_pad_id, int max_rows, etd_dtrain** out);
void etd_dtrain_destroy(etd_dtrain*);
/* what = 0: bytes of saved activations and scratch; 1: bytes of weights + gradients + the two moments */
long long etd_dtrain_bytes(const etd_dtrain*, int what);
/* n sequences packed as for etd_decoder_score (T[n] rows each; ids / cls / labels int32 host [M = sum(T)], attrs4 int32 host [4][M] in C-ABI attribute order; a row's
 * label is the token it should predict, NOT shifted, or -100).  *loss = F.cross_entropy's mean over the labelled rows, *n_scored their count, and
 * loss_scale * d loss / d p is ADDED to every parameter's gradient (gradient accumulation passes 1 / grad_accum_steps).  A call with no labelled row returns
 * *loss = nan and *n_scored = 0 and launches nothing: the accumulated gradients keep every bit (train.py:169 skips such a batch).  Out-of-range ids / classes / bins /
 * labels, a sequence longer than max_position_embeddings or more rows than max_rows are ETD_EINVAL before anything runs.  Synchronous. */
int etd_dtrain_forward_backward(etd_dtrain*, int n, const int32_t* T, const int32_t* ids, const int32_t* cls, const int32_t* attrs4, const int32_t* labels,
                                float loss_scale, float* loss, int32_t* n_scored, void* stream);
int etd_dtrain_zero_grad(etd_dtrain*, void* stream);
/* L2 norm over all gradients: fp64 partial sums of the fp32 squares in a fixed order, one square root.  Synchronous. */
int etd_dtrain_grad_norm(etd_dtrain*, double* norm, void* stream);
/* torch.nn.utils.clip_grad_norm_ (g *= min(1, max_norm / (norm + 1e-6)); max_norm <= 0 = no clipping) followed by one torch.optim.AdamW step of the single-tensor path
 * on every parameter (decoupled decay p *= 1 - lr * weight_decay on all of them: the reference passes model.parameters() as one group; bias corrections from the
 * handle's step count, advanced here, in double on the host).  *norm (may be NULL) = the norm before clipping.  The gradients are left clipped, not zeroed. */
int etd_dtrain_clip_and_step(etd_dtrain*, double max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, double* norm, void* stream);
/* the optimizer's step count (0 after create); set it, with etd_dtrain_write_moment, to resume */
int etd_dtrain_set_step(etd_dtrain*, long long step);
long long etd_dtrain_get_step(const etd_dtrain*);
/* One tensor by its state-dict name, fp32 to / from the host; numel must be the tensor's.  second = 0: exp_avg, 1: exp_avg_sq.  Synchronous. */
int etd_dtrain_read_param(etd_dtrain*, const char* name, float* out_host, long long numel, void* stream);
int etd_dtrain_read_grad(etd_dtrain*, const char* name, float* out_host, long long numel, void* stream);
int etd_dtrain_read_moment(etd_dtrain*, const char* name, int second, float* out_host, long long numel, void* stream);
int etd_dtrain_write_moment(etd_dtrain*, const char* name, int second, const float* in_host, long long numel, void* stream);

/* ------------------------------------------------------------------ Beat-Transformer training (the model of etd_beat with saved activations, this project's beat /
 * tempo loss, the backward pass for every parameter, gradient accumulation, clip_grad_norm_ and torch.optim.AdamW), all in fp32.  DESIGN.md 4s is the contract.
 * The trained arithmetic is the inference arithmetic: there is no dropout.  Every dense product is the fp32 GEMM family of the decoder trainer; no floating-point
 * atomics anywhere: the same call on the same inputs gives the same bits.
 *   loss = sum_c (1 / n_c) sum_{scored (f, c)} (1 + (pos_weight_c - 1) y) bce_with_logits(z, y)  +  tempo_weight * mean_{songs with a target} -sum_k p_k log_softmax(t)_k */
typedef struct etd_btrain etd_btrain;
typedef struct {
  int struct_bytes;       /* sizeof(etd_btrain_cfg) of the caller: a mismatch is ETD_EINVAL */
  int attn_len, instr, ntoken, dmodel, nhead, d_hid, nlayers, norm_first, n_mels, tempo_out;      /* the limits of etd_beat_create; tempo_out = 300 */
  int max_rows;           /* rows (instr x frames) of one etd_btrain_loss_backward call: sizes the workspace, 1 .. 2^17 */
  int max_seqs;           /* songs of one call, 1 .. 65535 */
  float tempo_weight;     /* >= 0 */
  float dropout;          /* must be 0: dropout is not implemented */
} etd_btrain_cfg;
/* HOST ONLY: bytes of saved activations and scratch a handle created with this config holds; negative = ETD_EINVAL (the limits of etd_btrain_create) */
long long etd_btrain_workspace_bytes(const etd_btrain_cfg* cfg);
/* The state-dict names of etd_beat_create.  Keeps fp32 master weights, gradients and AdamW's exp_avg / exp_avg_sq (zero) on the device.  pos_weight [ntoken] host
 * (NULL = ones), each finite and > 0.  An unsupported architecture, dropout != 0, a missing weight or a wrong element count is ETD_EINVAL before the device is touched. */
int etd_btrain_create(const etd_btrain_cfg* cfg, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n, const float* pos_weight,
                      etd_btrain** out);
void etd_btrain_destroy(etd_btrain*);
/* what = 0: bytes of saved activations and scratch; 1: bytes of weights + gradients + the two moments */
long long etd_btrain_bytes(const etd_btrain*, int what);
/* HOST ONLY: the argument checks of etd_btrain_loss_backward (more songs than max_seqs or rows than max_rows, T < 1, a beat target that is neither in [0, 1] nor -1,
 * a tempo row that is negative, not finite or does not sum to 1 within 1e-5).  n_scored [ntoken] and n_tempo may be NULL. */
int etd_btrain_check_batch(const etd_btrain_cfg* cfg, int n_seq, const int64_t* T_host, const float* beat_targets, const float* tempo_targets,
                           const int32_t* has_tempo, int32_t* n_scored, int32_t* n_tempo);
/* feat_dev: the songs' [instr][T_s][128] fp32 blocks back to back on the device (PRECONDITION as etd_beat_forward: finite, |x| <= 80; the Python mirror checks it).
 * beat_targets: host [sum T_s][ntoken] in [0, 1], -1 = that (frame, class) cell is not scored.  tempo_targets: host [n_seq][300] distributions, read where
 * has_tempo[s] != 0 (both may be NULL: no tempo term).  *loss = loss_scale * loss and loss_scale * d loss / d p is ADDED to every parameter's gradient.
 * *n_scored = scored beat cells.  A call with no scored cell and no tempo target returns *loss = nan and *skipped = 1 and launches nothing.  Synchronous. */
int etd_btrain_loss_backward(etd_btrain*, const float* feat_dev, int n_seq, const int64_t* T_host, const float* beat_targets, const float* tempo_targets,
                             const int32_t* has_tempo, float loss_scale, float* loss, int32_t* n_scored, int32_t* skipped, void* stream);
int etd_btrain_zero_grad(etd_btrain*, void* stream);
int etd_btrain_grad_norm(etd_btrain*, double* norm, void* stream);
/* clip_grad_norm_ then one AdamW step, exactly as etd_dtrain_clip_and_step (the same scalars and update kernel).  *norm (may be NULL) = the norm before clipping. */
int etd_btrain_step(etd_btrain*, double max_norm, double lr, double beta1, double beta2, double eps, double weight_decay, double* norm, void* stream);
int etd_btrain_set_step(etd_btrain*, long long step);
long long etd_btrain_get_step(const etd_btrain*);
/* One tensor by its state-dict name, fp32 to / from the host, in the state dict's own layout.  which: 0 parameter, 1 gradient, 2 exp_avg, 3 exp_avg_sq.  Synchronous. */
int etd_btrain_read(etd_btrain*, const char* name, int which, float* out_host, long long numel, void* stream);
int etd_btrain_write(etd_btrain*, const char* name, int which, const float* in_host, long long numel, void* stream);

/* ------------------------------------------------------------------ note renderer (note lists -> mono fp32 waveforms of this project's own piano voice, the audio
 * the alignment features of a generated cover are computed from).  The voice is a contract of this project (restated in fp64 in tests/render_np.py):
 * parity with pretty_midi.synthesize or a SoundFont player is not claimed.  No atomics anywhere: a cover's samples depend on its notes, tuning and rate alone. */
typedef struct etd_render etd_render;
typedef struct {
  int struct_bytes;          /* sizeof(etd_render_cfg) of the caller: a mismatch is ETD_EINVAL */
  int sample_rate;           /* 22050; 8000 .. 48000 */
  int partials;              /* 8: partials k = 1 .. K of a note, 1 .. 16 */
  int flags;                 /* 3: bit 0 = the decay exp(-tau / T_k), bit 1 = the release (off: a note ends at its offset) */
  double inharmonicity;      /* 3.5e-4: B at pitch 60; f_k = k f0 sqrt(1 + B k^2) */
  double inharmonicity_step; /* 10: B doubles every so many semitones */
  double partial_rolloff;    /* 1.5: A_k = (velocity / 127)^velocity_power k^-partial_rolloff */
  double velocity_power;     /* 2 */
  double attack;             /* 0.004 s: min(tau / attack, 1) */
  double decay_base;         /* 3.0 s: T at pitch 21 */
  double decay_halving;      /* 24: T halves every so many semitones */
  double decay_partial;      /* 0.25: T_k = T / (1 + decay_partial (k - 1)) */
  double release_tau;        /* 0.06 s: behind the offset, exp(-u / release_tau) (1 - u / release_len) */
  double release_len;        /* 0.48 s: a note is exactly 0 from offset + release_len on */
  double gain;               /* 0.1 */
  double nyquist_fraction;   /* 0.45: a partial at or above this fraction of the sample rate does not exist */
} etd_render_cfg;
/* HOST ONLY: the constants of this build: notes per cover (65 536), samples per cover (etd_alignfeat_limits' max_samples), partials (16), covers per call (4 096),
 * samples a workgroup owns (1 024); any may be NULL */
int etd_render_limits(int* max_notes, long long* max_samples, int* max_partials, int* max_covers, int* block);
/* Needs no GPU.  A value outside the ranges above is ETD_EINVAL. */
int etd_render_create(const etd_render_cfg* cfg, etd_render** out);
void etd_render_destroy(etd_render*);
/* HOST ONLY: bytes of device workspace a call with these covers needs (32 per cover, 8 per 1 024 samples, 472 per note, each part rounded up to 256); negative =
 * ETD_EINVAL: n_covers outside 1 .. 4 096, a cover above the note or sample limit, decreasing offsets */
long long etd_render_bytes(const etd_render*, int n_covers, const int64_t* note_offsets_host, const int64_t* num_samples_host);
/* A ragged batch: cover b is notes_host[note_offsets_host[b] .. note_offsets_host[b + 1]) (HOST; sorted by onset, ties in the caller's order; 0 <= onset < offset,
 * pitch 21 .. 108, velocity 1 .. 127), tuned by cents_host[b] (|c| <= 50; NULL = 0), and becomes the num_samples_host[b] fp32 samples at
 * out_dev + sample_offsets_host[b] (DEVICE; offsets ascending, multiples of 4, covers not overlapping).  Every sample of every cover is written exactly once, zeros
 * included; what lies between two covers is not touched.  Anything else is refused with ETD_EINVAL and a message naming the cover and the note before the device is
 * touched.  Two launches (three above 2^23 blocks) and one upload; synchronises `stream` once (the upload).  A cover's samples are bit-identical alone, in any batch,
 * in any order and from run to run. */
int etd_render_run(etd_render*, const etd_note* notes_host, const int64_t* note_offsets_host, const double* cents_host, int n_covers, const int64_t* num_samples_host,
                   const int64_t* sample_offsets_host, float* out_dev, void* workspace_dev, long long workspace_bytes, void* stream);
/* peaks_dev[b] = max |x| over the num_samples_dev[b] samples at samples_dev + sample_offsets_dev[b] (both DEVICE int64 [n_covers]; 0 for an empty cover).  ONE launch,
 * one workgroup per cover.  Asynchronous on `stream`. */
int etd_render_peaks(etd_render*, const float* samples_dev, const int64_t* sample_offsets_dev, const int64_t* num_samples_dev, int n_covers, float* peaks_dev,
                     void* stream);

/* ------------------------------------------------------------------ source separator (a song's audio -> its stems; csrc/separator.hip)
 * A U-Net mask separator modelled on Spleeter 2.x's 5stems model: STFT, one six-level U-Net per instrument on the magnitudes below bin F, a softmax over the
 * instruments, ratio masks, inverse STFT.  DESIGN.md 4m is the contract (tests/separator_np.py restates it; parity with Spleeter's TensorFlow graph and its
 * checkpoints is unpinned).  fp32 operands and accumulation, no floating-point atomics: every sum runs in an order the shapes fix. */
typedef struct etd_sep etd_sep;
#define ETD_SEP_LEVELS 6
#define ETD_SEP_MAX_INSTR 16
#define ETD_SEP_MAX_CHANNELS 8
typedef struct {
  int struct_bytes;            /* sizeof(etd_sep_cfg) of the caller: a mismatch is ETD_EINVAL */
  int n_instr;                 /* 1 .. ETD_SEP_MAX_INSTR */
  int n_channels;              /* 1 .. ETD_SEP_MAX_CHANNELS */
  int n_fft;                   /* a power of two in 1024 .. 4096 */
  int hop;                     /* n_fft / 4 */
  int T, F;                    /* frames per segment and bins the U-Net reads: multiples of 64, F <= n_fft / 2 */
  int filters[ETD_SEP_LEVELS]; /* each >= 1 */
  int separation_exponent;     /* 1 .. 8 (Spleeter: 2) */
  float mask_eps, bn_eps;      /* positive, finite (1e-10, 1e-3) */
  long long workspace_bytes;   /* budget of the handle's device workspace: songs are grouped and units sub-batched under it; one song with one unit is the floor; 0 = 4 GiB */
} etd_sep_cfg;
/* instr_names [n_instr] and the checkpoint as a weight table (HOST fp32): per instrument "{instr}.conv{l}.weight" [5][5][Cin][Cout], ".bias" [Cout] (l = 1 .. 6),
 * "{instr}.deconv{j}.weight" [5][5][Cout][Cin], ".bias" (j = 1 .. 6), "{instr}.bn{n}.gamma / .beta / .mean / .var" (n = 1 .. 12: the encoder's six, then the
 * decoder's), "{instr}.head.weight" [4][4][1][n_channels], ".bias".  A missing key or a wrong size is ETD_EINVAL with the key in the message.  Needs no GPU: the
 * weights go to the device with the first run. */
int etd_sep_create(const etd_sep_cfg* cfg, const char* const* instr_names, const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n,
                   etd_sep** out);
void etd_sep_destroy(etd_sep*);
/* HOST ONLY: STFT frames of a song of N >= 1 samples, 1 + (N + n_fft) / hop (negative = ETD_EINVAL) */
long long etd_sep_num_frames(const etd_sep*, long long N);
/* HOST ONLY: bytes of activations one (segment, instrument) unit of the U-Net holds */
long long etd_sep_unit_bytes(const etd_sep*);
/* HOST ONLY: bytes of device memory a call with these songs makes the handle hold: at most the budget, unless one song (spectra, magnitudes, mask logits, masked
 * spectra) with one unit's activations needs more */
long long etd_sep_workspace_bytes(const etd_sep*, int n_songs, const int64_t* N_host);
/* wav_ptrs / out_ptrs: HOST arrays of n_songs DEVICE pointers; song s is planar [n_channels][N_host[s]] fp32 and becomes [n_instr][n_channels][N_host[s]] fp32 --
 * etd_stemfeat_run's input.  A song's stems are bit-identical alone, in any batch, under any workspace budget and from run to run.  Synchronises `stream` when the
 * workspace grows. */
int etd_sep_run(etd_sep*, const float* const* wav_ptrs, int n_songs, const int64_t* N_host, float* const* out_ptrs, void* stream);
/* FLOPs of the U-Nets of one segment, all instruments (2 per multiply-add that is not a structural zero) */
double etd_sep_segment_flops(const etd_sep*);
/* audio -> the U-Net's input: wav [n_channels][N] DEVICE fp32 -> mag [ceil(Tf / T)][T][F][n_channels] DEVICE fp32, |X| below bin F of the song's Tf =
 * etd_sep_num_frames(N) frames, zeros past the last (step 2 of etd_sep_run, by the same kernel).  Synchronises `stream` when the workspace grows. */
int etd_sep_magnitudes(etd_sep*, const float* wav_dev, long long N, float* mag_dev, void* stream);
/* HOST ONLY: multichannel Wiener filtering of the stems (csrc/separator_mwf.hip; DESIGN.md 4r is the contract, tests/separator_mwf_np.py restates it; modelled on
 * norbert.wiener, parity unpinned).  `iterations` in 0 .. 8 refinements of every later etd_sep_run's masked spectra between the mask pass and the inverse STFT, the
 * ratio mask being the initial estimate: per iteration a spatial covariance per (source, bin) over all frames of the song, then the multichannel Wiener gain per
 * (frame, bin), in fp64 on the fp32 spectra.  0 (a new handle's value) = none: etd_sep_run is then what it was.  iterations > 0 needs n_channels 1 or 2
 * (ETD_EINVAL otherwise).  The scratch comes from the workspace's work region and may raise its floor: etd_sep_workspace_bytes tells. */
int etd_sep_set_mwf(etd_sep*, int iterations);
/* HOST ONLY: the value set (negative = ETD_EINVAL) */
int etd_sep_get_mwf(const etd_sep*);

/* ---- training of the source separator (csrc/separator_train.hip; DESIGN.md 4n is the contract, tests/separator_train_np.py restates it) ----------------------
 * The U-Nets of etd_sep in training mode (every norm on the batch's statistics), the L1 loss on the softmax estimates, every gradient and torch.optim.Adam, in fp32
 * with no atomics: the same call gives the same bits.  One call is one batch of B units: mix [B][T][F][n_channels], target [n_instr][B][T][F][n_channels], DEVICE
 * fp32, finite and non-negative (the caller checks).  cfg.workspace_bytes is the budget of the per-call workspace (0 = 16 GiB): a batch that does not fit is
 * ETD_EINVAL with the bytes needed, before anything is launched; there is no sub-batching.  separation_exponent and mask_eps take no part. */
typedef struct etd_septrain etd_septrain;
/* etd_sep_create's arguments and refusals (no GPU is touched); max_units bounds B (max_units * n_instr <= 16384) */
int etd_septrain_create(const etd_sep_cfg* cfg, int max_units, const char* const* instr_names, const char* const* names, const float* const* host_ptrs,
                        const int64_t* numels, int n, etd_septrain** out);
void etd_septrain_destroy(etd_septrain*);
/* HOST ONLY: bytes of workspace a call with B units holds */
long long etd_septrain_workspace_bytes(const etd_septrain*, int B);
/* HOST ONLY: convolution FLOPs of one forward + backward of B units (forward, input gradients, weight gradients; structural zeros not counted) */
double etd_septrain_step_flops(const etd_septrain*, int B);
/* Forward in training mode, *loss = (1 / (I B T F C)) sum |softmax_i(logits) mix - target_i| (an fp64 sum of per-workgroup fp32 partials in a fixed order), and, with
 * backward != 0, loss_scale x its gradient ADDED to the handle's gradients.  frozen_stats != 0: the norms use the running statistics, which then do not move;
 * otherwise they move once, r <- 0.99 r + 0.01 batch (biased variance).  Synchronous. */
int etd_septrain_forward_backward(etd_septrain*, const float* mix_dev, const float* target_dev, int B, double loss_scale, int frozen_stats, int backward,
                                  double* loss, void* stream);
int etd_septrain_zero_grad(etd_septrain*, void* stream);
/* L2 norm over all gradients (fp64 partial sums in a fixed order).  Synchronous. */
int etd_septrain_grad_norm(etd_septrain*, double* norm, void* stream);
/* clip_grad_norm_ when max_norm > 0, then one torch.optim.Adam step of the single-tensor path (no weight decay; bias corrections and 1 - beta in double on the
 * host).  *norm (may be NULL) = the norm before clipping.  The gradients are left as they are (clipped), not zeroed. */
int etd_septrain_step(etd_septrain*, double max_norm, double lr, double beta1, double beta2, double eps, double* norm, void* stream);
int etd_septrain_set_step(etd_septrain*, long long step);
long long etd_septrain_get_step(const etd_septrain*);
/* One tensor by its state key, fp32 to / from the host.  which = 0: the state (running statistics included), 1: gradient, 2: exp_avg, 3: exp_avg_sq.  Synchronous. */
int etd_septrain_read(etd_septrain*, const char* name, int which, float* out_host, long long numel, void* stream);
int etd_septrain_write_moment(etd_septrain*, const char* name, int second, const float* in_host, long long numel, void* stream);
/* Decoder dropout (off at p = 0, the default): in every forward_backward call with backward != 0 the output y_j of the norm of decoder level j = 1, 2, 3
 * becomes keep ? y_j * s : 0 before anything reads it, s = 1 / (1 - p) formed in double and rounded once; dy_j is multiplied by the same mask before the norm's
 * backward.  The batch statistics are taken before the drop; a call with backward == 0 never drops.  The mask is Philox4x32-10 and is never stored: for flat
 * element e of y_j [B][n_instr][pos][C] the counter is (lo32(e >> 2), hi32(e >> 2), j, lo32(calls)), the key (lo32(seed), hi32(seed)), the element takes output
 * word e & 3 and is kept iff word < min(2^32 - 1, floor((1 - p) 2^32)).  `calls` goes up by one per dropping call.  p outside [0, 1) is ETD_EINVAL.  HOST ONLY. */
int etd_septrain_set_dropout(etd_septrain*, double p, unsigned long long seed);
int etd_septrain_set_dropout_calls(etd_septrain*, long long calls);
long long etd_septrain_get_dropout_calls(const etd_septrain*);

/* ------------------------------------------------------------------ training data of the source separator (csrc/separator_data.hip; DESIGN.md 4o is the contract,
 * tests/separator_data_np.py restates it).  The handle keeps the magnitudes of every track on the device, S [1 + n_instr][frames][F][n_channels] (0: the mix, then
 * the stems; frames = Tf rounded up to a multiple of T, zeros past Tf: what etd_sep_magnitudes writes), and cuts augmented training batches from them in one launch.
 * The device never draws a random number: the caller passes the draws. */
typedef struct etd_sepdata etd_sepdata;
typedef struct {
  int struct_bytes;            /* sizeof(etd_sepdata_cfg) of the caller: a mismatch is ETD_EINVAL */
  int n_instr, n_channels;     /* etd_sep_cfg's */
  int T, F;                    /* frames and bins of a unit: positive, T <= 65536 */
  long long max_bytes;         /* budget of the tracks' device memory; 0 = 16 GiB */
} etd_sepdata_cfg;
int etd_sepdata_create(const etd_sepdata_cfg* cfg, etd_sepdata** out);      /* needs no GPU */
void etd_sepdata_destroy(etd_sepdata*);
/* HOST ONLY: bytes a track of Tf frames holds; the bytes all tracks hold; the number of tracks; the frames Tf of one track (negative = ETD_EINVAL) */
long long etd_sepdata_track_bytes(const etd_sepdata*, long long Tf);
long long etd_sepdata_bytes(const etd_sepdata*);
int etd_sepdata_num_tracks(const etd_sepdata*);
long long etd_sepdata_track_frames(const etd_sepdata*, int track);
/* A new track of Tf frames: *mag_dev = its uninitialised S on the DEVICE, for the caller to fill (1 + n_instr calls of etd_sep_magnitudes, each writing
 * [frames][F][n_channels]); *track = its id.  A track that does not fit the budget is ETD_EINVAL with the bytes needed, and nothing is allocated. */
int etd_sepdata_add_track(etd_sepdata*, long long Tf, float** mag_dev, int* track);
/* mix[e] = ((stem_0[e] + stem_1[e]) + ...) in fp32, in instrument order, e < n.  stems: HOST array of n_instr DEVICE pointers. */
int etd_sepdata_sum_stems(etd_sepdata*, const float* const* stems_dev, long long n, float* mix_dev, void* stream);
/* One launch: unit u = (track[u], t0[u], a[u], q[u]) -> mix [B][T][F][C] and target [n_instr][B][T][F][C] (DEVICE fp32), the same draw for the mix and every stem.
 * With W = frames t0 .. t0 + T - 1 of the track (zeros from Tf on): time stretch to T' = floor(T a) frames by align-corners linear interpolation, centre crop
 * (T' >= T) or zero pad (T' < T) back to T; then the frequency axis to F' = floor(F q) bins likewise, bins f < min(F, F') kept and zeros above.  Positions and weights
 * are formed in double and the weight rounded once to fp32; lerp(u, v, w) = fmaf(w, v - u, u), time first; a = q = 1 copies the frames.  A unit's output depends on
 * its draw and its track alone.  Arrays are HOST.  ETD_EINVAL naming the unit, before the launch, for a track id outside the handle, t0 outside 0 .. Tf - 1, a
 * non-finite factor, T' < 2 or F' < 2. */
int etd_sepdata_gather(etd_sepdata*, int B, const int32_t* track, const int64_t* t0, const double* a, const double* q, float* mix_dev, float* target_dev,
                       void* stream);

/* ------------------------------------------------------------------ BSS Eval v4 scores of a separation (csrc/bss.hip; DESIGN.md 4p is the contract, tests/bss_np.py
 * restates it).  References and estimates [J][C][N] -> the eight energies per (source, window) that SDR, ISR, SIR, SAR and the plain SDR are formed from; the metrics
 * themselves are host arithmetic (etude_amd/bss.py).  This project's own contract, modelled on museval's bss_eval (v4, images, time-invariant filters): parity with
 * museval is unpinned, its lstsq fallback and its framewise-filter and permutation modes are not restated.  Everything is fp64 on the fp64 matrix cores, no atomics. */
typedef struct etd_bss etd_bss;
typedef struct {
  int struct_bytes;            /* sizeof(etd_bss_cfg) of the caller: a mismatch is ETD_EINVAL */
  int filters_len;             /* L = 512: a multiple of 16 in 16 .. 512 */
  int window;                  /* 44100: samples of a window, >= filters_len */
  int hop;                     /* 44100: 1 .. window */
  long long workspace_bytes;   /* budget of the handle's device workspace; 0 = 4 GiB */
} etd_bss_cfg;
int etd_bss_create(const etd_bss_cfg* cfg, etd_bss** out);      /* needs no GPU */
void etd_bss_destroy(etd_bss*);
/* HOST ONLY: windows of a track of N samples: floor((N - window + hop) / hop), 1 for N < window (negative = ETD_EINVAL) */
long long etd_bss_num_windows(const etd_bss*, long long N);
/* HOST ONLY: bytes of workspace a track of J sources (1 .. 8), C channels (1, 2) and N samples (>= filters_len, J C filters_len <= 8192) needs at the least: the
 * correlation partials, the matrices, the filters and one window's projections; negative = ETD_EINVAL */
long long etd_bss_workspace_bytes(const etd_bss*, int J, int C, long long N);
/* ref_ptrs / est_ptrs: HOST arrays of n_tracks DEVICE pointers, track b planar [J_host[b]][C_host[b]][N_host[b]] fp32 (finite: the caller checks).  E_ptrs[b]: DEVICE
 * fp64 [J][nwin][8] (E0 .. E7 of DESIGN.md 4p; NaN in a silent window and for a singular track), silent_ptrs[b]: DEVICE int32 [nwin], status_dev: DEVICE int32
 * [n_tracks] (1 = a Cholesky pivot was <= 0 or not finite).  A shape outside the limits, or a track that needs more than the budget (the message carries its bytes),
 * is ETD_EINVAL before anything is launched, and the handle serves the next call.  Tracks run one after another in one workspace: a track's bits are the same alone,
 * at any place in a batch, under any budget that admits it and from run to run.  Synchronises `stream` when the workspace grows. */
int etd_bss_run(etd_bss*, int n_tracks, const float* const* ref_ptrs, const float* const* est_ptrs, const int32_t* J_host, const int32_t* C_host, const int64_t* N_host,
                double* const* E_ptrs, int32_t* const* silent_ptrs, int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
