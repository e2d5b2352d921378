"""etude_amd -- MI355X-native (gfx950) implementation of Etude's Extract and Decode hot paths.

Drop-in surfaces (same names/signatures as the reference):
    etude_amd.AMTAPC_Extractor      <- etude.data.extractor.AMTAPC_Extractor
    etude_amd.load_etude_decoder    <- etude.utils.model_loader.load_etude_decoder
    etude_amd.EtudeDecoder.generate <- etude.models.etude_decoder.EtudeDecoder.generate
    etude_amd.Vocab / Event         <- etude.data.vocab
    etude_amd.HFT_Transformer       <- etude.models.hft_transformer.HFT_Transformer (prepare.py's transcriber)
    etude_amd.TinyREMITokenizer     <- etude.data.tokenizer.TinyREMITokenizer (native encode / split / decode_to_notes)
    etude_amd.BeatDetector          <- etude.data.beat_detector.BeatDetector (the Beat-Transformer model; tracker="native" decodes with the library's own DBN)
    etude_amd.DBNBeatTracker / DBNDownBeatTracker  <- madmom's DBNBeatTrackingProcessor / DBNDownBeatTrackingProcessor (csrc/dbn.hip)
    etude_amd.StemFeatures          <- process_stems_to_spectrogram of scripts/run_separation.py (stems -> mel-dB features; csrc/stemfeat.hip)
    etude_amd.StemSeparator         <- the separator in front of them (a U-Net mask separator modelled on Spleeter's 5stems; audio -> stems; csrc/separator.hip)
    etude_amd.BeatTrainer / init_beat_state  (no counterpart: the Beat-Transformer's training -- beat / tempo loss, backward, clipping, AdamW, no dropout; csrc/beat_train.hip)
    etude_amd.SeparatorTrainer / training_segments  (no counterpart: the separator's training -- batch statistics, decoder dropout, L1 loss, backward, Adam; csrc/separator_train.hip)
    etude_amd.SegmentSampler / fit_separator / validate_separator / save_separator_checkpoint / load_separator_checkpoint  (its data and loop: tracks kept on the device,
                                    augmented batches in one launch, epochs, validation, resumable checkpoints; csrc/separator_data.hip)
    etude_amd.BSSEval / BSSEvalConfig / evaluate_separator  (its quality: BSS Eval v4 SDR / ISR / SIR / SAR per source, modelled on museval, parity unpinned; csrc/bss.hip)
    etude_amd.AlignFeatures         <- the feature extraction in front of the aligner (synctoolbox's pitch filterbank, chroma, DLNCO; csrc/alignfeat.hip)
    etude_amd.TuningEstimator / estimate_tuning  <- synctoolbox's estimate_tuning, the first call of AudioAligner._compute_alignment (csrc/tuning.hip)
    etude_amd.AudioAligner          <- etude.data.aligner.AudioAligner behind the feature extraction (exact DTW, transposition search, wp.json cache; csrc/dtw.hip)
    etude_amd.WPDCalculator         <- etude.evaluation.metrics.wpd.WPDCalculator (host arithmetic on the warping path)
    etude_amd.RGCCalculator / IPECalculator / RhythmMetrics  <- etude.evaluation.metrics.rgc / ipe (a ragged batch of note lists; csrc/rhythm.hip)
    etude_amd.EtudeDataset / BarAttributes / attribute_adherence  <- etude.data.dataset.EtudeDataset (bar attributes, bin edges, training samples; csrc/attributes.hip)
    etude_amd.NoteRenderer / PianoVoice / align_notes_many  (no counterpart: the reference leaves rendering a cover's .mid to an external synthesiser; csrc/render.hip)
    etude_amd.AudioLoader / read_wav_raw / resample_filter  <- librosa.load(path, sr=22050) and torchaudio.load in front of every chain (WAV bytes -> an engine's rate and
                                    layout: decode, mono mean and a windowed-sinc resampler of this project's own, parity unpinned; csrc/resample.hip)
    etude_amd.BeatAnalyzer          <- etude.data.beat_analyzer.BeatAnalyzer (beat_pred.json -> tempo.json; host Python)
All arithmetic runs in libetude_hip.so (hand-written HIP, see csrc/); importing the heavy
modules is lazy so that `import etude_amd` works on a box without a GPU.
"""
import os as _os

# Four decoder engines (run_engines) want four hardware queues that sit on four different compute pipes.  The HIP runtime's
# default of four queues puts the fourth engine's stream on a queue it shares with the null stream: with the default, four engines
# stepping together reach 7.8 engine-steps per ms instead of 10.0 ((history: 4ac2f57) tools/runs/r2_run15.sh vs r2_run16.sh).  The runtime reads
# this when it initialises, so it only takes effect if etude_amd is imported before the first HIP call of the process.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

__all__ = ["AMTAPC_Extractor", "EtudeDecoder", "EtudeDecoderConfig", "load_etude_decoder", "Vocab", "Event",
           "ExtractorConfig", "DecoderConfig", "HFT_Transformer", "HFTConfig", "TinyREMITokenizer", "run_engines",
           "BeatDetector", "BeatDetectorConfig", "BeatDetectorModelConfig", "DBNBeatTracker", "DBNDownBeatTracker", "BeatAnalyzer", "structuralize_many",
           "structuralize_stems_many", "StemFeatures", "mel_filterbank", "AudioAligner", "align_features", "align_features_many", "align_and_filter_many",
           "WPDCalculator", "wpd_many", "AlignFeatures", "ellip_bandpass_sos", "pitch_filterbank", "align_audio_many", "align_and_filter_audio_many",
           "TuningEstimator", "estimate_tuning", "RhythmMetrics", "RGCCalculator", "IPECalculator", "get_onsets_from_file", "rhythm_metrics_for_notes",
           "evaluate_many", "BarAttributes", "EtudeDataset", "split_into_bars", "calculate_bin_edges", "save_bin_edges", "load_bin_edges", "attribute_adherence",
           "DecoderTrainer", "cosine_schedule_with_warmup", "init_decoder_state", "NoteRenderer", "PianoVoice", "default_note_renderer", "align_notes_many",
           "read_midi_notes", "save_wav", "StemSeparator", "SeparatorConfig", "init_separator_state", "load_separator_state", "structuralize_audio_many", "SeparatorTrainer", "training_segments",
           "SegmentSampler", "fit_separator", "validate_separator", "save_separator_checkpoint", "load_separator_checkpoint",
           "BSSEval", "BSSEvalConfig", "evaluate_separator",
           "BeatTrainer", "init_beat_state",
           "AudioLoader", "resample_filter", "resampled_len", "read_wav_raw", "align_files_many", "structuralize_files_many"]


def __getattr__(name):
    if name == "AMTAPC_Extractor":
        from .extractor import AMTAPC_Extractor
        return AMTAPC_Extractor
    if name in ("EtudeDecoder", "EtudeDecoderConfig", "load_etude_decoder", "run_engines"):
        from . import decoder
        return getattr(decoder, name)
    if name in ("Vocab", "Event"):
        from . import vocab
        return getattr(vocab, name)
    if name == "TinyREMITokenizer":
        from .tokenizer import TinyREMITokenizer
        return TinyREMITokenizer
    if name == "HFT_Transformer":
        from .hft_transformer import HFT_Transformer
        return HFT_Transformer
    if name == "BeatDetector":
        from .beat import BeatDetector
        return BeatDetector
    if name in ("DBNBeatTracker", "DBNDownBeatTracker"):
        from . import dbn
        return getattr(dbn, name)
    if name in ("StemFeatures", "mel_filterbank"):
        from . import stemfeat
        return getattr(stemfeat, name)
    if name in ("AlignFeatures", "ellip_bandpass_sos", "pitch_filterbank"):
        from . import alignfeat
        return getattr(alignfeat, name)
    if name in ("TuningEstimator", "estimate_tuning"):
        from . import tuning
        return getattr(tuning, name)
    if name in ("RhythmMetrics", "RGCCalculator", "IPECalculator", "get_onsets_from_file", "rhythm_metrics_for_notes", "evaluate_many", "read_midi_notes"):
        from . import rhythm
        return getattr(rhythm, name)
    if name in ("BarAttributes", "EtudeDataset", "split_into_bars", "calculate_bin_edges", "save_bin_edges", "load_bin_edges", "attribute_adherence"):
        from . import attributes
        return getattr(attributes, name)
    if name in ("AudioAligner", "align_features", "align_features_many", "align_and_filter_many", "align_audio_many", "align_and_filter_audio_many", "align_notes_many", "align_files_many"):
        from . import aligner
        return getattr(aligner, name)
    if name in ("NoteRenderer", "PianoVoice", "default_note_renderer"):
        from . import render
        return getattr(render, name)
    if name == "save_wav":
        from .extractor import save_wav
        return save_wav
    if name in ("WPDCalculator", "wpd_many"):
        from . import evaluation
        return getattr(evaluation, name)
    if name in ("SeparatorTrainer", "training_segments"):
        from . import separator_train
        return getattr(separator_train, name)
    if name == "SegmentSampler":
        from .separator_data import SegmentSampler
        return SegmentSampler
    if name in ("fit_separator", "validate_separator", "save_separator_checkpoint", "load_separator_checkpoint"):
        from . import separator_data
        return getattr(separator_data, {"fit_separator": "fit", "validate_separator": "validate", "save_separator_checkpoint": "save_checkpoint",
                                        "load_separator_checkpoint": "load_checkpoint"}[name])
    if name in ("AudioLoader", "resample_filter", "resampled_len", "read_wav_raw"):
        from . import audio
        return getattr(audio, name)
    if name in ("BSSEval", "BSSEvalConfig"):
        from . import bss
        return getattr(bss, name)
    if name == "evaluate_separator":
        from .separator_eval import evaluate_separator
        return evaluate_separator
    if name in ("StemSeparator", "SeparatorConfig", "init_separator_state", "load_separator_state"):
        from . import separator
        return getattr(separator, name)
    if name in ("BeatAnalyzer", "structuralize_many", "structuralize_stems_many", "structuralize_audio_many", "structuralize_files_many"):
        from . import beat_analyzer
        return getattr(beat_analyzer, name)
    if name in ("BeatTrainer", "init_beat_state"):
        from . import beat_train
        return getattr(beat_train, name)
    if name in ("DecoderTrainer", "cosine_schedule_with_warmup", "init_decoder_state"):
        from . import train
        return getattr(train, name)
    if name in ("ExtractorConfig", "DecoderConfig", "HFTConfig", "BeatDetectorConfig", "BeatDetectorModelConfig"):
        from . import config
        return getattr(config, name)
    raise AttributeError(name)
