"""ctypes binding of libetude_hip.so (the C ABI declared in include/etude_hip.h).

``import torch`` happens first on purpose: torch ships its own ``libamdhip64.so`` (same SONAME as
/opt/rocm's), and loading our library afterwards makes the dynamic linker bind it to that already
loaded HIP runtime -- one runtime per process, so ``tensor.data_ptr()`` addresses and
``torch.cuda`` streams are valid inside the library.

There is NO fallback: if the shared object is missing or a symbol is absent this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

LIB_PATH = Path(os.environ["ETD_LIB_PATH"]) if os.environ.get("ETD_LIB_PATH") else Path(__file__).resolve().parent / "libetude_hip.so"     # (ETD_LIB_PATH: measurement builds side by side, tools/runs)

c_int_p = C.POINTER(C.c_int)
c_i32_p = C.POINTER(C.c_int32)
c_i64_p = C.POINTER(C.c_int64)
c_f32_p = C.POINTER(C.c_float)


class _SizedCfg(C.Structure):
    """Config structs (since ABI version 2) lead with `struct_bytes` = sizeof of the caller's layout; the library refuses any other."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_bytes = C.sizeof(type(self))


class ExtCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("n_margin", "n_frame", "n_bin", "cnn_channel", "cnn_kernel", "hid_dim", "pf_dim",
                                       "n_heads", "n_layers_enc", "n_layers_dec", "n_note", "n_velocity")] + \
               [("min_value", C.c_float), ("max_windows", C.c_int), ("chunk_frames", C.c_int), ("precision", C.c_int)]


class DecCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads",
                                       "intermediate_size", "max_position_embeddings", "num_classes",
                                       "num_attribute_bins", "attribute_emb_dim")] + \
               [("rotary_pct", C.c_float), ("rope_theta", C.c_float), ("layer_norm_eps", C.c_float),
                ("max_streams", C.c_int), ("max_ctx", C.c_int), ("precision", C.c_int), ("max_prefill_rows", C.c_int)]


class DecTaps(_SizedCfg):
    """etd_debug_dec_taps (include/etude_hip_debug.h): device destinations of the 16-bit decoder's stage taps"""
    PTRS = ("hin", "ln1", "ln2", "q", "qb", "xcat", "slabs", "hout", "step_slot", "step_pos", "next_h", "next_ln1", "next_ln2", "next_pos")
    _fields_ = [("struct_bytes", C.c_int), ("layer_mask", C.c_uint)] + [(n, C.c_int) for n in ("rows", "hidden", "intermediate", "slab_cap", "slices")] + \
               [(n, C.c_void_p) for n in PTRS]


class BeatCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("attn_len", "instr", "ntoken", "dmodel", "nhead", "d_hid", "nlayers", "norm_first",
                                       "n_mels", "tempo_out", "max_rows")]


class BeatTrainCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("attn_len", "instr", "ntoken", "dmodel", "nhead", "d_hid", "nlayers", "norm_first",
                                       "n_mels", "tempo_out", "max_rows", "max_seqs")] + [("tempo_weight", C.c_float), ("dropout", C.c_float)]


class BeatTaps(_SizedCfg):
    """etd_debug_beat_taps (include/etude_hip_debug.h): device destinations of the Beat-Transformer engine's stage taps"""
    PTRS = ("c1", "c2", "x3", "c3", "front", "ln1", "qkv", "skip", "x_attn", "tacc", "ln2", "hid", "x_ffn", "iln1", "iqkv", "iao", "ix_attn", "iln2", "ihid", "ix_ffn", "part")
    _fields_ = [("struct_bytes", C.c_int), ("layer_mask", C.c_uint)] + [(n, C.c_int) for n in ("rows", "frames", "segs", "d_hid", "slices", "islices")] + \
               [(n, C.c_void_p) for n in PTRS]


class DbnCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int), ("fps", C.c_double), ("min_bpm", C.c_double), ("max_bpm", C.c_double), ("transition_lambda", C.c_double),
                ("observation_lambda", C.c_double), ("threshold", C.c_double), ("correct", C.c_int), ("num_tempi", C.c_int), ("n_bars", C.c_int),
                ("beats_per_bar", C.c_int * 8)]


class StemFeatCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_mels", C.c_int), ("framing", C.c_int), ("amin", C.c_float), ("top_db", C.c_float)]


class DtwCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int), ("cens_window", C.c_int), ("cens_decimation", C.c_int), ("reserved", C.c_int), ("step_weights", C.c_double * 3),
                ("shift_weights", C.c_double * 3), ("alpha", C.c_float), ("norm_threshold", C.c_float)]


class AlignFeatCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("sample_rate", "hop", "fir_taps", "decimation", "chunk", "n_banks", "reserved")]


class TuningCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("sample_rate", "n_fft", "hop")]


class ResampleCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("sr_in", "sr_out", "quality", "up", "down", "half", "reserved")]


class RhythmCfg(_SizedCfg):
    _fields_ = ([("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("top_k", "precision_digits", "n_gram", "n_clusters", "n_random")]
                + [("min_ioi", C.c_double), ("max_ioi", C.c_double), ("random_host", C.POINTER(C.c_double))])


class RenderCfg(_SizedCfg):
    _fields_ = ([("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("sample_rate", "partials", "flags")]
                + [(n, C.c_double) for n in ("inharmonicity", "inharmonicity_step", "partial_rolloff", "velocity_power", "attack", "decay_base", "decay_halving",
                                             "decay_partial", "release_tau", "release_len", "gain", "nyquist_fraction")])


class SepCfg(_SizedCfg):
    _fields_ = ([("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("n_instr", "n_channels", "n_fft", "hop", "T", "F")] + [("filters", C.c_int * 6)]
                + [("separation_exponent", C.c_int), ("mask_eps", C.c_float), ("bn_eps", C.c_float), ("workspace_bytes", C.c_longlong)])


class SepDataCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("n_instr", "n_channels", "T", "F")] + [("max_bytes", C.c_longlong)]


class BssCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int), ("filters_len", C.c_int), ("window", C.c_int), ("hop", C.c_int), ("workspace_bytes", C.c_longlong)]


class AttrCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int), ("type_pos", C.c_int), ("type_note", C.c_int), ("type_duration", C.c_int)]


# etd_tuning_debug_layout's int64 [7] (include/etude_hip_debug.h), in order
TUNING_LAYOUT = ("F", "G", "off_part", "off_Y", "off_Yi", "off_R", "off_sim")

# etd_alignfeat_debug_layout's int64 [24] (include/etude_hip_debug.h), in order
ALIGNFEAT_LAYOUT = ("T", "n0", "n1", "n2", "nc0", "nc1", "nc2", "nm0", "nm1", "nm2", "off_x1", "off_x2", "off_u", "off_y", "off_st", "off_E", "off_nov", "off_ph",
                    "off_pf", "off_L", "off_g", "off_G", "off_D", "out_off")


class G3Case(_SizedCfg):
    """etd_debug_g3_case of include/etude_hip_debug.h: one k_gemm3 / k_gemm3_s launch with any epilogue, strides and row metadata"""
    _fields_ = [("struct_bytes", C.c_int), ("kernel", C.c_int), ("epi", C.c_int)] + [(n, C.c_int) for n in ("M", "N", "K", "ldx", "ldy")] + \
               [("X", C.c_void_p), ("x_elems", C.c_longlong), ("W", C.c_void_p), ("bias", C.c_void_p), ("x_bound", C.c_float),
                ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("Y", C.c_void_p), ("y_elems", C.c_longlong),
                ("add", C.c_void_p), ("hin", C.c_void_p), ("hout", C.c_void_p), ("h_elems", C.c_longlong),
                ("pos", C.c_void_p), ("slot", C.c_void_p), ("active", C.c_void_p)] + [(n, C.c_int) for n in ("n_heads", "max_ctx", "n_slots", "rope_rows")] + \
               [("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p), ("Q", C.c_void_p), ("q_elems", C.c_longlong), ("Kc", C.c_void_p), ("Vc", C.c_void_p), ("kv_elems", C.c_longlong)]


class Attn3Case(_SizedCfg):
    """etd_debug_attn3_case of include/etude_hip_debug.h: one launch_attn3 call, strided or ragged causal, with every stride, slot and bound"""
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("n_seq", "n_heads", "Sq", "Sk")] + \
               [f for x in "qkvo" for f in ((x.upper(), C.c_void_p), (x + "_elems", C.c_longlong), ("ld" + x, C.c_int), (x + "_seq", C.c_longlong))] + \
               [(n, C.c_float) for n in ("q_bound", "k_bound", "v_bound")] + [("seq_len", C.c_void_p), ("slot_of_seq", C.c_void_p), ("slot_stride", C.c_longlong)] + \
               [(n, C.c_int) for n in ("max_ctx", "n_slots", "row0")] + [("log2_out3", C.c_void_p)]


G3_KERNEL_AUTO, G3_KERNEL_TILE, G3_KERNEL_SMALL = 0, 1, 2                                            # ETD_G3_KERNEL_*
G3_EPI = {"bias": 0, "gelu": 1, "resid": 2, "logits": 3, "qkv": 4, "relu": 6}                        # ETD_G3_EPI_*


class Job(C.Structure):
    _fields_ = [("x_ids", C.c_void_p), ("x_offsets", C.c_void_p), ("n_bars", C.c_int), ("attrs4", C.c_void_p), ("ready", C.c_void_p)]


class ScoreJob(C.Structure):
    _fields_ = [("x_ids", C.c_void_p), ("x_offsets", C.c_void_p), ("n_bars", C.c_int), ("attrs4", C.c_void_p),
                ("y_ids", C.c_void_p), ("y_offsets", C.c_void_p), ("n_y_bars", C.c_int)]


class SchedCfg(_SizedCfg):
    _fields_ = [("struct_bytes", C.c_int)] + [(n, C.c_int) for n in ("bar_bos_id", "bar_eos_id", "n_ctx_pairs", "max_position_embeddings", "max_output_tokens",
                                       "max_bar_token_limit")] + [("context_overlap_ratio", C.c_float)] + \
               [(n, C.c_int) for n in ("force_bar_tokens", "max_streams", "max_prefill_rows", "steps_per_poll")] + \
               [("temperature", C.c_float), ("top_p", C.c_float), ("seed", C.c_ulonglong), ("job_key_offset", C.c_int), ("job_key_stride", C.c_int)]


class TempoRegion(C.Structure):
    _fields_ = [("bpm", C.c_double), ("time_sig", C.c_int), ("start", C.c_double), ("downbeats", C.c_void_p), ("n_downbeats", C.c_int)]


class TokEvent(C.Structure):
    _fields_ = [("type", C.c_int32), ("value", C.c_int32)]


class Note(C.Structure):
    _fields_ = [("onset", C.c_double), ("offset", C.c_double), ("pitch", C.c_int32), ("velocity", C.c_int32)]


ABI_VERSION = 3          # == ETD_ABI_VERSION of include/etude_hip.h; lib() refuses any other

# name -> (restype, argtypes); mirrors include/etude_hip.h (the boundary) and include/etude_hip_debug.h (test / measurement hooks) one to one
SIGNATURES = {
    "etd_version": (C.c_int, []),
    "etd_last_error": (C.c_char_p, []),
    "etd_build_id": (C.c_char_p, []),
    "etd_extractor_operand_type": (C.c_int, []),
    "etd_decoder_operand_type": (C.c_int, []),
    "etd_has_experiments": (C.c_int, []),
    "etd_prof_enable": (C.c_int, [C.c_int]),
    "etd_prof_reset": (C.c_int, []),
    "etd_prof_collect": (C.c_int, []),
    "etd_prof_count": (C.c_int, []),
    "etd_prof_entry": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "etd_debug_boundary_cost": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "etd_debug_linear": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]),
    "etd_debug_kernel_loop": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "etd_debug_g3_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "etd_debug_gemm3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_gemm3_case": (C.c_int, [C.POINTER(G3Case), C.c_void_p]),
    "etd_debug_ln_rows_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_g3_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_int32)]),
    "etd_debug_attn3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_debug_attn3_case": (C.c_int, [C.POINTER(Attn3Case), C.c_void_p]),
    "etd_debug_dattn_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p]),
    "etd_debug_empty_launch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_frontend_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_void_p)]),
    "etd_frontend_destroy": (None, [C.c_void_p]),
    "etd_frontend_set_pad_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "etd_rms_frames": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_frontend_resampled_len": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_frontend_num_frames": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_frontend_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                   C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_extractor_create": (C.c_int, [C.POINTER(ExtCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int,
                                       C.POINTER(C.c_void_p)]),
    "etd_extractor_destroy": (None, [C.c_void_p]),
    "etd_transcript": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_void_p] * 8 + [C.c_void_p]),
    "etd_transcript_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p]),
    "etd_extractor_debug_vel_logits": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_extractor_debug_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "etd_extractor_window_flops": (C.c_double, [C.c_void_p]),
    "etd_mpe2note": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_float,
                               C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(Note), C.c_longlong, C.POINTER(C.c_longlong)]),
    "etd_mpe2note_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Note), C.c_longlong, C.POINTER(C.c_longlong)]),
    "etd_mpe2note_dev_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "etd_mpe2note_dev_destroy": (None, [C.c_void_p]),
    "etd_mpe2note_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float,
                                   C.c_int, C.c_int, C.c_int, C.POINTER(Note), C.c_longlong, C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_mpe2note_dev_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Note), C.c_longlong, C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_tok_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "etd_tok_destroy": (None, [C.c_void_p]),
    "etd_tok_num_measures": (C.c_int, [C.c_void_p]),
    "etd_tok_measures": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_tok_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]),
    "etd_tok_split_bars": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                     C.POINTER(C.c_longlong)]),
    "etd_tok_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                 C.POINTER(C.c_longlong)]),
    "etd_midi_write": (C.c_int, [C.c_void_p, C.c_longlong, C.c_char_p]),
    "etd_decoder_create": (C.c_int, [C.POINTER(DecCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int,
                                     C.POINTER(C.c_void_p)]),
    "etd_decoder_destroy": (None, [C.c_void_p]),
    "etd_decoder_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "etd_decoder_set_sampling": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_ulonglong, C.c_void_p]),
    "etd_decoder_set_keys": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_decoder_begin_bar": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p]),
    "etd_decoder_begin_bars": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_void_p]),
    "etd_decoder_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "etd_decoder_poll": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_decoder_read_tokens": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, c_int_p, C.c_void_p]),
    "etd_decoder_read_many": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_decoder_run_jobs": (C.c_int, [C.c_void_p, C.POINTER(SchedCfg), C.POINTER(Job), C.c_int, C.c_void_p, C.c_longlong, C.c_void_p,
                                       C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_debug_assemble_prompt": (C.c_int, [C.POINTER(SchedCfg), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_int_p]),
    "etd_decoder_generate_bar": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int, C.c_int, C.c_void_p, c_int_p, C.c_void_p]),
    "etd_decoder_prefill_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p]),
    "etd_decoder_score": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 11 + [C.c_void_p]),
    "etd_decoder_score_jobs": (C.c_int, [C.c_void_p, C.POINTER(SchedCfg), C.POINTER(ScoreJob), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_assemble_scored": (C.c_int, [C.POINTER(SchedCfg), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_int_p]),
    "etd_decoder_step_bytes": (C.c_double, [C.c_void_p, C.c_int, C.c_int]),
    "etd_decoder_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p]),
    "etd_decoder_stats_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_decoder_stamp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "etd_decoder_stamp_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_debug_decoder_force_pair": (C.c_int, [C.c_void_p, C.c_int]),
    "etd_debug_decoder_step_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "etd_debug_decoder_bar_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "etd_debug_sample_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_decoder_checksum": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int, C.c_void_p]),
    "etd_debug_decoder_kv_rowsums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_debug_decoder_trace_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "etd_debug_decoder_trace_slabs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "etd_debug_decoder_trace_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "etd_debug_decoder_trace_q": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "etd_debug_decoder_stage_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_decoder_peek_kv_many": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_decoder_peek_kv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_beat_create": (C.c_int, [C.POINTER(BeatCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.POINTER(C.c_void_p)]),
    "etd_beat_destroy": (None, [C.c_void_p]),
    "etd_beat_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_beat_flops": (C.c_double, [C.c_void_p, C.c_longlong]),
    "etd_beat_debug_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_beat_debug_stage_taps": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_dbn_describe": (C.c_int, [C.POINTER(DbnCfg), C.c_int, C.c_void_p, C.c_int, c_int_p, c_int_p, c_int_p, C.c_void_p, C.c_void_p]),
    "etd_dbn_workspace_bytes": (C.c_longlong, [C.POINTER(DbnCfg), C.c_longlong, C.c_int]),
    "etd_dbn_create": (C.c_int, [C.POINTER(DbnCfg), C.POINTER(C.c_void_p)]),
    "etd_dbn_destroy": (None, [C.c_void_p]),
    "etd_dbn_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_i64_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p]),
    "etd_dbn_debug_viterbi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.POINTER(C.c_double)]),
    "etd_stemfeat_create": (C.c_int, [C.POINTER(StemFeatCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "etd_stemfeat_destroy": (None, [C.c_void_p]),
    "etd_stemfeat_num_frames": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_stemfeat_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int, c_i64_p]),
    "etd_stemfeat_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, c_i64_p, C.c_void_p, C.c_void_p]),
    "etd_dtw_create": (C.c_int, [C.POINTER(DtwCfg), C.POINTER(C.c_void_p)]),
    "etd_dtw_destroy": (None, [C.c_void_p]),
    "etd_dtw_limits": (C.c_int, [c_int_p, c_int_p, C.POINTER(C.c_longlong), c_int_p]),
    "etd_dtw_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p, c_i64_p, C.POINTER(C.c_longlong), c_i64_p]),
    "etd_dtw_align": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_i64_p, c_i64_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_dtw_debug_cost": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]),
    "etd_dtw_debug_path": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]),
    "etd_dtw_debug_total": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_longlong, C.c_longlong, C.c_int, C.POINTER(C.c_double)]),
    "etd_alignfeat_limits": (C.c_int, [c_int_p, c_int_p, C.POINTER(C.c_longlong), c_int_p, c_int_p]),
    "etd_alignfeat_create": (C.c_int, [C.POINTER(AlignFeatCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "etd_alignfeat_destroy": (None, [C.c_void_p]),
    "etd_alignfeat_num_frames": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_alignfeat_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p]),
    "etd_alignfeat_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_i64_p, c_i32_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_alignfeat_debug_layout": (C.c_int, [C.c_void_p, C.c_int, c_i64_p, C.c_int, c_i64_p, C.c_int]),
    "etd_tuning_limits": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), c_int_p]),
    "etd_tuning_create": (C.c_int, [C.POINTER(TuningCfg), C.POINTER(C.c_void_p)]),
    "etd_tuning_destroy": (None, [C.c_void_p]),
    "etd_tuning_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p]),
    "etd_tuning_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_i64_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_tuning_debug_layout": (C.c_int, [C.c_void_p, C.c_int, c_i64_p, C.c_int, c_i64_p, C.c_int]),
    "etd_tuning_debug_power": (C.c_int, [C.c_void_p, C.c_int, c_i32_p, C.c_int, C.c_void_p]),
    "etd_resample_create": (C.c_int, [C.POINTER(ResampleCfg), C.c_void_p, C.POINTER(C.c_void_p)]),
    "etd_resample_destroy": (None, [C.c_void_p]),
    "etd_resample_out_len": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_resample_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p, c_i32_p, c_i32_p]),
    "etd_resample_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_i64_p, c_i32_p, c_i32_p, c_i32_p, c_i64_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_resample_debug_layout": (C.c_int, [C.c_void_p, C.c_int, c_i64_p, c_i32_p, c_i32_p, c_i64_p, C.c_longlong, C.POINTER(C.c_longlong)]),
    "etd_rhythm_limits": (C.c_int, [c_int_p, c_int_p, c_int_p, c_int_p]),
    "etd_rhythm_create": (C.c_int, [C.POINTER(RhythmCfg), C.POINTER(C.c_void_p)]),
    "etd_rhythm_destroy": (None, [C.c_void_p]),
    "etd_rhythm_check": (C.c_int, [C.c_void_p, c_i64_p, C.c_int]),
    "etd_rhythm_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_rhythm_debug_logioi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_attr_limits": (C.c_int, [c_int_p, c_int_p, c_int_p, c_int_p]),
    "etd_attr_create": (C.c_int, [C.POINTER(AttrCfg), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "etd_attr_destroy": (None, [C.c_void_p]),
    "etd_attr_check": (C.c_int, [C.c_void_p, c_i64_p, C.c_int]),
    "etd_attr_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_i64_p, C.c_int, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_render_limits": (C.c_int, [c_int_p, C.POINTER(C.c_longlong), c_int_p, c_int_p, c_int_p]),
    "etd_render_create": (C.c_int, [C.POINTER(RenderCfg), C.POINTER(C.c_void_p)]),
    "etd_render_destroy": (None, [C.c_void_p]),
    "etd_render_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p, c_i64_p]),
    "etd_render_run": (C.c_int, [C.c_void_p, C.c_void_p, c_i64_p, C.c_void_p, C.c_int, c_i64_p, c_i64_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_render_peaks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_render_debug_plan": (C.c_int, [C.c_void_p, C.c_void_p, c_i64_p, C.c_int, c_i64_p, C.c_void_p, C.c_void_p]),
    "etd_sep_create": (C.c_int, [C.POINTER(SepCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.POINTER(C.c_void_p)]),
    "etd_sep_destroy": (None, [C.c_void_p]),
    "etd_sep_num_frames": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_sep_unit_bytes": (C.c_longlong, [C.c_void_p]),
    "etd_sep_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, c_i64_p]),
    "etd_sep_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_i64_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "etd_sep_segment_flops": (C.c_double, [C.c_void_p]),
    "etd_sep_debug_stft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sep_debug_layer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_sep_debug_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sep_debug_istft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sep_magnitudes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sep_set_mwf": (C.c_int, [C.c_void_p, C.c_int]),
    "etd_sep_get_mwf": (C.c_int, [C.c_void_p]),
    "etd_sep_debug_mwf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "etd_septrain_create": (C.c_int, [C.POINTER(SepCfg), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.POINTER(C.c_void_p)]),
    "etd_septrain_destroy": (None, [C.c_void_p]),
    "etd_septrain_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int]),
    "etd_septrain_step_flops": (C.c_double, [C.c_void_p, C.c_int]),
    "etd_septrain_forward_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "etd_septrain_zero_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_septrain_grad_norm": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "etd_septrain_step": (C.c_int, [C.c_void_p] + [C.c_double] * 5 + [C.POINTER(C.c_double), C.c_void_p]),
    "etd_septrain_set_step": (C.c_int, [C.c_void_p, C.c_longlong]),
    "etd_septrain_get_step": (C.c_longlong, [C.c_void_p]),
    "etd_septrain_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_septrain_write_moment": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_septrain_debug_dx": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_septrain_debug_dw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_septrain_debug_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_septrain_debug_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "etd_septrain_set_dropout": (C.c_int, [C.c_void_p, C.c_double, C.c_ulonglong]),
    "etd_septrain_set_dropout_calls": (C.c_int, [C.c_void_p, C.c_longlong]),
    "etd_septrain_get_dropout_calls": (C.c_longlong, [C.c_void_p]),
    "etd_septrain_debug_dropout": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sepdata_create": (C.c_int, [C.POINTER(SepDataCfg), C.POINTER(C.c_void_p)]),
    "etd_sepdata_destroy": (None, [C.c_void_p]),
    "etd_sepdata_track_bytes": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_sepdata_bytes": (C.c_longlong, [C.c_void_p]),
    "etd_sepdata_num_tracks": (C.c_int, [C.c_void_p]),
    "etd_sepdata_track_frames": (C.c_longlong, [C.c_void_p, C.c_int]),
    "etd_sepdata_add_track": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(C.c_void_p), c_int_p]),
    "etd_sepdata_sum_stems": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_sepdata_gather": (C.c_int, [C.c_void_p, C.c_int, c_i32_p, c_i64_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_bss_create": (C.c_int, [C.POINTER(BssCfg), C.POINTER(C.c_void_p)]),
    "etd_bss_destroy": (None, [C.c_void_p]),
    "etd_bss_num_windows": (C.c_longlong, [C.c_void_p, C.c_longlong]),
    "etd_bss_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int, C.c_longlong]),
    "etd_bss_run": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i32_p, c_i32_p, c_i64_p, C.POINTER(C.c_void_p),
                              C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    "etd_bss_debug_corr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_bss_debug_solve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_bss_debug_filters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_bss_debug_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_bss_debug_timing": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "etd_dtrain_workspace_bytes": (C.c_longlong, [C.POINTER(DecCfg), C.c_int]),
    "etd_dtrain_create": (C.c_int, [C.POINTER(DecCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_void_p)]),
    "etd_dtrain_destroy": (None, [C.c_void_p]),
    "etd_dtrain_bytes": (C.c_longlong, [C.c_void_p, C.c_int]),
    "etd_dtrain_forward_backward": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, c_f32_p, c_i32_p, C.c_void_p]),
    "etd_dtrain_zero_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_dtrain_grad_norm": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "etd_dtrain_clip_and_step": (C.c_int, [C.c_void_p] + [C.c_double] * 6 + [C.POINTER(C.c_double), C.c_void_p]),
    "etd_dtrain_set_step": (C.c_int, [C.c_void_p, C.c_longlong]),
    "etd_dtrain_get_step": (C.c_longlong, [C.c_void_p]),
    "etd_dtrain_read_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_dtrain_read_grad": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_dtrain_read_moment": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_dtrain_write_moment": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_debug_dtrain_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "etd_debug_dtrain_attn": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_dtrain_ln": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 11),
    "etd_debug_dtrain_gelu": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_debug_dtrain_add3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "etd_debug_dtrain_rope": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "etd_debug_dtrain_embed": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 13),
    "etd_debug_dtrain_ce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "etd_debug_dtrain_colred": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "etd_debug_dtrain_embed_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_debug_dtrain_adamw": (C.c_int, [C.c_void_p] * 4 + [C.c_longlong] + [C.c_double] * 7 + [C.c_longlong, C.c_void_p]),
    "etd_debug_dtrain_sumsq": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_void_p]),
    "etd_btrain_workspace_bytes": (C.c_longlong, [C.POINTER(BeatTrainCfg)]),
    "etd_btrain_create": (C.c_int, [C.POINTER(BeatTrainCfg), C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "etd_btrain_destroy": (None, [C.c_void_p]),
    "etd_btrain_bytes": (C.c_longlong, [C.c_void_p, C.c_int]),
    "etd_btrain_check_batch": (C.c_int, [C.POINTER(BeatTrainCfg), C.c_int, c_i64_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "etd_btrain_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_i64_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, c_f32_p, c_i32_p, c_i32_p, C.c_void_p]),
    "etd_btrain_zero_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "etd_btrain_grad_norm": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "etd_btrain_step": (C.c_int, [C.c_void_p] + [C.c_double] * 6 + [C.POINTER(C.c_double), C.c_void_p]),
    "etd_btrain_set_step": (C.c_int, [C.c_void_p, C.c_longlong]),
    "etd_btrain_get_step": (C.c_longlong, [C.c_void_p]),
    "etd_btrain_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_btrain_write": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_debug_btrain_dattn": (C.c_int, [C.c_int, c_i64_p, C.c_int, C.c_int] + [C.c_void_p] * 12),
    "etd_debug_btrain_iattn": (C.c_int, [C.c_int, c_i64_p, C.c_int] + [C.c_void_p] * 5),
    "etd_debug_btrain_fold2": (C.c_int, [C.c_int] + [C.c_void_p] * 4),
    "etd_debug_btrain_conv1_bwd": (C.c_int, [C.c_int, c_i64_p, C.c_int] + [C.c_void_p] * 8),
    "etd_debug_btrain_bce": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3),
    "etd_debug_btrain_tempo_ce": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_int] + [C.c_void_p] * 3),
    "etd_debug_btrain_read_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "etd_debug_btrain_front_fwd": (C.c_int, [C.c_int, C.c_int, c_i64_p, C.c_int] + [C.c_void_p] * 5),
    "etd_debug_btrain_front_bwd": (C.c_int, [C.c_int, C.c_int, c_i64_p, C.c_int] + [C.c_void_p] * 4),
    "etd_debug_btrain_repack": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 3),
    "etd_debug_btrain_colsum": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3),
    "etd_debug_btrain_slice_sum": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_debug_btrain_means": (C.c_int, [C.c_int, C.c_int, c_i64_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "etd_debug_btrain_relu": (C.c_int, [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3),
    "etd_debug_btrain_conv_wgrad": (C.c_int, [C.c_int] * 3 + [C.c_void_p] * 5),
    "etd_debug_btrain_ffn_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "etd_debug_btrain_proj_bwd": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "etd_debug_decoder_trace_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
}

_lib = None


class EtudeHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the library; raises if it is missing -- there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise EtudeHipError(f"{LIB_PATH} not found: build it with `python -m etude_amd.build` "
                                "(hipcc --offload-arch=gfx950); etude_amd has no CPU fallback")
        l = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("ETD_PARTIAL") and not hasattr(l, name):
                continue                   # bring-up only: a library built from a subset of the sources
            fn = getattr(l, name)          # AttributeError if the .so does not export it: fail loudly
            fn.restype = res
            fn.argtypes = args
        if l.etd_version() != ABI_VERSION:
            raise EtudeHipError(f"{LIB_PATH} speaks ABI version {l.etd_version()}, this binding {ABI_VERSION}; rebuild with `python -m etude_amd.build`")
        # provenance: the binary must have been built from the sources it sits next to (diagnostic builds opt out explicitly)
        if not os.environ.get("ETD_PARTIAL") and not os.environ.get("ETD_ALLOW_STALE_LIB"):
            from .build import src_hash
            have, want = (l.etd_build_id() or b"").decode(), src_hash()
            if have != want:
                raise EtudeHipError(f"{LIB_PATH} is stale: built from sources {have}, the tree is {want}; rebuild with `python -m etude_amd.build`")
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().etd_last_error()
        raise EtudeHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def weights_arrays(state: dict):
    """name->float32 ndarray dict  ->  (names**, ptrs**, numels*, n, keepalive)."""
    import numpy as np
    names = list(state.keys())
    arrs = [np.ascontiguousarray(np.asarray(state[k], dtype=np.float32)) for k in names]
    c_names = (C.c_char_p * len(names))(*[k.encode() for k in names])
    c_ptrs = (C.c_void_p * len(names))(*[a.ctypes.data for a in arrs])
    c_num = (C.c_int64 * len(names))(*[a.size for a in arrs])
    return c_names, c_ptrs, c_num, len(names), arrs


def prof_enable(on: bool) -> None:
    lib().etd_prof_enable(1 if on else 0)


def prof_reset() -> None:
    lib().etd_prof_reset()


def prof_report() -> dict:
    """name -> dict(ms, launches, flops, bytes) accumulated since the last reset (synchronises)."""
    l = lib()
    l.etd_prof_collect()
    out = {}
    for i in range(l.etd_prof_count()):
        name = C.create_string_buffer(64)
        ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        check(l.etd_prof_entry(i, name, 64, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "etd_prof_entry")
        out[name.value.decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
    return out
