"""Beat-Transformer beat / downbeat activations on the MI355X: ``BeatDetector`` <- etude.data.beat_detector.BeatDetector.

``BeatDetector(config, model_path, device).detect(input_npy_path, output_json_path, cleanup_input)`` (etude/data/beat_detector.py:99-164): the model
(Demixed_DilatedTransformerModel, etude/models/beat_transformer.py) runs in libetude_hip.so (csrc/beat.hip, exact-parity fp32-grade arithmetic).  The DBN trackers
that turn the activations into beat times are, by default (``tracker="madmom"``), madmom's, imported lazily by ``detect``; ``tracker="native"`` uses the library's
own (csrc/dbn.hip, etude_amd/dbn.py) on the logits where they lie on the device, and ``detect_many`` (native only) does so for many songs in one ragged model pass
plus one tracking call.  ``detect_stems_many`` / ``activations_from_stems_many`` start one step earlier, from the separated stems: ``etude_amd.StemFeatures`` makes the
features on the device and they go straight into the model.

Other entry points: ``activations(features)`` -> (beat, downbeat) float32 arrays (what the reference hands to madmom), ``activations_many([features, ...])`` (one
ragged pass for many songs: prepare.py's use), ``forward(x [B][instr][T][128])`` -> (logits [B][T][ntoken], tempo [B][300]).

Input precondition: finite features with |x| <= 80 (``power_to_db``'s top_db floor, scripts/run_separation.py:176-183); every entry point checks it BEFORE anything is
launched and raises ValueError otherwise.
"""
from __future__ import annotations

import ctypes as C
import json
import warnings
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, i64
from .config import BeatDetectorConfig

FEATURE_BOUND = 80.0


def _check_range(x: torch.Tensor, what: str) -> None:
    if x.numel() == 0:
        return
    amax = float(x.detach().abs().amax())          # (NaN propagates through amax)
    if not amax <= FEATURE_BOUND:
        raise ValueError(f"{what}: features must be finite with |x| <= {FEATURE_BOUND:g} (power_to_db output, top_db = 80); got max |x| = {amax}")


def load_state_dict(model_path: Union[str, Path], map_location="cpu") -> Dict[str, torch.Tensor]:
    """beat_detector.py:93-95: torch.load(weights_only=True), then the nested "state_dict" if present; no prefix stripping."""
    ck = torch.load(model_path, map_location=map_location, weights_only=True)
    return ck.get("state_dict", ck)


def expected_keys(cfg) -> Dict[str, tuple]:
    """key -> shape of Demixed_DilatedTransformerModel.state_dict() for a model config (beat_transformer.py:23-52)"""
    D, H, nh, L = cfg.dmodel, cfg.d_hid, cfg.nhead, cfg.attn_len
    k = {"conv1.weight": (32, 1, 5, 3), "conv1.bias": (32,), "conv2.weight": (64, 32, 1, 12), "conv2.bias": (64,), "conv3.weight": (D, 64, 3, 6), "conv3.bias": (D,)}
    for l in range(cfg.nlayers):
        p = f"Transformer_layers.time_attention_{l}."
        for n in ("key", "value", "query"):
            k[p + f"self_attn.{n}.weight"], k[p + f"self_attn.{n}.bias"] = (D, D), (D,)
        k[p + "self_attn.Er"] = (nh, D // nh, L)
        k[p + "linear1.weight"], k[p + "linear1.bias"], k[p + "linear2.weight"], k[p + "linear2.bias"] = (H, D), (H,), (D, H), (D,)
        for n in ("norm1", "norm2"):
            k[p + f"{n}.weight"], k[p + f"{n}.bias"] = (D,), (D,)
        if 3 <= l <= 5:
            q = f"Transformer_layers.instr_attention_{l}."
            k[q + "self_attn.in_proj_weight"], k[q + "self_attn.in_proj_bias"] = (3 * D, D), (3 * D,)
            k[q + "self_attn.out_proj.weight"], k[q + "self_attn.out_proj.bias"] = (D, D), (D,)
            k[q + "linear1.weight"], k[q + "linear1.bias"], k[q + "linear2.weight"], k[q + "linear2.bias"] = (H, D), (H,), (D, H), (D,)
            for n in ("norm1", "norm2"):
                k[q + f"{n}.weight"], k[q + f"{n}.bias"] = (D,), (D,)
    k["out_linear.weight"], k["out_linear.bias"] = (cfg.ntoken, D), (cfg.ntoken,)
    k["out_linear_t.weight"], k["out_linear_t.bias"] = (300, D), (300,)
    return k


def check_state_dict(sd: Dict, cfg) -> None:
    """strict load_state_dict semantics: missing / unexpected keys and shape mismatches raise RuntimeError"""
    want = expected_keys(cfg)
    missing = sorted(set(want) - set(sd))
    unexpected = sorted(set(sd) - set(want))
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for Demixed_DilatedTransformerModel: missing keys {missing[:8]}, unexpected keys {unexpected[:8]}")
    bad = [(k, tuple(np.shape(sd[k])), s) for k, s in want.items() if tuple(np.shape(sd[k])) != s]
    if bad:
        raise RuntimeError(f"Error(s) in loading state_dict for Demixed_DilatedTransformerModel: size mismatch {bad[:4]}")


class BeatDetector(Engine):
    _destroy = "etd_beat_destroy"

    def __init__(self, config: Optional[BeatDetectorConfig] = None, model_path: Union[str, Path, None] = None, device: Union[str, torch.device] = "auto",
                 state_dict: Optional[Dict] = None, max_rows: int = 1 << 17, tracker: str = "madmom"):
        self.config = config if config is not None else BeatDetectorConfig()
        if tracker not in ("madmom", "native"):
            raise ValueError(f"BeatDetector: tracker must be 'madmom' or 'native', got {tracker!r}")
        self.tracker = tracker
        self._dbn = None
        if device == "auto":
            device = "cuda"
        self.device = torch.device(device)
        self._device()
        if state_dict is None:
            if model_path is None:
                raise ValueError("BeatDetector: model_path (or state_dict) is required")
            state_dict = load_state_dict(model_path)
        m = self.config.model
        check_state_dict(state_dict, m)
        sd = {k: (v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)) for k, v in state_dict.items()}
        self.fps = 44100 / self.config.fps_divisor
        cfg = _lib.BeatCfg(attn_len=m.attn_len, instr=m.instr, ntoken=m.ntoken, dmodel=m.dmodel, nhead=m.nhead, d_hid=m.d_hid, nlayers=m.nlayers,
                           norm_first=1 if m.norm_first else 0, n_mels=128, tempo_out=300, max_rows=int(max_rows))
        names, ptrs, nums, n, keep = _lib.weights_arrays(sd)
        h = C.c_void_p()
        lib = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.check(lib.etd_beat_create(C.byref(cfg), names, ptrs, nums, n, C.byref(h)), "etd_beat_create")
        del keep
        self._adopt(h)
        self._lib = lib
        self.instr, self.ntoken = m.instr, m.ntoken

    # ------------------------------------------------------------------ model
    def _run(self, feat: torch.Tensor, Ts: Sequence[int], want_tempo: bool = True):
        """feat: contiguous device fp32, the songs' [instr][T][128] blocks back to back -> (logits [sum T][ntoken], tempo [n][300])"""
        n = len(Ts)
        logits = torch.empty((int(sum(Ts)), self.ntoken), dtype=torch.float32, device=self.device)
        tempo = torch.empty((n, 300), dtype=torch.float32, device=self.device) if want_tempo else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.etd_beat_forward(self.h, C.c_void_p(feat.data_ptr()), n, i64(Ts), C.c_void_p(logits.data_ptr()),
                                                  C.c_void_p(tempo.data_ptr()) if tempo is not None else None, self._stream(self.device)), "etd_beat_forward")
        return logits, tempo

    def _songs_to_device(self, songs: Sequence) -> Tuple[torch.Tensor, List[int]]:
        ts = []
        for i, f in enumerate(songs):
            t = torch.as_tensor(f)
            if t.dim() != 3 or t.shape[0] != self.instr or t.shape[2] != 128 or t.shape[1] < 1:
                raise ValueError(f"song {i}: features must be [instr={self.instr}][T >= 1][128], got {tuple(t.shape)}")
            _check_range(t, f"song {i}")
            ts.append(t)
        feat = torch.cat([t.to(torch.float32).reshape(-1) for t in ts]).to(self.device).contiguous()
        return feat, [int(t.shape[1]) for t in ts]

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Demixed_DilatedTransformerModel.forward: x [B][instr][T][128] -> (logits [B][T][ntoken], tempo [B][300]) on the device"""
        if x.dim() != 4 or x.shape[1] != self.instr or x.shape[3] != 128 or x.shape[2] < 1 or x.shape[0] < 1:
            raise ValueError(f"forward: x must be [B][instr={self.instr}][T >= 1][128], got {tuple(x.shape)}")
        _check_range(x, "forward")
        B, T = int(x.shape[0]), int(x.shape[2])
        feat = x.to(self.device, torch.float32).contiguous()
        logits, tempo = self._run(feat, [T] * B)
        return logits.view(B, T, self.ntoken), tempo

    __call__ = forward

    def activations_many(self, songs: Sequence) -> List[Tuple[np.ndarray, np.ndarray]]:
        """one ragged pass over many songs' [instr][T_s][128] features -> [(beat, downbeat)] float32 sigmoid activations per song"""
        if len(songs) == 0:
            return []
        feat, Ts = self._songs_to_device(songs)
        logits, _ = self._run(feat, Ts, want_tempo=False)
        act = torch.sigmoid(logits).cpu().numpy()
        out, o = [], 0
        for T in Ts:
            out.append((np.ascontiguousarray(act[o:o + T, 0]), np.ascontiguousarray(act[o:o + T, 1])))
            o += T
        return out

    def activations(self, features) -> Tuple[np.ndarray, np.ndarray]:
        """beat_detector.py:121-131: [instr][T][128] -> (sigmoid(logits[:, 0]), sigmoid(logits[:, 1])) as float32 numpy arrays"""
        return self.activations_many([features])[0]

    # ------------------------------------------------------------------ detect (beat_detector.py:99-164)
    def _trackers(self):
        try:
            from madmom.features.beats import DBNBeatTrackingProcessor
            from madmom.features.downbeats import DBNDownBeatTrackingProcessor
        except ImportError as e:
            raise ImportError("BeatDetector.detect needs madmom (DBNBeatTrackingProcessor / DBNDownBeatTrackingProcessor) for the beat / downbeat "
                              "decoding; install madmom or use activations() and decode elsewhere") from e
        c = self.config
        beat = DBNBeatTrackingProcessor(min_bpm=c.min_bpm, max_bpm=c.max_bpm, fps=self.fps, threshold=c.threshold)
        down = DBNDownBeatTrackingProcessor(beats_per_bar=c.beats_per_bar, min_bpm=c.min_bpm, max_bpm=c.max_bpm, fps=self.fps, threshold=c.threshold)
        return beat, down

    def _native(self):
        """the library's DBN trackers for this config (beat HMM + one bar HMM per beats_per_bar entry), created on first use"""
        if self._dbn is None:
            from .dbn import DBNEngine
            c = self.config
            self._dbn = DBNEngine(self.fps, c.min_bpm, c.max_bpm, c.threshold, list(c.beats_per_bar), self.device)
        return self._dbn

    def _detect_native(self, songs: Sequence) -> List[Dict]:
        """one ragged model pass + one tracking call; the activations never leave the device"""
        self._native()
        feat, Ts = self._songs_to_device(songs)
        return self._detect_packed(feat, Ts)

    def _detect_packed(self, feat: torch.Tensor, Ts: Sequence[int]) -> List[Dict]:
        """the same from features already packed on the device (``_run``'s layout), range-checked by the caller"""
        from .dbn import IN_ACTIVATIONS
        dbn = self._native()
        logits, _ = self._run(feat, Ts, want_tempo=False)
        act = torch.sigmoid(logits[:, :2]).contiguous()          # the same fp32 sigmoid activations() returns
        out = []
        for beats, rows, _ in dbn.track(act, Ts, IN_ACTIVATIONS):
            down = rows[rows[:, 1] == 1][:, 0]
            out.append({"beat_pred": (beats.astype(np.float64) / self.fps).tolist(), "downbeat_pred": (down.astype(np.float64) / self.fps).tolist()})
        return out

    @staticmethod
    def _write_json(results: Dict, output_json_path) -> None:
        output_file = Path(output_json_path)
        output_file.parent.mkdir(parents=True, exist_ok=True)
        with open(output_file, "w") as f:
            json.dump(results, f, indent=4)

    def detect_many(self, features_or_paths: Sequence, output_json_paths: Optional[Sequence] = None, cleanup_input: bool = False) -> List[Dict]:
        """``detect`` for many songs with the native trackers: entries are [instr][T][128] feature arrays or paths of .npy files holding them; ``output_json_paths``
        (one per song, entries may be None) are written like ``detect`` writes its own; ``cleanup_input`` unlinks the entries that were paths."""
        if output_json_paths is not None and len(output_json_paths) != len(features_or_paths):
            raise ValueError("detect_many: one output path per song")
        if len(features_or_paths) == 0:
            return []
        paths = [Path(f) if isinstance(f, (str, Path)) else None for f in features_or_paths]
        songs = [np.load(p) if p is not None else f for p, f in zip(paths, features_or_paths)]
        results = self._detect_native(songs)
        for i, r in enumerate(results):
            if output_json_paths is not None and output_json_paths[i]:
                self._write_json(r, output_json_paths[i])
        if cleanup_input:
            for p in paths:
                if p is not None and p.exists():
                    p.unlink()
        return results

    # ------------------------------------------------------------------ from separated stems (etude_amd.StemFeatures: the features are made on the device)
    def _stem_features(self, stem_features=None):
        if stem_features is None:
            if getattr(self, "_stemfeat", None) is None:
                from .stemfeat import StemFeatures
                self._stemfeat = StemFeatures(device=self.device)
            stem_features = self._stemfeat
        if stem_features.n_mels != 128:
            raise ValueError(f"stem_features: the model reads 128 mel bands, this StemFeatures makes {stem_features.n_mels}")
        return stem_features

    def _features_from_stems(self, stems_list: Sequence, stem_features=None) -> Tuple[torch.Tensor, List[int]]:
        """stems -> the packed device feature buffer ``_run`` reads: written once by the feature kernels, checked where it lies (a NaN or Inf sample, or a
        StemFeatures with top_db > 80, is refused here, before the model launches), never copied or concatenated"""
        sf = self._stem_features(stem_features)
        for i, x in enumerate(stems_list):
            if hasattr(x, "shape") and len(x.shape) == 3 and x.shape[0] != self.instr:
                raise ValueError(f"song {i}: stems must be [instr={self.instr}][channels][N], got {tuple(x.shape)}")
        feat, Ts = sf.features_many(stems_list)
        if feat.device != self.device:
            raise ValueError(f"stem_features works on {feat.device}, the detector on {self.device}")
        _check_range(feat, "stem features")
        return feat, Ts

    def activations_from_stems_many(self, stems_list: Sequence, stem_features=None) -> List[Tuple[np.ndarray, np.ndarray]]:
        """``activations_many`` from the songs' separated stems [instr][channels][N_s] (device or host tensors, numpy arrays)"""
        if len(stems_list) == 0:
            return []
        feat, Ts = self._features_from_stems(stems_list, stem_features)
        logits, _ = self._run(feat, Ts, want_tempo=False)
        act = torch.sigmoid(logits).cpu().numpy()
        out, o = [], 0
        for T in Ts:
            out.append((np.ascontiguousarray(act[o:o + T, 0]), np.ascontiguousarray(act[o:o + T, 1])))
            o += T
        return out

    def detect_stems_many(self, stems_list: Sequence, output_json_paths: Optional[Sequence] = None, stem_features=None) -> List[Dict]:
        """``detect_many`` from the songs' separated stems: features (``stem_features``, default ``StemFeatures()`` = the Demucs branch of run_separation.py), model and
        the native trackers in one pass each, with nothing but the beat frames coming back from the device"""
        if output_json_paths is not None and len(output_json_paths) != len(stems_list):
            raise ValueError("detect_stems_many: one output path per song")
        if len(stems_list) == 0:
            return []
        self._native()
        feat, Ts = self._features_from_stems(stems_list, stem_features)
        results = self._detect_packed(feat, Ts)
        for i, r in enumerate(results):
            if output_json_paths is not None and output_json_paths[i]:
                self._write_json(r, output_json_paths[i])
        return results

    def detect_audio_many(self, separator, wavs: Sequence, output_json_paths: Optional[Sequence] = None) -> List[Dict]:
        """``detect_stems_many`` from the songs' audio: ``separator`` (an ``etude_amd.StemSeparator`` with this model's instruments) makes the stems on the device,
        ``StemFeatures(framing="spleeter")`` reads them where they lie, and the stems path takes over; no stem or feature visits the host"""
        if len(separator.config.instruments) != self.instr:
            raise ValueError(f"detect_audio_many: the separator makes {len(separator.config.instruments)} stems, the model reads {self.instr}")
        if getattr(self, "_stemfeat_spleeter", None) is None or self._stemfeat_spleeter.sample_rate != separator.config.sample_rate:
            from .stemfeat import StemFeatures
            self._stemfeat_spleeter = StemFeatures(sample_rate=separator.config.sample_rate, framing="spleeter", device=self.device)
        return self.detect_stems_many(separator.separate_many(wavs), output_json_paths, stem_features=self._stemfeat_spleeter)

    def detect(self, input_npy_path: Union[str, Path], output_json_path: Optional[Union[str, Path]] = None, cleanup_input: bool = True) -> Dict:
        if self.tracker == "native":
            input_file = Path(input_npy_path)
            results = self._detect_native([np.load(input_file)])[0]
            if output_json_path:
                self._write_json(results, output_json_path)
            if cleanup_input and input_file.exists():
                input_file.unlink()
            return results
        beat_tracker, downbeat_tracker = self._trackers()          # (before any GPU work: a missing madmom fails here)
        input_file = Path(input_npy_path)
        features = np.load(input_file)
        beat_activation, downbeat_activation = self.activations(features)
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", category=RuntimeWarning)
            dbn_beat_pred = beat_tracker(beat_activation)
            beat_minus_downbeat = np.maximum(beat_activation - downbeat_activation, 0)
            combined_act = np.stack([beat_minus_downbeat, downbeat_activation], axis=-1)
            dbn_downbeat_pred_raw = downbeat_tracker(combined_act)
        dbn_downbeat_pred = dbn_downbeat_pred_raw[dbn_downbeat_pred_raw[:, 1] == 1][:, 0]
        results = {"beat_pred": dbn_beat_pred.tolist(), "downbeat_pred": dbn_downbeat_pred.tolist()}
        if output_json_path:
            output_file = Path(output_json_path)
            output_file.parent.mkdir(parents=True, exist_ok=True)
            with open(output_file, "w") as f:
                json.dump(results, f, indent=4)
        if cleanup_input and input_file.exists():
            input_file.unlink()
        return results

    # ------------------------------------------------------------------ measurement
    def flops(self, T: int) -> float:
        """algorithmic FLOPs of one song of T frames"""
        return float(self._lib.etd_beat_flops(self.h, int(T)))

    def debug_taps(self, front: Optional[torch.Tensor], layer0: Optional[torch.Tensor]) -> None:
        """test hook: following calls copy the token rows after the front end / time layer 0 into these [rows][256] device tensors (None = off)"""
        _lib.check(self._lib.etd_beat_debug_taps(self.h, C.c_void_p(front.data_ptr()) if front is not None else None,
                                                 C.c_void_p(layer0.data_ptr()) if layer0 is not None else None), "etd_beat_debug_taps")

    def debug_stage_taps(self, layer_mask: int = 0, rows: int = 0, frames: int = 0, segs: int = 0, slices: int = 0, islices: int = 0, **bufs: torch.Tensor) -> None:
        """Test hook (etd_beat_debug_stage_taps): register contiguous fp32 device tensors as the destinations of every launch's output, named as the members of
        etd_debug_beat_taps and shaped as include/etude_hip_debug.h states; no tensors = taps off.  The caller keeps the tensors alive."""
        if not bufs:
            _lib.check(self._lib.etd_beat_debug_stage_taps(self.h, None), "etd_beat_debug_stage_taps")
            return
        t = _lib.BeatTaps(layer_mask=int(layer_mask), rows=int(rows), frames=int(frames), segs=int(segs), d_hid=int(self.config.model.d_hid), slices=int(slices),
                          islices=int(islices))
        per = {"tacc": frames, "part": segs}
        width = dict(c1=42 * 32, c2=42 * 64, x3=3 * 1152, c3=3 * 256, qkv=768, iqkv=768, hid=t.d_hid, ihid=t.d_hid)
        for k, v in bufs.items():
            if k not in _lib.BeatTaps.PTRS or v.device != self.device or v.dtype != torch.float32 or not v.is_contiguous():
                raise ValueError(f"debug_stage_taps: {k} must name a tap and be a contiguous fp32 device tensor")
            n_sl = 1 if k in ("c1", "c2", "x3", "c3", "front", "part") else islices if k.startswith("i") else slices
            need = n_sl * per.get(k, rows) * width.get(k, 256)
            if v.numel() < need:
                raise ValueError(f"debug_stage_taps: {k} holds {v.numel()} floats, the stated sizes need {need}")
            setattr(t, k, v.data_ptr())
        _lib.check(self._lib.etd_beat_debug_stage_taps(self.h, C.byref(t)), "etd_beat_debug_stage_taps")


def structuralize_files_many(detector: BeatDetector, separator, paths: Sequence, loader=None) -> List[List[Dict]]:
    """WAV files of any rate -> their tempo.json rows: ``beat_analyzer.structuralize_files_many`` under the detector's module name"""
    from .beat_analyzer import structuralize_files_many as run
    return run(detector, separator, paths, loader)
