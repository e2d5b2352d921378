"""Stage 3 "Align & Filter" on the MI355X: ``AudioAligner`` stands in for etude.data.aligner.AudioAligner (etude/data/aligner.py) behind the feature extraction.

The reference aligns a cover to its origin with synctoolbox: CENS features -> compute_optimal_chroma_shift -> sync_via_mrmsdtw (multi-resolution DTW, an approximation
a host needs) -> make_path_strictly_monotonic.  Here the exact full-resolution DTW runs in libetude_hip.so (csrc/dtw.hip, DESIGN.md 4e is the contract): one wave per
pair for a ragged batch of pairs, the 12 transposition problems in a launch of their own, 2-bit backpointers, and one copy of O(N1 + N2) integers to the host per call.

The feature extraction in front (estimate_tuning, audio_to_pitch_features, audio_to_pitch_onset_features, DLNCO: synctoolbox's multirate IIR filterbank) enters
``AudioAligner(feature_fn=...)`` as a callable path -> (quantized chroma [12][N], DLNCO [12][N]); without one a cache miss returns None.  The library's own is
``AlignFeatures.as_feature_fn(load_fn, tuning_fn="estimate")`` (csrc/alignfeat.hip, csrc/tuning.hip); ``align_audio_many(pairs, "estimate")`` is the batch form.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, i64, nonneg, ptrs

log = logging.getLogger(__name__)

HDR = 8          # DTW_HDR of csrc/dtw.h: int32 header of a pair's result block
Feats = Tuple[Union[np.ndarray, torch.Tensor], Union[np.ndarray, torch.Tensor]]      # (quantized chroma [12][N], DLNCO [12][N])


def limits() -> dict:
    """Host only: the constants of the built library (rows of a row block, cells per backpointer word, frames per side, pairs per call)."""
    b, w, p, f = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    _lib.check(_lib.lib().etd_dtw_limits(C.byref(b), C.byref(w), C.byref(f), C.byref(p)), "etd_dtw_limits")
    return dict(row_block=b.value, cells_per_word=w.value, max_frames=f.value, max_pairs=p.value)


def make_cfg(step_weights=(1.5, 1.5, 2.0), shift_weights=(1.0, 1.0, 1.0), alpha: float = 0.5, norm_threshold: float = 1e-3, cens_window: int = 201,
             cens_decimation: int = 50) -> "_lib.DtwCfg":
    cfg = _lib.DtwCfg(cens_window=int(cens_window), cens_decimation=int(cens_decimation), reserved=0, alpha=float(alpha), norm_threshold=float(norm_threshold))
    for k in range(3):
        cfg.step_weights[k] = float(step_weights[k])
        cfg.shift_weights[k] = float(shift_weights[k])
    return cfg


class DTWEngine(Engine):
    """One etd_dtw handle."""
    _destroy = "etd_dtw_destroy"

    def __init__(self, device="cuda", **cfg):
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.EtudeHipError("etude_amd's DTW needs a ROCm GPU (device='cuda'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cfg = make_cfg(**cfg)
        self._lib = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._lib.etd_dtw_create(C.byref(self.cfg), C.byref(h)), "etd_dtw_create")
        self._adopt(h)

    # ---- sizes (host arithmetic)
    def workspace_bytes(self, N1s: Sequence[int], N2s: Sequence[int]) -> Tuple[int, int, np.ndarray]:
        """-> (workspace bytes, int32 elements of the result buffer, each pair's offset in it)"""
        n = len(N1s)
        r, off = C.c_longlong(), (C.c_int64 * max(n, 1))()
        ws = nonneg(self._lib.etd_dtw_workspace_bytes(self.h, n, i64(N1s), i64(N2s), C.byref(r), off), "etd_dtw_workspace_bytes")
        return ws, int(r.value), np.array(off[:n], np.int64)

    # ---- input checks
    def _to_device(self, x, what: str, nonneg: bool) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            t = x.detach()
            if t.dim() != 2 or t.shape[0] != 12 or t.shape[1] < 1:
                raise ValueError(f"{what}: need [12][N >= 1], got {tuple(t.shape)}")
            t = t.to(self.device, torch.float32).contiguous()
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{what}: holds a non-finite value")
            if nonneg and bool((t < 0).any()):
                raise ValueError(f"{what}: holds a negative value")
            return t
        a = np.asarray(x)
        if a.ndim != 2 or a.shape[0] != 12 or a.shape[1] < 1:
            raise ValueError(f"{what}: need [12][N >= 1], got {a.shape}")
        a = np.ascontiguousarray(a, np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: holds a non-finite value")
        if nonneg and (a < 0).any():
            raise ValueError(f"{what}: holds a negative value")
        return torch.from_numpy(a).to(self.device)

    def _pair(self, i: int, cover: Feats, origin: Feats) -> List[torch.Tensor]:
        if len(cover) != 2 or len(origin) != 2:
            raise ValueError(f"pair {i}: each side is (quantized chroma, DLNCO)")
        ts = [self._to_device(cover[0], f"pair {i}: cover chroma", True), self._to_device(cover[1], f"pair {i}: cover DLNCO", False),
              self._to_device(origin[0], f"pair {i}: origin chroma", True), self._to_device(origin[1], f"pair {i}: origin DLNCO", False)]
        if ts[0].shape != ts[1].shape or ts[2].shape != ts[3].shape:
            raise ValueError(f"pair {i}: chroma and DLNCO of one side differ in length ({tuple(ts[0].shape)} / {tuple(ts[1].shape)}, {tuple(ts[2].shape)} / {tuple(ts[3].shape)})")
        return ts

    # ---- the call
    def align_raw(self, tensors: Sequence[Sequence[torch.Tensor]], ws: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
        """tensors: per pair the four checked device tensors.  ws (uint8) / res (int32): device buffers of the caller's own (tests put canaries around them).
        -> (the result buffer on the host, each pair's offset in it)"""
        n = len(tensors)
        N1s, N2s = [int(t[0].shape[1]) for t in tensors], [int(t[2].shape[1]) for t in tensors]
        ws_bytes, res_ints, off = self.workspace_bytes(N1s, N2s)
        with torch.cuda.device(self.device):
            if ws is None:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            if res is None:
                res = torch.empty(res_ints, dtype=torch.int32, device=self.device)
            host = np.zeros(res_ints, np.int32)
            _lib.check(self._lib.etd_dtw_align(self.h, ptrs([t for ts in tensors for t in ts]), n, i64(N1s), i64(N2s), C.c_void_p(ws.data_ptr()),
                                               ws.numel() * ws.element_size(), C.c_void_p(res.data_ptr()), res.numel(), host.ctypes.data,
                                               self._stream(self.device)), "etd_dtw_align")
        return host, off

    def align_many(self, pairs: Sequence[Tuple[Feats, Feats]], details: bool = False) -> List[Dict]:
        """pairs: (cover feats, origin feats) each -> the reference's result dicts (aligner.py:128-133); details adds "opt_shift" and "total" (D[-1,-1])."""
        if len(pairs) == 0:
            return []
        tensors = [self._pair(i, c, o) for i, (c, o) in enumerate(pairs)]
        host, off = self.align_raw(tensors)
        out = []
        for p, ts in enumerate(tensors):
            N1, N2 = int(ts[0].shape[1]), int(ts[2].shape[1])
            cap = min(N1, N2) + 1
            blk = host[off[p]: off[p] + HDR + 2 * cap]
            L = int(blk[0])
            r = {"wp": np.stack([blk[HDR: HDR + L], blk[HDR + cap: HDR + cap + L]]).astype(np.int64), "pitch_shift": int(blk[2]),
                 "num_frames_cover": N1, "num_frames_origin": N2}
            if details:
                r["opt_shift"] = int(blk[1])
                r["total"] = float(blk[4:6].view(np.float64)[0])
            out.append(r)
        return out

    # ---- test hooks
    def debug_cost(self, cover: Feats, origin: Feats, shift: int) -> np.ndarray:
        ts = self._pair(0, cover, origin)
        N1, N2 = int(ts[0].shape[1]), int(ts[2].shape[1])
        with torch.cuda.device(self.device):
            out = torch.empty((N1, N2) if N1 * N2 <= (1 << 22) else (1,), dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)
            _lib.check(self._lib.etd_dtw_debug_cost(self.h, ptrs(ts), N1, N2, int(shift), C.c_void_p(out.data_ptr())), "etd_dtw_debug_cost")
            return out.cpu().numpy()

    def debug_path(self, cover: Feats, origin: Feats, shift: int) -> np.ndarray:
        """the unfiltered step path of the final DTW with `shift` -> int64 [2][n], increasing"""
        ts = self._pair(0, cover, origin)
        N1, N2 = int(ts[0].shape[1]), int(ts[2].shape[1])
        buf, n = np.zeros((N1 + N2, 2), np.int32), C.c_longlong()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(self._lib.etd_dtw_debug_path(self.h, ptrs(ts), N1, N2, int(shift), buf.ctypes.data, N1 + N2, C.byref(n)), "etd_dtw_debug_path")
        return buf[: n.value][::-1].T.astype(np.int64)

    def debug_total(self, cover: Feats, origin: Feats, shift: int) -> float:
        ts = self._pair(0, cover, origin)
        tot = C.c_double()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(self._lib.etd_dtw_debug_total(self.h, ptrs(ts), int(ts[0].shape[1]), int(ts[2].shape[1]), int(shift), C.byref(tot)), "etd_dtw_debug_total")
        return tot.value


_engines: Dict[str, DTWEngine] = {}


def default_engine(device="cuda") -> DTWEngine:
    """The engine of the reference's parameters (aligner.py:43, 106-121) on `device`, made once."""
    key = str(torch.device(device))
    if key not in _engines:
        _engines[key] = DTWEngine(device)
    return _engines[key]


def align_features_many(pairs: Sequence[Tuple[Feats, Feats]], device="cuda") -> List[Dict]:
    """_compute_warping_path behind the features for a batch: ONE ragged call.  pairs: ((cover chroma, cover DLNCO), (origin chroma, origin DLNCO)), numpy arrays or
    device tensors, [12][N] each.  Shape, finiteness and chroma >= 0 are checked before anything is launched."""
    return default_engine(device).align_many(pairs)


def align_features(cover_feats: Feats, origin_feats: Feats, device="cuda") -> Dict:
    return align_features_many([(cover_feats, origin_feats)], device)[0]


def align_audio_many(pairs_of_wavs: Sequence[Tuple], tuning_offsets: Union[None, str, Sequence[Tuple[float, float]]] = None, device="cuda", features=None) -> List[Dict]:
    """From audio: pairs of (cover samples, origin samples), mono at 22 050 Hz (arrays or tensors) -> the result dicts of ``align_features_many``.  The features of
    both sides of every pair come from ONE ``AlignFeatures.features_many`` call (csrc/alignfeat.hip), then one ragged DTW call.  tuning_offsets: per pair
    (cover cents, origin cents), default 0; ``"estimate"`` estimates every side's on the device first (``etude_amd.tuning``, DESIGN.md 4g: the reference's two
    ``estimate_tuning`` calls; every side then needs N >= 32 768).  features: an ``AlignFeatures`` to use (default: one per device, made once)."""
    if len(pairs_of_wavs) == 0:
        return []
    if tuning_offsets is not None and not isinstance(tuning_offsets, str) and len(tuning_offsets) != len(pairs_of_wavs):
        raise ValueError(f"align_audio_many: {len(pairs_of_wavs)} pairs but {len(tuning_offsets)} tuning offset pairs")
    if features is None:
        from .alignfeat import default_align_features
        features = default_align_features(device)
    wavs = [w for pair in pairs_of_wavs for w in pair]
    if len(wavs) != 2 * len(pairs_of_wavs):
        raise ValueError("align_audio_many: every pair is (cover samples, origin samples)")
    tun = tuning_offsets if tuning_offsets is None or isinstance(tuning_offsets, str) else [float(t) for pair in tuning_offsets for t in pair]
    feats = features.features_many(wavs, tun)
    return align_features_many([(feats[2 * i], feats[2 * i + 1]) for i in range(len(pairs_of_wavs))], device)


def align_files_many(pairs_of_paths: Sequence[Tuple], loader=None, tuning: Union[None, str, Sequence[Tuple[float, float]]] = "estimate", device="cuda",
                     features=None) -> List[Dict]:
    """From files: pairs of (cover WAV, origin WAV) of any rate and channel count -> the result dicts of ``align_audio_many``.  Every file is loaded on the device as
    mono 22 050 Hz (``etude_amd.audio``; one launch per source rate); loader: an ``AudioLoader`` (default: one per device, made once); tuning: the
    ``tuning_offsets`` of ``align_audio_many``, by default estimated as the reference does."""
    from .alignfeat import FS
    if loader is None:
        from .audio import default_audio_loader
        loader = default_audio_loader(device)
    paths = [p for pair in pairs_of_paths for p in pair]
    if len(paths) != 2 * len(pairs_of_paths):
        raise ValueError("align_files_many: every pair is (cover path, origin path)")
    wavs = loader.load_many(paths, FS, mono=True)
    return align_audio_many([(wavs[2 * i], wavs[2 * i + 1]) for i in range(len(pairs_of_paths))], tuning, device, features)


def align_notes_many(pairs: Sequence[Tuple], tuning_offsets: Optional[Sequence[Tuple[float, float]]] = None, device="cuda", renderer=None, features=None) -> List[Dict]:
    """From notes: pairs of (cover notes, origin) -> the result dicts of ``align_features_many``.  Cover notes: whatever ``NoteRenderer.render_many`` takes (a
    NOTE_DTYPE array, a list of note dicts, a ``.json`` / ``.mid`` path); origin: mono samples at 22 050 Hz, or its features (quantised chroma, DLNCO) computed
    before.  The covers are rendered on the device (csrc/render.hip) sub-batch after sub-batch under the renderer's budget, each sub-batch's samples go
    straight into ``AlignFeatures.features_many`` (with the origins given as samples in the first one: ONE call when the covers fit one sub-batch) and are dropped,
    then one ragged DTW call.  tuning_offsets: per pair (cover cents, origin cents), default 0: the cover is rendered AND analysed at its offset; the origin's
    applies when it is given as samples."""
    n = len(pairs)
    if n == 0:
        return []
    if tuning_offsets is not None and len(tuning_offsets) != n:
        raise ValueError(f"align_notes_many: {n} pairs but {len(tuning_offsets)} tuning offset pairs")
    from .alignfeat import FS, default_align_features
    from .render import default_note_renderer
    renderer = renderer or default_note_renderer(device)
    features = features or default_align_features(device)
    if renderer.sample_rate != FS:
        raise ValueError(f"align_notes_many: the renderer runs at {renderer.sample_rate} Hz, the alignment features need {FS}")
    for i, pr in enumerate(pairs):
        if len(pr) != 2:
            raise ValueError(f"pair {i}: need (cover notes, origin)")
    tun = [(0.0, 0.0)] * n if tuning_offsets is None else [(float(a), float(b)) for a, b in tuning_offsets]
    packed = renderer.pack([c for c, _ in pairs], [t[0] for t in tun])
    for i, N in enumerate(packed.num_samples):
        if N < 1:
            raise ValueError(f"pair {i}: the cover has no notes")
    as_audio = [i for i, (_, o) in enumerate(pairs) if not (isinstance(o, (tuple, list)) and len(o) == 2)]
    origin_feats: Dict[int, Feats] = {i: tuple(o) for i, (_, o) in enumerate(pairs) if i not in set(as_audio)}
    cover_feats: Dict[int, Feats] = {}
    first = True
    for idx, samples in renderer.iter_rendered(packed):
        extra = as_audio if first else []
        feats = features.features_many(list(samples) + [pairs[i][1] for i in extra], [tun[i][0] for i in idx] + [tun[i][1] for i in extra])
        cover_feats.update(zip(idx, feats[:len(idx)]))
        origin_feats.update(zip(extra, feats[len(idx):]))
        first = False
        del samples
    return align_features_many([(cover_feats[i], origin_feats[i]) for i in range(n)], device)


class AudioAligner:
    """etude.data.aligner.AudioAligner: same attributes, same cache-first ``align`` and the same rich ``wp.json`` format.  ``feature_fn(path) -> (quantized chroma,
    DLNCO)`` supplies what the reference's ``_get_features`` computes; without it a cache miss is a logged None."""

    def __init__(self, fs: int = 22050, feature_rate: int = 50, feature_fn: Optional[Callable] = None, device="cuda"):
        self.fs = fs
        self.feature_rate = feature_rate
        self.feature_fn = feature_fn
        self.device = device
        self.step_weights = np.array([1.5, 1.5, 2.0])
        self.threshold_rec = 10 ** 6                       # (the reference's multi-resolution threshold; the exact DTW here has no use for it)
        self.win_len_smooth = np.array([101, 51, 21, 1])   # (likewise)

    def align(self, origin_audio_path, cover_audio_path, song_dir) -> Optional[Dict]:
        version_key = Path(cover_audio_path).stem
        cached = self._load_from_cache(song_dir, version_key)
        if cached:
            return cached
        if self.feature_fn is None:
            log.warning("no valid cache for '%s' and no feature_fn: the pitch / onset feature extraction is the caller's", version_key)
            return None
        if not Path(origin_audio_path).exists() or not Path(cover_audio_path).exists():
            return None
        try:
            origin = self.feature_fn(origin_audio_path)
            cover = self.feature_fn(cover_audio_path)
        except Exception as e:      # noqa: BLE001  (the reference's "failed to load" branch)
            log.warning("failed to compute features for alignment: %s", e)
            return None
        result = align_features(cover, origin, self.device)
        self._save_to_cache(song_dir, version_key, result)
        return result

    def align_features_many(self, pairs: Sequence[Tuple[Feats, Feats]]) -> List[Dict]:
        return align_features_many(pairs, self.device)

    def align_audio_many(self, pairs_of_wavs: Sequence[Tuple], tuning_offsets: Union[None, str, Sequence[Tuple[float, float]]] = None, features=None) -> List[Dict]:
        return align_audio_many(pairs_of_wavs, tuning_offsets, self.device, features)

    def _load_from_cache(self, song_dir, version_key: str) -> Optional[Dict]:
        path = Path(song_dir) / "wp.json"
        if not path.exists():
            return None
        try:
            with open(path, "r", encoding="utf-8") as f:
                everything = json.load(f)
            entry = everything.get(version_key)
            if isinstance(entry, dict) and all(k in entry for k in ("wp", "num_frames_cover", "num_frames_origin")):
                entry["wp"] = np.array(entry["wp"], dtype=int)
                entry.setdefault("pitch_shift", 0)
                return entry
            return None
        except (json.JSONDecodeError, KeyError, TypeError):
            return None

    def _save_to_cache(self, song_dir, version_key: str, result_data: Dict):
        path = Path(song_dir) / "wp.json"
        everything = {}
        if path.exists():
            try:
                with open(path, "r", encoding="utf-8") as f:
                    everything = json.load(f)
            except json.JSONDecodeError:
                pass
        entry = dict(result_data)
        entry["wp"] = result_data["wp"].tolist()
        everything[version_key] = entry
        with open(path, "w", encoding="utf-8") as f:
            json.dump(everything, f, indent=4)


def filter_and_weakly_align(align_results: Sequence[Optional[Dict]], downbeats_list: Sequence[Sequence[float]], notes_list: Sequence[List[Dict]],
                            wp_std_threshold: float, names: Optional[Sequence[str]] = None, feature_rate: int = 50) -> Tuple[List[Optional[List[Dict]]], List[Dict]]:
    """The host half of stage 3 (prepare.py:229-248) for songs already aligned.  -> (per song the aligned notes `cover.json` would hold, or None when the song is
    skipped or filtered; the entries `metadata.json` would hold)."""
    from .preprocess import compute_wp_std, create_time_map_from_downbeats, weakly_align
    outputs, metadata = [], []
    for i, res in enumerate(align_results):
        name = names[i] if names is not None else str(i)
        if not res:
            outputs.append(None)
            continue
        time_map = create_time_map_from_downbeats(downbeats_list[i], res, feature_rate)
        wp_std = compute_wp_std(time_map)
        if wp_std > wp_std_threshold:
            outputs.append(None)
            continue
        outputs.append(weakly_align(notes_list[i], time_map))
        metadata.append({"dir_name": name, "status": "kept", "wp_std": wp_std})
    return outputs, metadata


def align_and_filter_many(aligner: AudioAligner, pairs: Sequence[Tuple[Feats, Feats]], downbeats_list: Sequence[Sequence[float]], notes_list: Sequence[List[Dict]],
                          wp_std_threshold: float, names: Optional[Sequence[str]] = None) -> Tuple[List[Optional[List[Dict]]], List[Dict]]:
    """Stage 3 for a batch (prepare.py:222-248): one ragged DTW call, then per song the time map from the origin's downbeats, the WP-Std filter and the weak alignment
    of the cover's transcription.  pairs as for ``align_features_many``."""
    if not (len(pairs) == len(downbeats_list) == len(notes_list)):
        raise ValueError("align_and_filter_many: pairs, downbeats_list and notes_list differ in length")
    results = aligner.align_features_many(pairs)
    return filter_and_weakly_align(results, downbeats_list, notes_list, wp_std_threshold, names, aligner.feature_rate)


def align_and_filter_audio_many(aligner: AudioAligner, pairs_of_wavs: Sequence[Tuple], downbeats_list: Sequence[Sequence[float]], notes_list: Sequence[List[Dict]],
                                wp_std_threshold: float, names: Optional[Sequence[str]] = None, tuning_offsets: Union[None, str, Sequence[Tuple[float, float]]] = None,
                                features=None) -> Tuple[List[Optional[List[Dict]]], List[Dict]]:
    """``align_and_filter_many`` from audio: pairs of (cover samples, origin samples) and tuning_offsets (``"estimate"`` included) as for ``align_audio_many``."""
    if not (len(pairs_of_wavs) == len(downbeats_list) == len(notes_list)):
        raise ValueError("align_and_filter_audio_many: pairs_of_wavs, downbeats_list and notes_list differ in length")
    results = aligner.align_audio_many(pairs_of_wavs, tuning_offsets, features)
    return filter_and_weakly_align(results, downbeats_list, notes_list, wp_std_threshold, names, aligner.feature_rate)
