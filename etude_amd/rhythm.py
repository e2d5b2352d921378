"""Rhythm metrics on the MI355X: ``RhythmMetrics`` -- note onsets of a batch of covers -> Rhythmic Grid Consistency (``rgc_score``, ``inferred_tau``) and IOI Pattern
Entropy (``ipe_score``), the two metrics of the reference's evaluation that need a note list and no audio.

Stands in for ``RGCCalculator`` / ``IPECalculator`` (etude/evaluation/metrics/rgc.py, ipe.py) and the scikit-learn ``KMeans`` the second one fits per file: one launch
for the whole ragged batch, one workgroup per cover, exact fp64 in a fixed order (csrc/rhythm.hip).  DESIGN.md 4h is the contract; tests/rhythm_np.py restates it in
fp64 numpy.  scikit-learn is not a dependency: the 29 random numbers ``KMeans(random_state=42)`` draws do not depend on the data and are formed here with numpy.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine

RGC_ERRORS = {1: "Not enough onsets for IOI calculation.", 2: "Not enough IOIs to analyze.", 3: "Not enough unique IOIs to determine a grid.",
              4: "Could not infer a valid rhythmic grid period (tau)."}
IPE_ERRORS = {1: "Not enough onsets for IOI calculation.", 2: "Could not extract a valid IOI sequence after processing.", 3: "Could not quantize IOI sequence into symbols."}
N_RANDOM = 29


def limits() -> dict:
    """Host only: the constants of the built library"""
    v = [C.c_int() for _ in range(4)]
    _lib.check(_lib.lib().etd_rhythm_limits(*[C.byref(x) for x in v]), "etd_rhythm_limits")
    return dict(zip(("max_onsets", "max_covers", "max_top_k", "max_n_gram"), [x.value for x in v]))


class RhythmMetrics(Engine):
    """Onset lists -> the reference's two result dicts merged.  A cover is any sequence of onsets in seconds (``np.unique`` sorts and de-duplicates it, as
    ``get_onsets_from_file`` does), at most 8 192 distinct ones.  Constructing needs no GPU; ``metrics_many`` does: there is no CPU path."""
    _destroy = "etd_rhythm_destroy"

    def __init__(self, top_k: int = 8, precision_digits: int = 4, n_gram: int = 8, n_clusters: int = 8, min_ioi: float = 0.0625, max_ioi: float = 4.0,
                 device: Union[str, torch.device] = "cuda"):
        self.device = torch.device("cuda" if device == "auto" else device)
        self._lib = _lib.lib()
        self.limits = limits()
        self.params = dict(top_k=int(top_k), precision_digits=int(precision_digits), n_gram=int(n_gram), n_clusters=int(n_clusters), min_ioi=float(min_ioi),
                           max_ioi=float(max_ioi))
        self.random = np.ascontiguousarray(np.random.RandomState(42).random_sample(N_RANDOM))      # data-independent: the first centre, then the local trials
        cfg = _lib.RhythmCfg(n_random=N_RANDOM, random_host=self.random.ctypes.data_as(C.POINTER(C.c_double)), **self.params)
        h = C.c_void_p()
        _lib.check(self._lib.etd_rhythm_create(C.byref(cfg), C.byref(h)), "etd_rhythm_create")
        self._adopt(h)
        self._tap = None

    def pack(self, onsets_list: Sequence) -> Tuple[np.ndarray, np.ndarray]:
        """host: every cover through ``np.unique`` -> (one int64 buffer holding the offsets [B + 1] and, behind them, the onsets' fp64 bits; the offsets).  Checks that
        the onsets are finite and that no rounded IOI leaves the sort key; the per-cover limit is the library's check (``check_offsets``)."""
        covers = []
        for i, x in enumerate(onsets_list):
            u = np.unique(np.asarray(x, np.float64).reshape(-1)) if len(x) else np.zeros(0)
            if u.size and not np.isfinite(u).all():
                raise ValueError(f"cover {i}: holds a non-finite onset")
            if u.size > 1 and float(u[-1] - u[0]) * 10.0 ** self.params["precision_digits"] >= 2.0 ** 50:
                raise ValueError(f"cover {i}: spans {float(u[-1] - u[0])} s, too long to count IOIs rounded to {self.params['precision_digits']} digits")
            covers.append(u)
        offsets = np.zeros(len(covers) + 1, np.int64)
        np.cumsum([len(u) for u in covers], out=offsets[1:])
        packed = np.empty(len(offsets) + int(offsets[-1]), np.int64)
        packed[:len(offsets)] = offsets
        if covers:
            packed[len(offsets):] = np.concatenate(covers + [np.zeros(0)]).view(np.int64)
        return packed, offsets

    def check_offsets(self, offsets: np.ndarray) -> None:
        """host only: the library's refusal of a call (a cover above the limit, too many covers), before anything touches the device"""
        off = np.ascontiguousarray(offsets, np.int64)
        _lib.check(self._lib.etd_rhythm_check(self.h, off.ctypes.data_as(_lib.c_i64_p), len(off) - 1), "etd_rhythm_check")

    def tap(self, on: bool) -> None:
        """test hook: the following ``run_packed`` calls also return what the device clustered (``last_tap``: centred log-IOIs, labels, centres)"""
        self._tap = {} if on else None
        if not on:
            _lib.check(self._lib.etd_rhythm_debug_logioi(self.h, None, None, None), "etd_rhythm_debug_logioi")

    def run_packed(self, packed: np.ndarray, offsets: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """one copy to the device, one launch, the results back: (out float64 [B][3] = rgc_score, inferred_tau, ipe_score; status int32 [B])"""
        B = len(offsets) - 1
        self.check_offsets(offsets)
        dev = self._device()
        with torch.cuda.device(dev):
            buf = torch.from_numpy(packed).to(dev)
            out = torch.empty(B, 3, dtype=torch.float64, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            base = buf.data_ptr()
            tap = None
            if self._tap is not None:
                total = max(int(offsets[-1]), 1)
                tap = (torch.full((total,), float("nan"), dtype=torch.float64, device=dev), torch.full((total,), -1, dtype=torch.int8, device=dev),
                       torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev))
                _lib.check(self._lib.etd_rhythm_debug_logioi(self.h, *[C.c_void_p(t.data_ptr()) for t in tap]), "etd_rhythm_debug_logioi")
            off = np.ascontiguousarray(offsets, np.int64)
            _lib.check(self._lib.etd_rhythm_run(self.h, C.c_void_p(base + 8 * (B + 1)), C.c_void_p(base), off.ctypes.data_as(_lib.c_i64_p), B,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), self._stream(dev)), "etd_rhythm_run")
            res = out.cpu().numpy(), status.cpu().numpy()
            if tap is not None:
                self._tap = dict(logioi=tap[0].cpu().numpy(), labels=tap[1].cpu().numpy(), centres=tap[2].cpu().numpy())
        return res

    @property
    def last_tap(self) -> Optional[dict]:
        return self._tap

    def raw_many(self, onsets_list: Sequence) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (out [B][3], status [B], offsets [B + 1] of the packed covers); calls above the library's covers-per-call limit are split"""
        packed, offsets = self.pack(onsets_list)
        B, cap = len(offsets) - 1, self.limits["max_covers"]
        if B == 0:
            return np.zeros((0, 3)), np.zeros(0, np.int32), offsets
        if B <= cap:
            out, status = self.run_packed(packed, offsets)
            return out, status, offsets
        self.check_offsets(offsets[:cap + 1])
        outs, stats = [], []
        for b0 in range(0, B, cap):
            o, s, _ = self.raw_many(onsets_list[b0:b0 + cap])
            outs.append(o); stats.append(s)
        return np.concatenate(outs), np.concatenate(stats), offsets

    def metrics_many(self, onsets_list: Sequence, details: bool = False) -> List[Dict]:
        """covers -> per cover ``{"rgc_score", "inferred_tau", "ipe_score"}``; where a metric fails its keys give way to ``rgc_error`` / ``ipe_error`` with the
        reference's message.  ``details`` adds ``relocated`` (Lloyd's iteration met an empty cluster: DESIGN.md 4h), ``n_clusters`` and ``iterations``.  A cover's
        numbers depend on its onsets alone: bit-identical alone, in any batch and from run to run."""
        out, status, _ = self.raw_many(onsets_list)
        rows = []
        for b in range(len(status)):
            st = int(status[b])
            rgc, ipe = st & 15, (st >> 4) & 15
            if rgc == 5 or ipe == 5:
                raise _lib.EtudeHipError(f"etd_rhythm_run: cover {b}: the device refused the onsets (status {st:#x})")
            row: Dict = {}
            if rgc == 0:
                row["rgc_score"], row["inferred_tau"] = float(out[b, 0]), float(out[b, 1])
            else:
                row["rgc_error"] = RGC_ERRORS[rgc]
            if ipe == 0:
                row["ipe_score"] = float(out[b, 2])
            else:
                row["ipe_error"] = IPE_ERRORS[ipe]
            if details:
                row.update(relocated=bool((st >> 8) & 1), n_clusters=(st >> 12) & 15, iterations=(st >> 16) & 511)
            rows.append(row)
        return rows


_default: Dict[tuple, RhythmMetrics] = {}


def default_rhythm_metrics(device="cuda", **params) -> RhythmMetrics:
    """one ``RhythmMetrics`` per device and parameter set, made once"""
    key = (str(torch.device(device)),) + tuple(sorted(params.items()))
    if key not in _default:
        _default[key] = RhythmMetrics(device=device, **params)
    return _default[key]


def rhythm_metrics_for_notes(notes_lists: Sequence[Sequence[Dict]], device="cuda", **params) -> List[Dict]:
    """the note dicts ``TinyREMITokenizer.decode_to_notes`` returns, one list per cover (a ``generate_many`` batch) -> ``metrics_many`` of their onsets: one call"""
    return default_rhythm_metrics(device, **params).metrics_many([[float(n["onset"]) for n in notes] for notes in notes_lists])


# ---------------------------------------------------------------------------------------------------------------- files
def _varlen(d: bytes, p: int) -> Tuple[int, int]:
    v = 0
    while True:
        b = d[p]
        p += 1
        v = (v << 7) | (b & 0x7F)
        if not b & 0x80:
            return v, p


def read_midi_onsets(path) -> np.ndarray:
    """A small standard-MIDI-file reader of this project's own, for what the metrics need: the start times in seconds of every note-on with velocity > 0 outside
    channel 10 (the drums), in file order.  Formats 0 and 1, ticks per beat (an SMPTE division is refused), the tempo map of all tracks, running status."""
    d = Path(path).read_bytes()
    if d[:4] != b"MThd" or int.from_bytes(d[4:8], "big") < 6:
        raise ValueError(f"{path}: not a standard MIDI file")
    fmt, ntrk, div = (int.from_bytes(d[8 + 2 * i:10 + 2 * i], "big") for i in range(3))
    if fmt > 1 or div & 0x8000 or div == 0:
        raise ValueError(f"{path}: format {fmt} / division {div:#x} is not supported (formats 0 and 1, ticks per beat)")
    p = 8 + int.from_bytes(d[4:8], "big")
    tempi, ons = [], []
    for _ in range(ntrk):
        if d[p:p + 4] != b"MTrk":
            raise ValueError(f"{path}: track header expected at byte {p}")
        end = p + 8 + int.from_bytes(d[p + 4:p + 8], "big")
        p += 8
        tick, running = 0, 0
        while p < end:
            dt, p = _varlen(d, p)
            tick += dt
            b = d[p]
            if b == 0xFF:
                kind = d[p + 1]
                ln, p = _varlen(d, p + 2)
                if kind == 0x51 and ln == 3:
                    tempi.append((tick, int.from_bytes(d[p:p + 3], "big")))
                p += ln
            elif b in (0xF0, 0xF7):
                ln, p = _varlen(d, p + 1)
                p += ln
            else:
                if b & 0x80:
                    running, p = b, p + 1
                kind, ch = running & 0xF0, running & 0x0F
                n_data = 1 if kind in (0xC0, 0xD0) else 2
                if kind == 0x90 and d[p + 1] > 0 and ch != 9:
                    ons.append(tick)
                p += n_data
        p = end
    # the tempo map: seconds at every change, 500 000 us per beat until the first
    tempi.sort(key=lambda x: x[0])
    ticks, secs, scales = [0], [0.0], [500000 * 1e-6 / div]
    for tk, us in tempi:
        if tk == ticks[-1]:
            scales[-1] = us * 1e-6 / div
        else:
            secs.append(secs[-1] + (tk - ticks[-1]) * scales[-1]); ticks.append(tk); scales.append(us * 1e-6 / div)
    ons = np.asarray(ons, np.int64)
    seg = np.searchsorted(np.asarray(ticks), ons, side="right") - 1
    return np.asarray(secs)[seg] + (ons - np.asarray(ticks)[seg]) * np.asarray(scales)[seg] if ons.size else np.zeros(0)


def read_midi_notes(path) -> np.ndarray:
    """The notes of a standard MIDI file as a NOTE_DTYPE array (onset, offset in seconds, pitch, velocity), for ``etude_amd.render``: every note-on with velocity > 0
    outside channel 10 (the drums) paired with the next note-off -- or note-on with velocity 0 -- of its channel and key (overlapping notes of one key end first in,
    first out; a note the file never ends stops at the file's last event), in the order of their onsets, ties in file order.  The parser, the supported files and the
    tempo map are ``read_midi_onsets``'s."""
    d = Path(path).read_bytes()
    if d[:4] != b"MThd" or int.from_bytes(d[4:8], "big") < 6:
        raise ValueError(f"{path}: not a standard MIDI file")
    fmt, ntrk, div = (int.from_bytes(d[8 + 2 * i:10 + 2 * i], "big") for i in range(3))
    if fmt > 1 or div & 0x8000 or div == 0:
        raise ValueError(f"{path}: format {fmt} / division {div:#x} is not supported (formats 0 and 1, ticks per beat)")
    p = 8 + int.from_bytes(d[4:8], "big")
    tempi, notes, last_tick = [], [], 0
    for _ in range(ntrk):
        if d[p:p + 4] != b"MTrk":
            raise ValueError(f"{path}: track header expected at byte {p}")
        end = p + 8 + int.from_bytes(d[p + 4:p + 8], "big")
        p += 8
        tick, running = 0, 0
        sounding: Dict[Tuple[int, int], List[int]] = {}      # (channel, key) -> indices into notes, oldest first
        while p < end:
            dt, p = _varlen(d, p)
            tick += dt
            b = d[p]
            if b == 0xFF:
                kind = d[p + 1]
                ln, p = _varlen(d, p + 2)
                if kind == 0x51 and ln == 3:
                    tempi.append((tick, int.from_bytes(d[p:p + 3], "big")))
                p += ln
            elif b in (0xF0, 0xF7):
                ln, p = _varlen(d, p + 1)
                p += ln
            else:
                if b & 0x80:
                    running, p = b, p + 1
                kind, ch = running & 0xF0, running & 0x0F
                n_data = 1 if kind in (0xC0, 0xD0) else 2
                if ch != 9 and kind == 0x90 and d[p + 1] > 0:
                    sounding.setdefault((ch, d[p]), []).append(len(notes))
                    notes.append([tick, -1, d[p], d[p + 1]])
                elif ch != 9 and kind in (0x80, 0x90) and sounding.get((ch, d[p])):
                    notes[sounding[(ch, d[p])].pop(0)][1] = tick
                p += n_data
        last_tick = max(last_tick, tick)
        p = end
    tempi.sort(key=lambda x: x[0])
    ticks, secs, scales = [0], [0.0], [500000 * 1e-6 / div]
    for tk, us in tempi:
        if tk == ticks[-1]:
            scales[-1] = us * 1e-6 / div
        else:
            secs.append(secs[-1] + (tk - ticks[-1]) * scales[-1]); ticks.append(tk); scales.append(us * 1e-6 / div)
    from .render import NOTE_DTYPE
    out = np.zeros(len(notes), NOTE_DTYPE)
    if notes:
        a = np.asarray(notes, np.int64)
        a[:, 1] = np.where(a[:, 1] < 0, last_tick, a[:, 1])

        def seconds(t):
            seg = np.searchsorted(np.asarray(ticks), t, side="right") - 1
            return np.asarray(secs)[seg] + (t - np.asarray(ticks)[seg]) * np.asarray(scales)[seg]
        out["onset"], out["offset"], out["pitch"], out["velocity"] = seconds(a[:, 0]), seconds(a[:, 1]), a[:, 2], a[:, 3]
        out = out[np.argsort(a[:, 0], kind="stable")]
    return out


def get_onsets_from_file(file_path) -> np.ndarray:
    """``get_onsets_from_file`` of the reference (etude/evaluation/metrics/base_metric.py): the sorted, unique note onsets of a ``.mid`` or ``.json`` file; an empty
    array for a missing or unreadable file and below two notes."""
    file_path = Path(file_path)
    onsets: Sequence = []
    if not file_path.exists():
        return np.array([])
    try:
        if file_path.suffix.lower() == ".mid":
            onsets = read_midi_onsets(file_path)
        elif file_path.suffix.lower() == ".json":
            with open(file_path, "r", encoding="utf-8") as f:
                notes = json.load(f)
            if notes:
                onsets = [note["onset"] for note in notes]
        if len(onsets) < 2:
            return np.array([])
        return np.unique(onsets)
    except Exception:      # noqa: BLE001  (as the reference)
        return np.array([])


class RGCCalculator:
    """``RGCCalculator`` of the reference: ``calculate(file_path)`` -> ``{"rgc_score", "inferred_tau"}`` or ``{"error"}``"""

    def __init__(self, top_k: int = 8, precision_digits: int = 4, device="cuda", **kwargs):
        self.top_k, self.precision_digits, self.device = top_k, precision_digits, device

    def calculate_many(self, file_paths: Sequence) -> List[Dict]:
        eng = default_rhythm_metrics(self.device, top_k=self.top_k, precision_digits=self.precision_digits)
        rows = eng.metrics_many([get_onsets_from_file(p) for p in file_paths])
        return [{"error": r["rgc_error"]} if "rgc_error" in r else {"rgc_score": r["rgc_score"], "inferred_tau": r["inferred_tau"]} for r in rows]

    def calculate(self, file_path) -> Dict:
        return self.calculate_many([file_path])[0]


class IPECalculator:
    """``IPECalculator`` of the reference: ``calculate(file_path)`` -> ``{"ipe_score"}`` or ``{"error"}``"""

    def __init__(self, n_gram: int = 8, n_clusters: int = 8, min_ioi: float = 0.0625, max_ioi: float = 4.0, device="cuda", **kwargs):
        self.n_gram, self.n_clusters, self.min_ioi, self.max_ioi, self.device = n_gram, n_clusters, min_ioi, max_ioi, device

    def calculate_many(self, file_paths: Sequence) -> List[Dict]:
        eng = default_rhythm_metrics(self.device, n_gram=self.n_gram, n_clusters=self.n_clusters, min_ioi=self.min_ioi, max_ioi=self.max_ioi)
        rows = eng.metrics_many([get_onsets_from_file(p) for p in file_paths])
        return [{"error": r["ipe_error"]} if "ipe_error" in r else {"ipe_score": r["ipe_score"]} for r in rows]

    def calculate(self, file_path) -> Dict:
        return self.calculate_many([file_path])[0]


def _align_rendered(eval_dir: Path, keys: Sequence[Tuple[str, str]], results: List[Optional[Dict]], renderer, device, loader=None) -> List[Optional[Dict]]:
    """``evaluate_many(renderer=...)``: the alignment results with those of the covers that exist as notes only filled in.  Every origin's features are computed
    once, whatever the number of its versions.  loader: an ``AudioLoader``; with one the origins are loaded on the device as mono 22 050 Hz, whatever their own
    rate and channel count."""
    from .aligner import align_notes_many
    from .alignfeat import FS, default_align_features
    from .extractor import read_wav
    if renderer.sample_rate != FS:
        raise ValueError(f"evaluate_many: the renderer runs at {renderer.sample_rate} Hz, the alignment features need {FS}")
    todo = []
    for i, (d, v) in enumerate(keys):
        if results[i] is not None or (eval_dir / d / f"{v}.wav").exists() or not (eval_dir / d / "origin.wav").exists():
            continue
        mid, js = eval_dir / d / f"{v}.mid", eval_dir / d / f"{v}.json"
        if mid.exists() or js.exists():
            todo.append((i, d, mid if mid.exists() else js))
    if not todo:
        return results
    songs = sorted({d for _, d, _ in todo})
    if loader is not None:
        wavs = loader.load_many([eval_dir / d / "origin.wav" for d in songs], FS, mono=True)
    else:
        wavs = []
        for d in songs:
            x, sr = read_wav(eval_dir / d / "origin.wav")
            if sr != FS or x.shape[0] != 1:
                raise ValueError(f"{eval_dir / d / 'origin.wav'}: {x.shape[0]} channel(s) at {sr} Hz; a rendered cover is aligned to a mono origin at {FS} Hz "
                                 f"(resample it first: FrontEnd(sr_in, {FS}).resample)")
            wavs.append(x[0])
    features = default_align_features(device)
    origin = dict(zip(songs, features.features_many(wavs)))
    out = list(results)
    for (i, _, _), res in zip(todo, align_notes_many([(f, origin[d]) for _, d, f in todo], device=device, renderer=renderer, features=features)):
        out[i] = res
    return out


def evaluate_many(eval_dir, metadata: Sequence[Dict], versions: Sequence[str], metrics: Sequence[str] = ("wpd", "rgc", "ipe"), aligner=None, device="cuda",
                  wpd_subsample_step: int = 1, wpd_trim_seconds: float = 0, renderer=None, loader=None, **rhythm_params) -> List[Dict]:
    """``EvaluationRunner.run`` of the reference (etude/evaluation/runner.py) -> its rows as dicts: ``song``, ``version``, then ``wpd_score``, ``rgc_score``,
    ``inferred_tau``, ``ipe_score`` where the metric succeeded; a row with no metric is dropped.  metadata: the loaded metadata list (``dir_name`` per song).  WPD
    goes through ``AudioAligner.align`` and ``wpd_many`` as they stand; RGC and IPE of every (song, version) come from ONE device call.

    renderer: a ``NoteRenderer`` (22 050 Hz).  With one, a (song, version) that ``align`` has no result for, whose ``{version}.wav`` is missing but whose ``.mid`` or
    ``.json`` exists next to an ``origin.wav``, gets its WPD from the cover rendered on the device (``aligner.align_notes_many``; nothing is written to ``wp.json``).
    loader: an ``etude_amd.AudioLoader``.  With one, ``origin.wav`` of any rate and channel count is loaded on the device as mono 22 050 Hz; without
    one it must already be mono at 22 050 Hz."""
    eval_dir = Path(eval_dir)
    keys = [(s["dir_name"], v) for s in metadata if s.get("dir_name") for v in versions]
    rows = [{"song": d, "version": v} for d, v in keys]
    if "wpd" in metrics:
        from .aligner import AudioAligner
        from .evaluation import wpd_many
        aligner = aligner or AudioAligner(device=device)
        results = [aligner.align(eval_dir / d / "origin.wav", eval_dir / d / f"{v}.wav", eval_dir / d) for d, v in keys]
        if renderer is not None:
            results = _align_rendered(eval_dir, keys, results, renderer, device, loader)
        for row, res in zip(rows, wpd_many(results, wpd_subsample_step, wpd_trim_seconds)):
            if "error" not in res:
                row.update(res)
    if "rgc" in metrics or "ipe" in metrics:
        files = []
        for d, v in keys:
            mid, js = eval_dir / d / f"{v}.mid", eval_dir / d / f"{v}.json"
            files.append(mid if mid.exists() else js if js.exists() else None)
        have = [i for i, f in enumerate(files) if f is not None]
        if have:
            res = default_rhythm_metrics(device, **rhythm_params).metrics_many([get_onsets_from_file(files[i]) for i in have])
            for i, r in zip(have, res):
                if "rgc" in metrics and "rgc_error" not in r:
                    rows[i].update(rgc_score=r["rgc_score"], inferred_tau=r["inferred_tau"])
                if "ipe" in metrics and "ipe_error" not in r:
                    rows[i].update(ipe_score=r["ipe_score"])
    return [r for r in rows if len(r) > 2]


def to_dataframe(rows: List[Dict]):
    """the reference's ``pd.DataFrame(results_list)``; needs pandas"""
    import pandas as pd
    return pd.DataFrame(rows)
