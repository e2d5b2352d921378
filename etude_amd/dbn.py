"""DBN beat / downbeat tracking on the MI355X: ``DBNBeatTracker`` / ``DBNDownBeatTracker`` stand in for madmom's DBNBeatTrackingProcessor /
DBNDownBeatTrackingProcessor (what etude.data.beat_detector.BeatDetector.detect calls, beat_detector.py:133-150), without madmom.

The HMMs, the fp64 log-space Viterbi, threshold trimming, peak picking and the choice of the bar length run in libetude_hip.so (csrc/dbn.hip), one
workgroup per (song, HMM) for a ragged batch of songs; only integer beat frames and beat numbers come back, and the times are formed here as frame / fps in float64.
``DBNEngine`` is the shared core: it tracks device-resident activations or logits (``BeatDetector(tracker="native")`` hands it the model's output where it lies).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._engine import Engine, i64, nonneg

IN_ACTIVATIONS, IN_LOGITS, IN_COMBINED = 0, 1, 2          # ETD_DBN_IN_*


def make_cfg(fps: float, min_bpm: float, max_bpm: float, threshold: float = 0.0, beats_per_bar: Sequence[int] = (), num_tempi: Optional[int] = None,
             transition_lambda: float = 100.0, observation_lambda: float = 16.0, correct: bool = True) -> "_lib.DbnCfg":
    bpb = [int(b) for b in (beats_per_bar if isinstance(beats_per_bar, (list, tuple)) else [beats_per_bar])]
    if len(bpb) > 8:
        raise ValueError("at most 8 bar lengths")
    cfg = _lib.DbnCfg(fps=float(fps), min_bpm=float(min_bpm), max_bpm=float(max_bpm), transition_lambda=float(transition_lambda),
                      observation_lambda=float(observation_lambda), threshold=float(threshold or 0.0), correct=1 if correct else 0,
                      num_tempi=int(num_tempi or 0), n_bars=len(bpb))
    for i, b in enumerate(bpb):
        cfg.beats_per_bar[i] = b
    return cfg


def describe(cfg: "_lib.DbnCfg", hmm_index: int, tables: bool = False) -> dict:
    """Host only: intervals, state count and beats of one HMM of a config (0 = the beat HMM); ``tables`` adds the log transitions [from][to] and the pointers."""
    lib = _lib.lib()
    n, S, B = C.c_int(), C.c_int(), C.c_int()
    _lib.check(lib.etd_dbn_describe(C.byref(cfg), hmm_index, None, 0, C.byref(n), C.byref(S), C.byref(B), None, None), "etd_dbn_describe")
    iv = np.zeros(n.value, np.int32)
    lt = np.zeros((n.value, n.value), np.float64) if tables else None
    ptr = np.zeros(S.value, np.uint8) if tables else None
    _lib.check(lib.etd_dbn_describe(C.byref(cfg), hmm_index, iv.ctypes.data, n.value, C.byref(n), C.byref(S), C.byref(B),
                                    lt.ctypes.data if tables else None, ptr.ctypes.data if tables else None), "etd_dbn_describe")
    out = dict(intervals=iv, n_states=S.value, num_beats=B.value)
    if tables:
        out.update(logtrans=lt, pointers=ptr)
    return out


def workspace_bytes(cfg: "_lib.DbnCfg", T: int, hmm_index: int = -1) -> int:
    return nonneg(_lib.lib().etd_dbn_workspace_bytes(C.byref(cfg), int(T), int(hmm_index)), "etd_dbn_workspace_bytes")


class DBNEngine(Engine):
    """One etd_dbn handle: the beat HMM and one bar HMM per entry of ``beats_per_bar``."""
    _destroy = "etd_dbn_destroy"

    def __init__(self, fps: float, min_bpm: float, max_bpm: float, threshold: float = 0.0, beats_per_bar: Sequence[int] = (), device="cuda", **model):
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.EtudeHipError("etude_amd DBN trackers need a ROCm GPU (device='cuda'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.fps = float(fps)
        self.cfg = make_cfg(fps, min_bpm, max_bpm, threshold, beats_per_bar, **model)
        self.beats_per_bar = [self.cfg.beats_per_bar[i] for i in range(self.cfg.n_bars)]
        self._lib = _lib.lib()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.etd_dbn_create(C.byref(self.cfg), C.byref(h)), "etd_dbn_create")
        self._adopt(h)

    def track(self, x: torch.Tensor, Ts: Sequence[int], kind: int = IN_ACTIVATIONS) -> List[Tuple[np.ndarray, np.ndarray, int]]:
        """x: device fp32 [sum T][2], the songs back to back -> per song (beat frames [n] int32, downbeat rows [m][2] int32 of (frame, beat number), index of the
        chosen bar length or -1)"""
        n = len(Ts)
        if n == 0:
            return []
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 2 or x.shape[0] != int(sum(Ts)) or not x.is_contiguous() or x.device != self.device:
            raise ValueError(f"track: need a contiguous fp32 [sum T = {int(sum(Ts))}][2] tensor on {self.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        T_arr = i64(Ts)
        cap_b = cap_d = max(16, int(sum(Ts)) // max(1, int(60.0 * self.fps / self.cfg.max_bpm) - 1) + 2 * n)
        with torch.cuda.device(self.device):
            st = self._stream(self.device)
            while True:
                bf = np.zeros(cap_b, np.int32)
                df, dn = np.zeros(cap_d, np.int32), np.zeros(cap_d, np.int32)
                bo, do = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
                choice = np.zeros(n, np.int32)
                need = (C.c_longlong * 2)()
                rc = self._lib.etd_dbn_track(self.h, C.c_void_p(x.data_ptr()), int(kind), n, T_arr, bf.ctypes.data, cap_b, bo.ctypes.data,
                                             df.ctypes.data, dn.ctypes.data, cap_d, do.ctypes.data, choice.ctypes.data, need, st)
                if rc == -12 and (need[0] > cap_b or need[1] > cap_d):          # ETD_ENOMEM: the contract of etd_mpe2note
                    cap_b, cap_d = max(cap_b, int(need[0])), max(cap_d, int(need[1]))
                    continue
                _lib.check(rc, "etd_dbn_track")
                break
        return [(bf[bo[s]:bo[s + 1]].copy(), np.stack([df[do[s]:do[s + 1]], dn[do[s]:do[s + 1]]], axis=1), int(choice[s])) for s in range(n)]

    def track_arrays(self, acts: Sequence[np.ndarray], kind: int) -> List[Tuple[np.ndarray, np.ndarray, int]]:
        """host [T][2] float arrays -> track (one upload)"""
        arrs = [np.ascontiguousarray(a, np.float32) for a in acts]
        for i, a in enumerate(arrs):
            if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
                raise ValueError(f"song {i}: activations must be [T >= 1][2], got {a.shape}")
        x = torch.from_numpy(np.concatenate(arrs, axis=0)).to(self.device)
        return self.track(x, [len(a) for a in arrs], kind)

    def debug_viterbi(self, hmm_index: int, densities: np.ndarray) -> Tuple[np.ndarray, float]:
        """test hook: the Viterbi kernel alone on fp64 densities [T][K] -> (state path [T], log probability)"""
        d = torch.from_numpy(np.ascontiguousarray(densities, np.float64)).to(self.device)
        path = np.zeros(d.shape[0], np.int32)
        lp = C.c_double()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _lib.check(self._lib.etd_dbn_debug_viterbi(self.h, int(hmm_index), C.c_void_p(d.data_ptr()), d.shape[0], path.ctypes.data, C.byref(lp)),
                       "etd_dbn_debug_viterbi")
        return path, lp.value


class DBNBeatTracker:
    """madmom.features.beats.DBNBeatTrackingProcessor: callable on a 1-D activation array -> beat times [n] in seconds (float64)."""

    def __init__(self, min_bpm: float = 55.0, max_bpm: float = 215.0, fps: Optional[float] = None, threshold: float = 0.0, num_tempi: Optional[int] = None,
                 transition_lambda: float = 100.0, observation_lambda: float = 16.0, correct: bool = True, device="cuda"):
        if fps is None:
            raise ValueError("DBNBeatTracker: fps is required")
        self.fps = float(fps)
        self.engine = DBNEngine(fps, min_bpm, max_bpm, threshold, (), device, num_tempi=num_tempi, transition_lambda=transition_lambda,
                                observation_lambda=observation_lambda, correct=correct)

    def track_many(self, activations: Sequence[np.ndarray]) -> List[np.ndarray]:
        acts = []
        for i, a in enumerate(activations):
            a = np.asarray(a, np.float32)
            if a.ndim != 1:
                raise ValueError(f"song {i}: beat activations must be 1-D, got {a.shape}")
            acts.append(np.stack([a, np.zeros_like(a)], axis=1))
        return [b.astype(np.float64) / self.fps for b, _, _ in self.engine.track_arrays(acts, IN_ACTIVATIONS)]

    def __call__(self, activations: np.ndarray) -> np.ndarray:
        if len(activations) == 0:
            return np.zeros(0, np.float64)
        return self.track_many([activations])[0]


class DBNDownBeatTracker:
    """madmom.features.downbeats.DBNDownBeatTrackingProcessor: callable on [T][2] (beat-only, downbeat) activations -> [n][2] of (seconds, beat number)."""

    def __init__(self, beats_per_bar, min_bpm: float = 55.0, max_bpm: float = 215.0, fps: Optional[float] = None, threshold: float = 0.05,
                 num_tempi: Optional[int] = None, transition_lambda: float = 100.0, observation_lambda: float = 16.0, correct: bool = True, device="cuda"):
        if fps is None:
            raise ValueError("DBNDownBeatTracker: fps is required")
        self.fps = float(fps)
        bpb = list(beats_per_bar) if isinstance(beats_per_bar, (list, tuple, np.ndarray)) else [beats_per_bar]
        if not bpb:
            raise ValueError("DBNDownBeatTracker: beats_per_bar is empty")
        self.engine = DBNEngine(fps, min_bpm, max_bpm, threshold, bpb, device, num_tempi=num_tempi, transition_lambda=transition_lambda,
                                observation_lambda=observation_lambda, correct=correct)
        self.beats_per_bar = self.engine.beats_per_bar

    def track_many(self, activations: Sequence[np.ndarray], with_bar: bool = False):
        res = self.engine.track_arrays(activations, IN_COMBINED)
        out = [np.stack([r[:, 0].astype(np.float64) / self.fps, r[:, 1].astype(np.float64)], axis=1) for _, r, _ in res]
        if with_bar:
            return out, [self.beats_per_bar[c] if c >= 0 else None for _, _, c in res]
        return out

    def __call__(self, activations: np.ndarray) -> np.ndarray:
        if len(activations) == 0:
            return np.zeros((0, 2), np.float64)
        return self.track_many([activations])[0]
