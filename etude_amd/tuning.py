"""Tuning estimation on the MI355X: ``TuningEstimator`` -- mono audio at 22 050 Hz -> the deviation from 440 Hz equal temperament in whole cents (-50 .. 49), the
``tuning_offset`` of ``AlignFeatures``' filterbanks.

Stands in for ``estimate_tuning(audio, fs)`` of the reference's ``AudioAligner._compute_alignment`` (etude/data/aligner.py:100-101), modelled on synctoolbox's routine
with its defaults: a long-window STFT (csrc/tuning.hip: a 16 384-point real FFT in LDS per frame, the hot path), log compression, the sum over time in a fixed order,
a not-a-knot cubic spline onto a 1-cent axis, a local average, rectification and a comb.  DESIGN.md 4g is the contract; tests/tuning_np.py restates it in fp64 numpy.
synctoolbox is not a dependency and parity with it is unpinned.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i32, i64, mono_songs_to_device, nonneg, ptrs

FS = 22050
N_FFT = 16384
HOP = 8192
N_THETA = 100


def limits() -> dict:
    """Host only: the constants of the built library"""
    lo, hi, ms = C.c_longlong(), C.c_longlong(), C.c_int()
    _lib.check(_lib.lib().etd_tuning_limits(C.byref(lo), C.byref(hi), C.byref(ms)), "etd_tuning_limits")
    return dict(min_samples=lo.value, max_samples=hi.value, max_songs=ms.value)


class TuningEstimator(Engine):
    """Mono audio at 22 050 Hz -> tuning in cents, an integer in -50 .. 49, and the comb similarity ``sim[100]`` it is the first maximum of.

    A song is a 1-d float32 array or tensor (host or device), finite, 32 768 <= N <= 2^27.  Constructing needs no GPU; ``estimate_many`` does: there is no CPU path."""
    _destroy = "etd_tuning_destroy"

    def __init__(self, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device("cuda" if device == "auto" else device)
        self._lib = _lib.lib()
        self.limits = limits()
        cfg = _lib.TuningCfg(sample_rate=FS, n_fft=N_FFT, hop=HOP)
        h = C.c_void_p()
        _lib.check(self._lib.etd_tuning_create(C.byref(cfg), C.byref(h)), "etd_tuning_create")
        self._adopt(h)

    def num_frames(self, N: int) -> int:
        if N < self.limits["min_samples"]:
            raise ValueError(f"num_frames: N must be >= {self.limits['min_samples']} (two windows), got {N}")
        return 1 + int(N) // HOP

    def workspace_bytes(self, Ns: Sequence[int]) -> int:
        return nonneg(self._lib.etd_tuning_workspace_bytes(self.h, len(Ns), i64(Ns)), "etd_tuning_workspace_bytes")

    def layout(self, Ns: Sequence[int], song: int) -> dict:
        """test hook (host arithmetic): where song `song` of a call with these lengths keeps its stages in the workspace (byte offsets), its frames and groups"""
        out = (C.c_int64 * len(_lib.TUNING_LAYOUT))()
        _lib.check(self._lib.etd_tuning_debug_layout(self.h, len(Ns), i64(Ns), int(song), out, len(_lib.TUNING_LAYOUT)), "etd_tuning_debug_layout")
        return dict(zip(_lib.TUNING_LAYOUT, [int(v) for v in out]))

    def tap_power(self, song: int, frames: Sequence[int], power: Union[torch.Tensor, None]) -> None:
        """test hook: the following runs also write P[f][0 .. 8192] of these frames (at most 8) of song `song` to `power` (device float32 [len(frames)][8193]);
        ``power=None`` turns it off"""
        if power is None:
            _lib.check(self._lib.etd_tuning_debug_power(self.h, 0, None, 0, None), "etd_tuning_debug_power")
            return
        if power.dtype != torch.float32 or power.numel() < len(frames) * (N_FFT // 2 + 1) or not power.is_contiguous():
            raise ValueError("tap_power: power must be a contiguous float32 tensor of [len(frames)][8193]")
        _lib.check(self._lib.etd_tuning_debug_power(self.h, int(song), i32(frames), len(frames), C.c_void_p(power.data_ptr())), "etd_tuning_debug_power")

    def run_raw(self, songs: Sequence[torch.Tensor], tuning: torch.Tensor, sim: torch.Tensor, ws: torch.Tensor) -> None:
        """one launch sequence on checked device tensors with the caller's buffers (tests put canaries around them): tuning int32 [n], sim float64 [n][100]"""
        n = len(songs)
        dev = self._device()
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_tuning_run(self.h, ptrs(songs), n, i64([t.numel() for t in songs]), C.c_void_p(tuning.data_ptr() if tuning is not None else None),
                                                C.c_void_p(sim.data_ptr() if sim is not None else None), C.c_void_p(ws.data_ptr()), ws.numel() * ws.element_size(),
                                                self._stream(dev)), "etd_tuning_run")

    def check_songs(self, wavs: Sequence) -> List[torch.Tensor]:
        """the input checks (1-d, the length limits, finite with ONE host synchronisation) -> the songs as contiguous float32 device tensors"""
        return mono_songs_to_device(wavs, self._device, self.limits["min_samples"], self.limits["max_samples"],
                                    f"is shorter than two windows ({self.limits['min_samples']} samples): the tuning cannot be estimated")

    def estimate_device(self, songs: Sequence[torch.Tensor]) -> Tuple[np.ndarray, torch.Tensor]:
        """checked device songs -> (tuning int64 [n] on the host, sim float64 [n][100] on the device)"""
        dev = self._device()
        tun, sims = [], []
        with torch.cuda.device(dev):
            for i0 in range(0, len(songs), self.limits["max_songs"]):
                group = songs[i0: i0 + self.limits["max_songs"]]
                tuning = torch.empty(len(group), dtype=torch.int32, device=dev)
                sim = torch.empty(len(group), N_THETA, dtype=torch.float64, device=dev)
                ws = torch.empty(self.workspace_bytes([int(t.numel()) for t in group]), dtype=torch.uint8, device=dev)
                self.run_raw(group, tuning, sim, ws)
                tun.append(tuning)
                sims.append(sim)
            hold(songs, dev)
        return torch.cat(tun).cpu().numpy().astype(np.int64), torch.cat(sims)

    def estimate_many(self, wavs: Sequence, details: bool = False):
        """songs [N_s] -> tuning in cents, int64 [n]; with ``details`` also sim float64 [n][100] (host).  A song's numbers depend on its samples alone: bit-identical
        alone, in any batch and in any order."""
        if len(wavs) == 0:
            return (np.zeros(0, np.int64), np.zeros((0, N_THETA))) if details else np.zeros(0, np.int64)
        tun, sim = self.estimate_device(self.check_songs(wavs))
        return (tun, sim.cpu().numpy()) if details else tun

    def estimate_files_many(self, paths: Sequence, loader=None, details: bool = False):
        """``estimate_many`` from WAV files of any rate and channel count, loaded on the device as mono 22 050 Hz (``etude_amd.audio``).  loader: an
        ``AudioLoader`` (default: one per device, made once)"""
        if loader is None:
            from .audio import default_audio_loader
            loader = default_audio_loader(self.device)
        return self.estimate_many(loader.load_many(paths, FS, mono=True), details)

    def estimate(self, wav) -> int:
        return int(self.estimate_many([wav])[0])


_default: Dict[str, TuningEstimator] = {}


def default_tuning_estimator(device="cuda") -> TuningEstimator:
    """one ``TuningEstimator`` per device, made once"""
    key = str(torch.device(device))
    if key not in _default:
        _default[key] = TuningEstimator(device)
    return _default[key]


def estimate_tuning(x, Fs: int = FS) -> int:
    """the reference's call shape: ``estimate_tuning(audio, fs)`` -> cents.  The engine is fixed to 22 050 Hz."""
    if int(Fs) != FS or Fs != int(Fs):
        raise ValueError(f"estimate_tuning: the engine is fixed to Fs = {FS}, got {Fs} (resample first: AudioLoader().resample_many([x], Fs, {FS}))")
    return default_tuning_estimator().estimate(x)
