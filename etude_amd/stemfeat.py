"""Stem mel-dB features on the MI355X: ``StemFeatures`` <- process_stems_to_spectrogram of scripts/run_separation.py:124-141, 163-183.

Per separated stem: channel mean, ``librosa.stft(n_fft=4096, hop_length=1024)``, ``|X|^2``, the 128-band Slaney mel filterbank (30 Hz .. 11 kHz at 44.1 kHz),
``librosa.power_to_db(ref=np.max)`` -- the [instr][T][128] features ``BeatDetector`` reads, made where the separator leaves its stems: on the device (csrc/stemfeat.hip,
three launches for a whole ragged batch of songs).  DESIGN.md 4d is the contract; tests/stemfeat_np.py restates it in fp64 numpy.  librosa is not a dependency and
parity with it is unpinned.

``mel_filterbank`` is a host function (``librosa.filters.mel`` with htk=False, norm="slaney", formed in fp64, returned as float32).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i64, nonneg, ptrs
from .frontend import _dense_to_csr

FRAMINGS = {"librosa": 0, "librosa_reflect": 1, "spleeter": 2}          # ETD_STEMFEAT_*


def _hz_to_mel(f: float) -> float:
    """Slaney scale: f / (200 / 3) below 1 kHz, 15 + ln(f / 1000) / (ln(6.4) / 27) above"""
    f = float(f)
    return 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0) if f >= 1000.0 else f / (200.0 / 3.0)


def _mel_to_hz(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sr: int = 44100, n_fft: int = 4096, n_mels: int = 128, fmin: float = 30.0, fmax: float = 11000.0) -> np.ndarray:
    """``librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)`` with its defaults (htk=False, norm="slaney") -> [n_mels][n_fft / 2 + 1] float32.

    n_mels + 2 points equally spaced on the Slaney mel scale, triangles max(0, min(lower, upper)) over rfftfreq, each scaled by 2 / (f[m + 2] - f[m]); formed in fp64."""
    if n_mels < 1 or n_fft < 2 or not 0 <= fmin < fmax:
        raise ValueError(f"mel_filterbank: need n_mels >= 1, n_fft >= 2, 0 <= fmin < fmax; got {n_mels}, {n_fft}, {fmin}, {fmax}")
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb.astype(np.float32)


def _csr(fb: np.ndarray):
    """[n_mels][bins] -> (start, length, weights) of each band's span of non-zeros (zeros inside a span are kept): the front end's, on its [bins][n_mels] layout"""
    return _dense_to_csr(fb.T)


class StemFeatures(Engine):
    """Separated stems -> the Beat-Transformer's mel-dB features, on the device.

    A song is [instr][channels][N] float32 (torch tensor on the device or the host, or a numpy array), finite, N >= 1.  Spleeter's ``{name: [N][channels]}`` dict maps
    onto it as ``np.stack([d[name].T for name in names])`` (the stems in the order the model was trained with); Demucs' [instr][channels][N] output is taken as it is.

    ``framing``: "librosa" (librosa.stft >= 0.10: centred frames, zeros outside the signal, T = 1 + N // hop), "librosa_reflect" (librosa < 0.10: reflection;
    N <= n_fft / 2 is refused) or "spleeter" (Spleeter 2.x's own STFT: n_fft zeros on both ends, T = 1 + (N + n_fft) // hop).
    Constructing needs no GPU (``num_frames`` is host arithmetic); ``features`` / ``features_many`` do: there is no CPU path."""
    _destroy = "etd_stemfeat_destroy"

    def __init__(self, sample_rate: int = 44100, n_fft: int = 4096, hop: int = 1024, n_mels: int = 128, fmin: float = 30.0, fmax: float = 11000.0,
                 top_db: float = 80.0, amin: float = 1e-10, framing: str = "librosa", device: Union[str, torch.device] = "cuda"):
        if framing not in FRAMINGS:
            raise ValueError(f"StemFeatures: framing must be one of {sorted(FRAMINGS)}, got {framing!r}")
        n_fft, hop, n_mels = int(n_fft), int(hop), int(n_mels)
        if n_fft < 64 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise ValueError(f"StemFeatures: n_fft must be a power of two in 64 .. 4096, got {n_fft}")
        if hop < 1 or not 1 <= n_mels <= 1024:
            raise ValueError(f"StemFeatures: need hop >= 1 and 1 <= n_mels <= 1024, got {hop}, {n_mels}")
        if not (amin > 0 and top_db > 0):
            raise ValueError(f"StemFeatures: amin and top_db must be positive, got {amin}, {top_db}")
        self.sample_rate, self.n_fft, self.hop, self.n_mels, self.framing = int(sample_rate), n_fft, hop, n_mels, framing
        self.top_db, self.amin = float(top_db), float(amin)
        self.device = torch.device("cuda" if device == "auto" else device)
        self.filterbank = mel_filterbank(self.sample_rate, n_fft, n_mels, fmin, fmax)
        window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(np.float32)          # periodic Hann
        start, length, w = _csr(self.filterbank)
        cfg = _lib.StemFeatCfg(n_fft=n_fft, hop=hop, n_mels=n_mels, framing=FRAMINGS[framing], amin=self.amin, top_db=self.top_db)
        self._lib = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._lib.etd_stemfeat_create(C.byref(cfg), window.ctypes.data, start.ctypes.data, length.ctypes.data, w.ctypes.data, C.byref(h)), "etd_stemfeat_create")
        self._adopt(h)

    def num_frames(self, N: int) -> int:
        T = int(self._lib.etd_stemfeat_num_frames(self.h, int(N)))
        if T < 0:
            raise ValueError(f"num_frames: N must be >= 1, got {N}")
        return T

    def features_many(self, stems_list: Sequence) -> Tuple[torch.Tensor, List[int]]:
        """songs [instr][channels][N_s] -> (the songs' [instr][T_s][n_mels] blocks back to back in one flat device tensor, [T_s]): ``BeatDetector``'s packed input.
        Every song of a call has the same instr and channels.  A host entry is uploaded on its own; nothing is concatenated."""
        if len(stems_list) == 0:
            raise ValueError("features_many: no songs")
        shapes = []
        for i, x in enumerate(stems_list):
            shp = tuple(x.shape) if hasattr(x, "shape") else None
            if shp is None or len(shp) != 3:
                raise ValueError(f"song {i}: stems must be [instr][channels][N], got shape {shp}")
            if shp[0] < 1 or shp[1] < 1 or shp[2] < 1:
                raise ValueError(f"song {i}: stems must be [instr >= 1][channels >= 1][N >= 1], got {shp}")
            if shp[:2] != tuple(stems_list[0].shape[:2]):
                raise ValueError(f"song {i}: [instr][channels] = {shp[:2]} differs from song 0's {tuple(stems_list[0].shape[:2])}")
            if self.framing == "librosa_reflect" and shp[2] <= self.n_fft // 2:
                raise ValueError(f"song {i}: framing 'librosa_reflect' needs N > n_fft / 2 = {self.n_fft // 2}, got {shp[2]}")
            shapes.append(shp)
        dev = self._device()
        songs = [torch.as_tensor(x).to(dev, torch.float32).contiguous() for x in stems_list]
        n, (instr, channels) = len(songs), shapes[0][:2]
        Ts = [self.num_frames(s[2]) for s in shapes]
        feat = torch.empty(instr * self.n_mels * sum(Ts), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_stemfeat_run(self.h, ptrs(songs), n, instr, channels, i64([s[2] for s in shapes]), C.c_void_p(feat.data_ptr()), self._stream(dev)),
                       "etd_stemfeat_run")
            hold(songs, dev)
        return feat, Ts

    def features(self, stems) -> torch.Tensor:
        """one song [instr][channels][N] -> [instr][T][n_mels] device tensor"""
        feat, Ts = self.features_many([stems])
        return feat.view(int(stems.shape[0]), Ts[0], self.n_mels)

    def workspace_bytes(self, Ns: Sequence[int], instr: int) -> int:
        return nonneg(self._lib.etd_stemfeat_workspace_bytes(self.h, len(Ns), int(instr), i64(Ns)), "etd_stemfeat_workspace_bytes")
