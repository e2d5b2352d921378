"""Audio loading on the MI355X: ``AudioLoader`` -- WAV files (or sample arrays) of any rate, width and channel count -> float32 device tensors at the rate and
layout an engine asks for: mono 22 050 Hz for ``AlignFeatures`` and ``TuningEstimator``, ``[2][N]`` at 44 100 Hz for ``StemSeparator``.

Stands in for ``librosa.load(path, sr=22050)`` (etude/data/aligner.py:71-72, scripts/preprocess.py:135) and ``torchaudio.load`` (scripts/run_separation.py:89).  The
host walks the file's chunks (``read_wav_raw``) and hands the ``data`` chunk's bytes to the device as they are; decoding, deinterleaving, the mono mean and the
polyphase windowed-sinc filter are one launch per source rate (csrc/resample.hip).  The filter is this project's own, modelled on resampy's ``kaiser_best`` and
``kaiser_fast``; DESIGN.md 4q is the contract, tests/audio_np.py restates it in fp64 numpy.  soxr, resampy and librosa are not dependencies and parity with them is
unpinned.  Files other than RIFF/WAVE stay the caller's to decode.
"""
from __future__ import annotations

import ctypes as C
from math import gcd
from pathlib import Path
from typing import Callable, Dict, List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i32, i64, nonneg, ptrs

# the sample formats of the C ABI (ETD_PCM_*) and their bytes per sample
FORMATS = {"U8": 0, "S16": 1, "S24": 2, "S32": 3, "F32": 4, "F64": 5, "F32_PLANAR": 6}
WIDTH = {"U8": 1, "S16": 2, "S24": 3, "S32": 4, "F32": 4, "F64": 8, "F32_PLANAR": 4}
# quality -> (zero crossings Z, Kaiser beta, roll-off r): resampy's kaiser_best and kaiser_fast
QUALITY = {"best": (64, 14.769656459379492, 0.9475937167399596), "fast": (16, 8.555504641634386, 0.85)}
MAX_TABLE = 1 << 22
MAX_SONGS = 4096


def _ratio(sr_in: int, sr_out: int) -> Tuple[int, int]:
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates are positive integers, got {sr_in} -> {sr_out}")
    g = gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def filter_shape(sr_in: int, sr_out: int, quality: str = "best") -> Tuple[int, int, int]:
    """-> (up, down, half): up / down = sr_out / sr_in in lowest terms, half = ceil(Z / min(1, up / down)) in integers"""
    if quality not in QUALITY:
        raise ValueError(f"quality is one of {sorted(QUALITY)}, got {quality!r}")
    up, down = _ratio(sr_in, sr_out)
    Z = QUALITY[quality][0]
    return up, down, Z if up >= down else -((-Z * down) // up)


def resample_filter(sr_in: int, sr_out: int, quality: str = "best") -> Tuple[np.ndarray, int, int, int]:
    """-> (table float64 [up][K = 2 half], up, down, half).  table[p][k] = h(t) at t = k - half + 1 - p / up input samples, the weight of x[i0 - half + 1 + k] in
    the output at i0 + p / up:  h(t) = s r sinc(s r t) I0(beta sqrt(1 - (s t / Z)^2)) / I0(beta) inside |s t| < Z, 0 elsewhere, s = min(1, up / down).
    t is kept as the integer m = (k - half + 1) up - p over up, so the window's edge is an integer comparison and h(-t) == h(t) exactly."""
    up, down, half = filter_shape(sr_in, sr_out, quality)
    Z, beta, r = QUALITY[quality]
    m = (np.arange(2 * half, dtype=np.int64)[None, :] - half + 1) * up - np.arange(up, dtype=np.int64)[:, None]
    big = max(up, down)                                  # s t = m / big
    u = m.astype(np.float64) / (big * Z)
    inside = np.abs(m) < Z * big
    s = min(1.0, up / down)
    win = np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta)
    h = s * r * np.sinc(r * (m.astype(np.float64) / big)) * win
    return np.where(inside, h, 0.0), up, down, half


def resampled_len(n: int, sr_in: int, sr_out: int) -> int:
    """N' = ceil(n up / down), in integers"""
    up, down = _ratio(sr_in, sr_out)
    return -((-int(n) * up) // down)


def read_wav_raw(path: Union[str, Path]) -> Tuple[np.ndarray, str, int, int, int]:
    """RIFF/WAVE -> (the ``data`` chunk's bytes as a uint8 array, format name (a key of FORMATS), channels, sample_rate, frames), nothing decoded.  Walks the chunks
    as ``extractor.read_wav`` does (odd sizes padded, WAVE_FORMAT_EXTENSIBLE resolved, unknown chunks skipped); a ``data`` size that runs past the end of the file is
    clipped to whole frames."""
    raw = np.fromfile(str(path), dtype=np.uint8)
    head = raw[:12].tobytes()
    if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    u = lambda a, b: int.from_bytes(raw[a:b].tobytes(), "little")      # noqa: E731
    pos, fmt = 12, None
    while pos + 8 <= raw.size:
        cid, size = raw[pos:pos + 4].tobytes(), u(pos + 4, pos + 8)
        b0 = pos + 8
        if cid == b"fmt ":
            tag, ch, sr, bits = u(b0, b0 + 2), u(b0 + 2, b0 + 4), u(b0 + 4, b0 + 8), u(b0 + 14, b0 + 16)
            if tag == 0xFFFE and size >= 26:
                tag = u(b0 + 24, b0 + 26)
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            if fmt is None:
                raise ValueError(f"{path}: data chunk before fmt chunk")
            tag, ch, sr, bits = fmt
            name = {(1, 8): "U8", (1, 16): "S16", (1, 24): "S24", (1, 32): "S32", (3, 32): "F32", (3, 64): "F64"}.get((tag, bits))
            if name is None:
                raise ValueError(f"{path}: unsupported WAV format tag={tag} bits={bits} (PCM of 8, 16, 24, 32 bits and IEEE float of 32, 64 are read)")
            if ch < 1:
                raise ValueError(f"{path}: the fmt chunk names {ch} channels")
            frames = min(size, raw.size - b0) // (ch * WIDTH[name])
            return raw[b0: b0 + frames * ch * WIDTH[name]], name, ch, sr, frames
        pos += 8 + size + (size & 1)
    raise ValueError(f"{path}: no data chunk")


class Resampler(Engine):
    """One handle of the C ABI: one (sr_in, sr_out, quality).  Constructing designs the table on the host and needs no GPU."""
    _destroy = "etd_resample_destroy"

    def __init__(self, sr_in: int, sr_out: int, quality: str = "best", device: Union[str, torch.device] = "cuda"):
        self.device = torch.device("cuda" if device == "auto" else device)
        self._lib = _lib.lib()
        self.sr_in, self.sr_out, self.quality = int(sr_in), int(sr_out), quality
        self.up, self.down, self.half = filter_shape(sr_in, sr_out, quality)
        cfg = _lib.ResampleCfg(sr_in=self.sr_in, sr_out=self.sr_out, quality={"best": 0, "fast": 1}[quality], up=self.up, down=self.down, half=self.half)
        # (a table above the budget is not designed: the library refuses the shape with its own sentence)
        tab = None
        if self.up * 2 * self.half <= MAX_TABLE and (self.up, self.down) != (1, 1):
            tab = np.ascontiguousarray(resample_filter(sr_in, sr_out, quality)[0].astype(np.float32))
        h = C.c_void_p()
        _lib.check(self._lib.etd_resample_create(C.byref(cfg), C.c_void_p(tab.ctypes.data if tab is not None else None), C.byref(h)), "etd_resample_create")
        self._adopt(h)

    def out_len(self, n: int) -> int:
        return nonneg(self._lib.etd_resample_out_len(self.h, int(n)), "etd_resample_out_len")

    def workspace_bytes(self, frames: Sequence[int], channels: Sequence[int], mono: Sequence[bool]) -> int:
        return nonneg(self._lib.etd_resample_workspace_bytes(self.h, len(frames), i64(frames), i32(channels), i32(mono)), "etd_resample_workspace_bytes")

    def plan(self, frames: Sequence[int], channels: Sequence[int], mono: Sequence[bool]) -> np.ndarray:
        """test hook (host arithmetic): the workgroups of a call with these shapes, int64 [n_tiles][4] = song, channel, first output, outputs"""
        n = C.c_longlong()
        args = (self.h, len(frames), i64(frames), i32(channels), i32(mono))
        rc = self._lib.etd_resample_debug_layout(*args, None, 0, C.byref(n))
        if rc != -12:                                        # (ETD_ENOMEM is the answer to a query without a buffer)
            _lib.check(rc, "etd_resample_debug_layout")
        out = np.zeros((n.value, 4), np.int64)
        _lib.check(self._lib.etd_resample_debug_layout(*args, out.ctypes.data_as(_lib.c_i64_p), n.value, C.byref(n)), "etd_resample_debug_layout")
        return out

    def run_raw(self, srcs: Sequence[torch.Tensor], frames, channels, formats, mono, outs: Sequence[torch.Tensor], ws: torch.Tensor) -> None:
        """one launch on device tensors with the caller's buffers: srcs the raw samples (uint8, or float32 for the planar format), outs float32 [C][N'] / [N']"""
        dev = self._device()
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_resample_run(self.h, ptrs(srcs), len(srcs), i64(frames), i32(channels), i32([FORMATS[f] for f in formats]), i32(mono),
                                                  i64([t.numel() * t.element_size() for t in srcs]), ptrs(outs), C.c_void_p(ws.data_ptr()),
                                                  ws.numel() * ws.element_size(), self._stream(dev)), "etd_resample_run")

    def run_many(self, srcs: Sequence[torch.Tensor], frames, channels, formats, mono) -> List[torch.Tensor]:
        """device tensors of raw samples -> one float32 tensor per song, [C][N'] or [N'] where mono; MAX_SONGS songs per launch"""
        dev = self._device()
        outs = []
        with torch.cuda.device(dev):
            for a in range(0, len(srcs), MAX_SONGS):
                sl = slice(a, a + MAX_SONGS)
                group = [torch.empty((self.out_len(n),) if m else (c, self.out_len(n)), dtype=torch.float32, device=dev)
                         for n, c, m in zip(frames[sl], channels[sl], mono[sl])]
                ws = torch.empty(self.workspace_bytes(frames[sl], channels[sl], mono[sl]), dtype=torch.uint8, device=dev)
                self.run_raw(srcs[sl], frames[sl], channels[sl], formats[sl], mono[sl], group, ws)
                outs += group
            hold(srcs, dev)
        return outs


class AudioLoader(Engine):
    """WAV files or sample arrays -> float32 device tensors at a target rate: ``[C][N']``, or ``[N']`` with ``mono=True`` (the fp32 mean of the channels, taken
    before the filter).  One ``Resampler`` per (source rate, target rate), made on first use and kept; a file already at the target rate is only decoded.
    Constructing needs no GPU; loading does: there is no CPU path."""

    def __init__(self, device: Union[str, torch.device] = "cuda", quality: str = "best"):
        if quality not in QUALITY:
            raise ValueError(f"quality is one of {sorted(QUALITY)}, got {quality!r}")
        self.device = torch.device("cuda" if device == "auto" else device)
        self.quality = quality
        self._resamplers: Dict[Tuple[int, int], Resampler] = {}

    def resampler(self, sr_in: int, sr_out: int) -> Resampler:
        key = (int(sr_in), int(sr_out))
        if key not in self._resamplers:
            self._resamplers[key] = Resampler(key[0], key[1], self.quality, self.device)
        return self._resamplers[key]

    def close(self) -> None:
        for r in getattr(self, "_resamplers", {}).values():
            r.close()
        self._resamplers = {}

    def load_many(self, paths: Sequence, sr: int, mono: bool = False) -> List[torch.Tensor]:
        """files -> one device tensor per file at ``sr`` Hz, in the order of ``paths``.  The files are grouped by their own rate: one launch per rate in the batch."""
        files = [read_wav_raw(p) for p in paths]
        if not files:
            return []
        dev = self._device()
        out: List[torch.Tensor] = [None] * len(files)
        for rate in sorted({f[3] for f in files}):
            idx = [i for i, f in enumerate(files) if f[3] == rate]
            rs = self.resampler(rate, sr)                    # (a rate pair the library refuses raises here, before anything is uploaded)
            live = [i for i in idx if files[i][4] > 0]
            for i in idx:
                if files[i][4] == 0:
                    out[i] = torch.zeros((0,) if mono else (files[i][2], 0), dtype=torch.float32, device=dev)
            if not live:
                continue
            srcs = [torch.from_numpy(files[i][0]).to(dev) for i in live]
            res = rs.run_many(srcs, [files[i][4] for i in live], [files[i][2] for i in live], [files[i][1] for i in live], [mono] * len(live))
            for i, t in zip(live, res):
                out[i] = t
        return out

    def load(self, path, sr: int, mono: bool = False) -> torch.Tensor:
        return self.load_many([path], sr, mono)[0]

    def resample_many(self, wavs: Sequence, sr_in: int, sr_out: int, mono: bool = False) -> List[torch.Tensor]:
        """``[C][N]`` or ``[N]`` arrays or tensors (host or device) at ``sr_in`` Hz -> device tensors at ``sr_out`` Hz: ``[C][N']``, or ``[N']`` for a 1-d song and
        with ``mono``.  The samples must be finite (checked with ONE host synchronisation)."""
        for i, x in enumerate(wavs):
            shp = tuple(x.shape) if hasattr(x, "shape") else None
            if shp is None or len(shp) not in (1, 2) or shp[-1] < 1 or (len(shp) == 2 and not 1 <= shp[0] <= 8):
                raise ValueError(f"song {i}: need samples [N] or [C][N] with 1 <= C <= 8 and N >= 1, got shape {shp}")
        if len(wavs) == 0:
            return []
        rs = self.resampler(sr_in, sr_out)
        dev = self._device()
        songs = [torch.as_tensor(x).detach().to(dev, torch.float32).contiguous() for x in wavs]
        bad = torch.stack([torch.isfinite(t).all() for t in songs]).logical_not().nonzero().flatten().tolist()      # (one host synchronisation for the call)
        if bad:
            raise ValueError(f"song {bad[0]}: holds a non-finite sample")
        res = rs.run_many(songs, [t.shape[-1] for t in songs], [t.shape[0] if t.dim() == 2 else 1 for t in songs], ["F32_PLANAR"] * len(songs), [mono] * len(songs))
        return [r[0] if (t.dim() == 1 and r.dim() == 2) else r for t, r in zip(songs, res)]

    def as_load_fn(self, sr: int = 22050) -> Callable:
        """-> the ``path -> mono samples at sr Hz`` callable ``AlignFeatures.as_feature_fn`` asks for"""
        return lambda path: self.load(path, sr, mono=True)


_default: Dict[str, AudioLoader] = {}


def default_audio_loader(device="cuda") -> AudioLoader:
    """one ``AudioLoader`` (quality "best") per device, made once"""
    key = str(torch.device(device))
    if key not in _default:
        _default[key] = AudioLoader(device)
    return _default[key]
