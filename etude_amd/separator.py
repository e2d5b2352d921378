"""A five-stem source separator on the MI355X: ``StemSeparator`` takes a song's audio to its stems, the stage in front of ``StemFeatures`` / ``BeatDetector``.

A U-Net mask separator modelled on Spleeter 2.x's ``5stems`` model (the default backend of scripts/run_separation.py): STFT (n_fft zeros on both ends, periodic Hann),
one six-level U-Net per instrument on the magnitudes below bin ``F`` in segments of ``T`` frames, a softmax over the instruments, ratio masks, inverse STFT
(csrc/separator.hip).  DESIGN.md 4m is the contract; tests/separator_np.py restates it.  Spleeter and its checkpoints are not dependencies, and parity with its
TensorFlow graph is unpinned; converting a TensorFlow checkpoint, Demucs and training are out of scope.

The state: a flat dict of float32 arrays, per instrument ``name``
    "{name}.conv{l}.weight"    [5][5][Cin][Cout]     l = 1 .. 6   Cin = n_channels, then conv_n_filters[l - 2]; Cout = conv_n_filters[l - 1]
    "{name}.conv{l}.bias"      [Cout]
    "{name}.deconv{j}.weight"  [5][5][Cout][Cin]     j = 1 .. 6   Cout = conv_n_filters[5 - j] (j = 6: 1); Cin = conv_n_filters[5] for j = 1, else 2 conv_n_filters[6 - j]
    "{name}.deconv{j}.bias"    [Cout]                             (the input channels are [skip conv_{7 - j}, decoder j - 1], the skip first)
    "{name}.bn{n}.gamma" / ".beta" / ".mean" / ".var"  [C]        n = 1 .. 6 the encoder's norms, n = 7 .. 12 the decoder's (C = that layer's Cout)
    "{name}.head.weight"       [4][4][1][n_channels]
    "{name}.head.bias"         [n_channels]
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i64, nonneg, ptrs

LEVELS = 6            # ETD_SEP_LEVELS
MAX_INSTR = 16        # ETD_SEP_MAX_INSTR
MAX_CHANNELS = 8      # ETD_SEP_MAX_CHANNELS
MWF_MAX_ITERATIONS = 8    # etd_sep_set_mwf's range
MWF_MAX_CHANNELS = 2


@dataclass
class SeparatorConfig:
    instruments: Tuple[str, ...] = ("vocals", "piano", "drums", "bass", "other")      # the order is the caller's to match to their weights
    sample_rate: int = 44100
    n_fft: int = 4096
    hop: int = 1024
    T: int = 512                                   # frames per segment
    F: int = 1024                                  # bins the U-Net reads; the masks are 0 above
    n_channels: int = 2
    conv_n_filters: Tuple[int, ...] = (16, 32, 64, 128, 256, 512)
    separation_exponent: int = 2
    mask_eps: float = 1e-10
    bn_eps: float = 1e-3

    def check(self) -> None:
        """ValueError for anything the engine refuses; needs no GPU"""
        self.instruments = tuple(self.instruments)
        self.conv_n_filters = tuple(int(c) for c in self.conv_n_filters)
        if len(self.instruments) < 1:
            raise ValueError("SeparatorConfig: no instruments")
        if len(self.instruments) > MAX_INSTR or len(set(self.instruments)) != len(self.instruments) or any(not isinstance(s, str) or not s for s in self.instruments):
            raise ValueError(f"SeparatorConfig: instruments must be 1 .. {MAX_INSTR} distinct non-empty names, got {self.instruments}")
        if self.n_fft < 1024 or self.n_fft > 4096 or self.n_fft & (self.n_fft - 1):
            raise ValueError(f"SeparatorConfig: n_fft must be a power of two in 1024 .. 4096, got {self.n_fft}")
        if self.hop * 4 != self.n_fft:
            raise ValueError(f"SeparatorConfig: hop must be n_fft / 4 = {self.n_fft // 4}, got {self.hop}")
        if len(self.conv_n_filters) != LEVELS:
            raise ValueError(f"SeparatorConfig: conv_n_filters must hold {LEVELS} counts, got {len(self.conv_n_filters)}")
        if any(c < 1 or c > 4096 for c in self.conv_n_filters):
            raise ValueError(f"SeparatorConfig: every filter count must be in 1 .. 4096, got {self.conv_n_filters}")
        if self.F > self.n_fft // 2:
            raise ValueError(f"SeparatorConfig: F must be <= n_fft / 2 = {self.n_fft // 2}, got {self.F}")
        m = 2 ** len(self.conv_n_filters)
        if self.T < m or self.T % m or self.F < m or self.F % m:
            raise ValueError(f"SeparatorConfig: T and F must be positive multiples of {m}, got {self.T}, {self.F}")
        if self.T > 65536:
            raise ValueError(f"SeparatorConfig: T must be <= 65536, got {self.T}")
        if not 1 <= self.n_channels <= MAX_CHANNELS:
            raise ValueError(f"SeparatorConfig: n_channels must be in 1 .. {MAX_CHANNELS}, got {self.n_channels}")
        if int(self.separation_exponent) != self.separation_exponent or not 1 <= self.separation_exponent <= 8:
            raise ValueError(f"SeparatorConfig: separation_exponent must be an integer in 1 .. 8, got {self.separation_exponent}")
        if not (self.mask_eps > 0 and np.isfinite(self.mask_eps) and self.bn_eps > 0 and np.isfinite(self.bn_eps)):
            raise ValueError(f"SeparatorConfig: mask_eps and bn_eps must be positive and finite, got {self.mask_eps}, {self.bn_eps}")
        if self.sample_rate < 1:
            raise ValueError(f"SeparatorConfig: sample_rate must be positive, got {self.sample_rate}")


def expected_keys(cfg: SeparatorConfig) -> Dict[str, tuple]:
    """key -> shape of the state a config reads (the layout in the module docstring)"""
    f = tuple(cfg.conv_n_filters)
    enc = (cfg.n_channels,) + f
    out: Dict[str, tuple] = {}
    for name in cfg.instruments:
        for l in range(1, LEVELS + 1):
            out[f"{name}.conv{l}.weight"] = (5, 5, enc[l - 1], enc[l])
            out[f"{name}.conv{l}.bias"] = (enc[l],)
            cout = f[5 - l] if l < LEVELS else 1
            cin = f[5] if l == 1 else 2 * f[6 - l]
            out[f"{name}.deconv{l}.weight"] = (5, 5, cout, cin)
            out[f"{name}.deconv{l}.bias"] = (cout,)
            for n, ch in ((l, enc[l]), (LEVELS + l, cout)):
                for part in ("gamma", "beta", "mean", "var"):
                    out[f"{name}.bn{n}.{part}"] = (ch,)
        out[f"{name}.head.weight"] = (4, 4, 1, cfg.n_channels)
        out[f"{name}.head.bias"] = (cfg.n_channels,)
    return out


def check_separator_state(state: Dict, cfg: SeparatorConfig) -> None:
    """ValueError naming the first key that is missing or has the wrong shape"""
    for k, shp in expected_keys(cfg).items():
        if k not in state:
            raise ValueError(f"separator state: missing key {k!r}")
        got = tuple(np.shape(state[k]))
        if got != shp:
            raise ValueError(f"separator state: {k!r} has shape {got}, expected {shp}")


def init_separator_state(cfg: Optional[SeparatorConfig] = None, seed: int = 0) -> Dict[str, np.ndarray]:
    """a random state: He-uniform kernels (bound sqrt(6 / fan_in), fan_in = taps x input channels), zero biases, gamma and var uniform in 0.5 .. 1.5, beta and mean
    normal with sigma 0.1; every value from ``numpy.random.default_rng(seed)`` in the order of ``expected_keys``"""
    cfg = cfg or SeparatorConfig()
    cfg.check()
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    for k, shp in expected_keys(cfg).items():
        if k.endswith(".weight"):
            cin = shp[3] if ".deconv" in k else shp[2]
            bound = np.sqrt(6.0 / (shp[0] * shp[1] * cin))
            v = rng.uniform(-bound, bound, shp)
        elif k.endswith(".bias"):
            v = np.zeros(shp)
        elif k.endswith(".gamma") or k.endswith(".var"):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.normal(0.0, 0.1, shp)
        out[k] = np.ascontiguousarray(v, np.float32)
    return out


def load_separator_state(path) -> Dict[str, np.ndarray]:
    """what ``StemSeparator.save`` wrote: a flat dict through ``torch.save``"""
    sd = torch.load(str(path), map_location="cpu")
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a separator state (a flat dict of arrays)")
    return {k: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v), np.float32) for k, v in sd.items()}


class StemSeparator(Engine):
    """A song's audio -> its stems, on the device.

    A song is [n_channels][N] float32 (torch tensor on the device or the host, or a numpy array), or [N] mono (duplicated to n_channels), finite, N >= 1.
    ``separate_many`` returns one [instr][n_channels][N] device tensor per song -- what ``StemFeatures.features_many`` takes; ``separate`` returns Spleeter's
    ``{name: [N][channels]}`` of numpy arrays.  A song's stems are bit-identical alone, in any batch, under any ``workspace_bytes`` and from run to run.
    ``workspace_bytes`` bounds the device workspace: songs are grouped and (segment, instrument) units sub-batched under it; one song with one unit is the floor
    (``workspace_total_bytes`` tells what a call holds).
    ``mwf_iterations`` (0 .. 8, default 0 = off; 1 or 2 channels) refines the masked spectra by that many passes of multichannel Wiener filtering before the inverse
    STFT, the ratio mask being the initial estimate (csrc/separator_mwf.hip; modelled on norbert's, parity unpinned).
    Constructing needs no GPU; separating does: there is no CPU path."""
    _destroy = "etd_sep_destroy"

    def __init__(self, config: Optional[SeparatorConfig] = None, state: Optional[Dict] = None, seed: int = 0, device: Union[str, torch.device] = "cuda",
                 workspace_bytes: int = 4 << 30, mwf_iterations: int = 0):
        self.config = cfg = config or SeparatorConfig()
        cfg.check()
        mwf_iterations = self._check_mwf(mwf_iterations)
        if workspace_bytes < 1:
            raise ValueError(f"StemSeparator: workspace_bytes must be positive, got {workspace_bytes}")
        if state is None:
            state = init_separator_state(cfg, seed)
        check_separator_state(state, cfg)
        keys = expected_keys(cfg)
        self.state = {k: np.ascontiguousarray(np.asarray(state[k].detach().cpu() if isinstance(state[k], torch.Tensor) else state[k]), np.float32) for k in keys}
        for k, v in self.state.items():
            if not np.isfinite(v).all():
                raise ValueError(f"separator state: {k!r} holds a non-finite value")
        self.device = torch.device("cuda" if device == "auto" else device)
        self.workspace_bytes = int(workspace_bytes)
        ccfg = _lib.SepCfg(n_instr=len(cfg.instruments), n_channels=cfg.n_channels, n_fft=cfg.n_fft, hop=cfg.hop, T=cfg.T, F=cfg.F,
                           filters=(C.c_int * LEVELS)(*cfg.conv_n_filters), separation_exponent=int(cfg.separation_exponent), mask_eps=cfg.mask_eps, bn_eps=cfg.bn_eps,
                           workspace_bytes=self.workspace_bytes)
        self._lib = _lib.lib()
        names, ptrs, numels, n, keep = _lib.weights_arrays(self.state)
        instr = (C.c_char_p * len(cfg.instruments))(*[s.encode() for s in cfg.instruments])
        h = C.c_void_p()
        _lib.check(self._lib.etd_sep_create(C.byref(ccfg), instr, names, ptrs, numels, n, C.byref(h)), "etd_sep_create")
        del keep
        self._adopt(h)
        self.mwf_iterations = mwf_iterations

    # ------------------------------------------------------------------ host arithmetic
    def num_frames(self, N: int) -> int:
        Tf = int(self._lib.etd_sep_num_frames(self.h, int(N)))
        if Tf < 0:
            raise ValueError(f"num_frames: N must be >= 1, got {N}")
        return Tf

    @property
    def unit_bytes(self) -> int:
        return int(self._lib.etd_sep_unit_bytes(self.h))

    def segment_flops(self) -> float:
        return float(self._lib.etd_sep_segment_flops(self.h))

    def workspace_total_bytes(self, Ns: Sequence[int]) -> int:
        return nonneg(self._lib.etd_sep_workspace_bytes(self.h, len(Ns), i64(Ns)), "etd_sep_workspace_bytes")

    def _check_mwf(self, n) -> int:
        """ValueError for what etd_sep_set_mwf refuses; needs no GPU"""
        if isinstance(n, bool) or int(n) != n or not 0 <= n <= MWF_MAX_ITERATIONS:
            raise ValueError(f"StemSeparator: mwf_iterations must be an integer in 0 .. {MWF_MAX_ITERATIONS}, got {n!r}")
        if n > 0 and self.config.n_channels > MWF_MAX_CHANNELS:
            raise ValueError(f"StemSeparator: multichannel Wiener filtering takes 1 or {MWF_MAX_CHANNELS} channels, the config has {self.config.n_channels}")
        return int(n)

    @property
    def mwf_iterations(self) -> int:
        """Wiener passes every ``separate_many`` runs between the masks and the inverse STFT (0 = none); settable"""
        return nonneg(self._lib.etd_sep_get_mwf(self.h), "etd_sep_get_mwf")

    @mwf_iterations.setter
    def mwf_iterations(self, n: int) -> None:
        _lib.check(self._lib.etd_sep_set_mwf(self.h, self._check_mwf(n)), "etd_sep_set_mwf")

    def save(self, path) -> None:
        torch.save({k: torch.from_numpy(v) for k, v in self.state.items()}, str(path))

    # ------------------------------------------------------------------ device
    def _song_shape(self, i: int, x) -> tuple:
        shp = tuple(x.shape) if hasattr(x, "shape") else None
        if shp is None or len(shp) not in (1, 2):
            raise ValueError(f"song {i}: audio must be [channels][N] or [N], got shape {shp}")
        if shp[-1] < 1:
            raise ValueError(f"song {i}: N must be >= 1, got shape {shp}")
        if len(shp) == 2 and shp[0] not in (1, self.config.n_channels):
            raise ValueError(f"song {i}: audio must have 1 or {self.config.n_channels} channels, got {shp[0]}")
        return shp

    def separate_many(self, wavs: Sequence, mwf_iterations: Optional[int] = None) -> List[torch.Tensor]:
        """songs [n_channels][N_s] (or mono [N_s] / [1][N_s]) -> [instr][n_channels][N_s] device tensors, one per song.  ``mwf_iterations``: this call's Wiener
        passes instead of the engine's"""
        if mwf_iterations is not None:
            n, own = self._check_mwf(mwf_iterations), self.mwf_iterations
            if n != own:
                self.mwf_iterations = n
                try:
                    return self.separate_many(wavs)
                finally:
                    self.mwf_iterations = own
        if len(wavs) == 0:
            return []
        shapes = [self._song_shape(i, x) for i, x in enumerate(wavs)]
        dev = self._device()
        nc, ni = self.config.n_channels, len(self.config.instruments)
        songs = []
        for x in wavs:
            t = torch.as_tensor(x).to(dev, torch.float32)
            if t.dim() == 1:
                t = t[None]
            if t.shape[0] == 1 and nc > 1:
                t = t.expand(nc, -1)                   # mono: every channel is the one given
            songs.append(t.contiguous())
        bad = torch.stack([torch.isfinite(t).all() for t in songs]).logical_not().nonzero().flatten().tolist()      # (one host synchronisation for the call)
        if bad:
            raise ValueError(f"song {bad[0]}: the audio holds a non-finite value")
        n = len(songs)
        Ns = [s[-1] for s in shapes]
        outs = [torch.empty((ni, nc, N), dtype=torch.float32, device=dev) for N in Ns]
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_run(self.h, ptrs(songs), n, i64(Ns), ptrs(outs), self._stream(dev)), "etd_sep_run")
            hold(songs, dev)
        return outs

    def separate(self, wav) -> Dict[str, np.ndarray]:
        """one song -> ``{instrument: [N][n_channels] float32}``, the shape Spleeter's ``Separator.separate`` returns"""
        out = self.separate_many([wav])[0].cpu().numpy()
        return {name: np.ascontiguousarray(out[i].T) for i, name in enumerate(self.config.instruments)}

    # ------------------------------------------------------------------ test hooks (include/etude_hip_debug.h)
    def debug_stft(self, wav: torch.Tensor) -> torch.Tensor:
        """[n_channels][N] device tensor -> X [n_channels][Tf][n_fft / 2 + 1] complex64"""
        dev = self._device()
        wav = wav.to(dev, torch.float32).contiguous()
        N = int(wav.shape[1])
        X = torch.empty((self.config.n_channels, self.num_frames(N), self.config.n_fft // 2 + 1, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_debug_stft(self.h, C.c_void_p(wav.data_ptr()), N, C.c_void_p(X.data_ptr()), self._stream(dev)), "etd_sep_debug_stft")
        return torch.view_as_complex(X)

    def debug_layer(self, instr: int, kind: int, layer: int, x0: torch.Tensor, x1: Optional[torch.Tensor] = None):
        """one U-Net layer of instrument ``instr`` on units [n][H][W][C]: kind 0 = encoder ``layer`` -> (pre, act); 1 = decoder ``layer`` on (skip, up) -> act;
        2 = the head -> logits"""
        dev = self._device()
        cfg = self.config
        f = tuple(cfg.conv_n_filters)
        x0 = x0.to(dev, torch.float32).contiguous()
        n = int(x0.shape[0])
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        pre = act = None
        if kind == 0:
            shp = (n, cfg.T >> layer, cfg.F >> layer, f[layer - 1])
            pre, act = torch.empty(shp, dtype=torch.float32, device=dev), torch.empty(shp, dtype=torch.float32, device=dev)
        elif kind == 1:
            x1 = x1.to(dev, torch.float32).contiguous() if x1 is not None else None
            act = torch.empty((n, cfg.T >> (6 - layer), cfg.F >> (6 - layer), f[5 - layer] if layer < LEVELS else 1), dtype=torch.float32, device=dev)
        else:
            pre = torch.empty((n, cfg.T, cfg.F, cfg.n_channels), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_debug_layer(self.h, int(instr), int(kind), int(layer), p(x0), p(x1), n, p(pre), p(act), self._stream(dev)), "etd_sep_debug_layer")
        return (pre, act) if kind == 0 else act if kind == 1 else pre

    def debug_mask(self, logits: torch.Tensor, mag: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
        """logits [segs][instr][T][F][C], mag [segs * T][F][C], X [C][Tf][F] complex64 -> Y [instr][C][Tf][F] complex64"""
        dev = self._device()
        cfg = self.config
        logits, mag = logits.to(dev, torch.float32).contiguous(), mag.to(dev, torch.float32).contiguous()
        Xr = torch.view_as_real(X.to(dev, torch.complex64).contiguous()).contiguous()
        Tf = int(X.shape[1])
        Y = torch.empty((len(cfg.instruments), cfg.n_channels, Tf, cfg.F, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_debug_mask(self.h, C.c_void_p(logits.data_ptr()), C.c_void_p(mag.data_ptr()), C.c_void_p(Xr.data_ptr()), Tf,
                                                    C.c_void_p(Y.data_ptr()), self._stream(dev)), "etd_sep_debug_mask")
        return torch.view_as_complex(Y)

    def debug_istft(self, Y: torch.Tensor, N: int) -> torch.Tensor:
        """Y [instr][C][Tf][F] complex64, Tf = num_frames(N) -> [instr][C][N]"""
        dev = self._device()
        cfg = self.config
        Yr = torch.view_as_real(Y.to(dev, torch.complex64).contiguous()).contiguous()
        if tuple(Yr.shape) != (len(cfg.instruments), cfg.n_channels, self.num_frames(N), cfg.F, 2):
            raise ValueError(f"debug_istft: Y has shape {tuple(Y.shape)}")
        out = torch.empty((len(cfg.instruments), cfg.n_channels, int(N)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_debug_istft(self.h, C.c_void_p(Yr.data_ptr()), int(N), C.c_void_p(out.data_ptr()), self._stream(dev)), "etd_sep_debug_istft")
        return out

    def debug_mwf(self, X: torch.Tensor, Y: torch.Tensor, iterations: int) -> torch.Tensor:
        """X [C][Tf][F] complex64, Y [instr][C][Tf][F] complex64 -> Y after ``iterations`` Wiener passes (a new tensor; the stage runs in place on a copy)"""
        dev = self._device()
        cfg = self.config
        iterations = self._check_mwf(iterations)
        if cfg.n_channels > MWF_MAX_CHANNELS:
            raise ValueError(f"debug_mwf: multichannel Wiener filtering takes 1 or {MWF_MAX_CHANNELS} channels, the config has {cfg.n_channels}")
        Xr = torch.view_as_real(X.to(dev, torch.complex64).contiguous()).contiguous()
        Yr = torch.view_as_real(Y.to(dev, torch.complex64).contiguous()).clone()
        Tf = int(X.shape[1])
        if tuple(Xr.shape) != (cfg.n_channels, Tf, cfg.F, 2) or tuple(Yr.shape) != (len(cfg.instruments), cfg.n_channels, Tf, cfg.F, 2) or Tf < 1:
            raise ValueError(f"debug_mwf: X has shape {tuple(X.shape)}, Y {tuple(Y.shape)}")
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sep_debug_mwf(self.h, C.c_void_p(Xr.data_ptr()), C.c_void_p(Yr.data_ptr()), Tf, iterations, self._stream(dev)), "etd_sep_debug_mwf")
        return torch.view_as_complex(Yr)
