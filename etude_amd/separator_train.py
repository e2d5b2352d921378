"""Training of the source separator on the MI355X: ``SeparatorTrainer`` owns fp32 weights, gradients and Adam's two moments on the device
(csrc/separator_train.hip, ``etd_septrain_*``) and hands a trained state to ``StemSeparator``::

    tr = SeparatorTrainer(config, max_units=8, lr=1e-4)
    mix, target = training_segments(tr.to_separator(), mix_wav, stem_wavs)      # magnitude segments, on the device
    for b in range(0, mix.shape[0], 8):
        loss = tr.train_step(mix[b:b + 8], target[:, b:b + 8])
    tr.save("separator.pth"); sep = tr.to_separator()

One call is one batch: every norm uses the batch's statistics, so the ``B`` units of a call must fit ``workspace_bytes`` together (there is no sub-batching).  The loss
is Spleeter's L1 between the softmax estimates ``softmax_i(logits) mix`` and the true magnitudes, modelled on Spleeter and not pinned to it.  ``dropout=p`` drops
the output of the norms of decoder levels 1 .. 3 in every ``loss_and_backward`` call (never in ``loss``) with a counter-based mask that is never stored.  Batches
across a corpus, augmentation, the epoch loop and checkpoints are ``etude_amd.separator_data``'s.  DESIGN.md 4n is the contract; tests/separator_train_np.py and
tests/separator_data_np.py restate it.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import nonneg
from ._trainer import Trainer
from .separator import LEVELS, SeparatorConfig, StemSeparator, check_separator_state, expected_keys, init_separator_state

TRAINABLE = (".weight", ".bias", ".gamma", ".beta")


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class SeparatorTrainer(Trainer):
    """fp32 training of the separator's U-Nets on the GPU.  ``state=None`` draws ``init_separator_state(config, seed)``; otherwise ``state`` is a separator state
    (``expected_keys``).  ``max_units`` bounds the units of one call, ``workspace_bytes`` the device workspace a call may hold (``workspace_total_bytes(B)`` tells
    what ``B`` units need).  ``max_norm=None``: no clipping.  ``dropout`` in [0, 1) is the decoder's drop rate (Spleeter: 0.5; 0 launches nothing), ``dropout_seed`` the
    key of its mask; the mask's call counter travels in ``optimizer_state_dict()["dropout_calls"]``.  Constructing needs no GPU; training does: there is no CPU path."""
    _destroy = "etd_septrain_destroy"
    _abi = "etd_septrain"

    def __init__(self, config: Optional[SeparatorConfig] = None, state: Optional[Dict] = None, seed: int = 0, device: Union[str, torch.device] = "cuda",
                 max_units: int = 8, workspace_bytes: int = 16 << 30, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 max_norm: Optional[float] = None, dropout: float = 0.0, dropout_seed: int = 0):
        self.config = cfg = config or SeparatorConfig()
        cfg.check()
        if workspace_bytes < 1:
            raise ValueError(f"SeparatorTrainer: workspace_bytes must be positive, got {workspace_bytes}")
        ni = len(cfg.instruments)
        if max_units < 1 or max_units * ni > 16384:
            raise ValueError(f"SeparatorTrainer: max_units must be in 1 .. {16384 // ni} for {ni} instruments, got {max_units}")
        if not (lr >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps >= 0):
            raise ValueError(f"SeparatorTrainer: lr and eps must be >= 0 and the betas in [0, 1), got {lr}, {betas}, {eps}")
        if max_norm is not None and not max_norm > 0:
            raise ValueError(f"SeparatorTrainer: max_norm must be positive or None, got {max_norm}")
        if not (0.0 <= float(dropout) < 1.0):
            raise ValueError(f"SeparatorTrainer: dropout must be in [0, 1), got {dropout}")
        if not 0 <= int(dropout_seed) < 2 ** 64:
            raise ValueError(f"SeparatorTrainer: dropout_seed must be in 0 .. 2^64 - 1, got {dropout_seed}")
        if state is None:
            state = init_separator_state(cfg, seed)
        check_separator_state(state, cfg)
        self._shapes = expected_keys(cfg)
        host = {k: np.ascontiguousarray(np.asarray(state[k].detach().cpu() if isinstance(state[k], torch.Tensor) else state[k]), np.float32) for k in self._shapes}
        for k, v in host.items():
            if not np.isfinite(v).all():
                raise ValueError(f"separator state: {k!r} holds a non-finite value")
        self.device = torch.device("cuda" if device == "auto" else device)
        self.max_units, self.workspace_bytes = int(max_units), int(workspace_bytes)
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), max_norm
        self.global_step = 0
        self.dropout, self.dropout_seed = float(dropout), int(dropout_seed)
        ccfg = _lib.SepCfg(n_instr=ni, n_channels=cfg.n_channels, n_fft=cfg.n_fft, hop=cfg.hop, T=cfg.T, F=cfg.F, filters=(C.c_int * LEVELS)(*cfg.conv_n_filters),
                           separation_exponent=int(cfg.separation_exponent), mask_eps=cfg.mask_eps, bn_eps=cfg.bn_eps, workspace_bytes=self.workspace_bytes)
        self._lib = _lib.lib()
        names, ptrs, numels, n, keep = _lib.weights_arrays(host)
        instr = (C.c_char_p * ni)(*[s.encode() for s in cfg.instruments])
        h = C.c_void_p()
        _lib.check(self._lib.etd_septrain_create(C.byref(ccfg), self.max_units, instr, names, ptrs, numels, n, C.byref(h)), "etd_septrain_create")
        del keep
        self._adopt(h)
        if self.dropout > 0.0:      # (at 0 the handle is left as it was created)
            _lib.check(self._lib.etd_septrain_set_dropout(self.h, self.dropout, self.dropout_seed), "etd_septrain_set_dropout")

    @property
    def dropout_calls(self) -> int:
        """the ``loss_and_backward`` calls that dropped so far: the fourth word of the mask's counter"""
        return nonneg(self._lib.etd_septrain_get_dropout_calls(self.h), "etd_septrain_get_dropout_calls")

    # ------------------------------------------------------------------ host arithmetic
    def workspace_total_bytes(self, B: int) -> int:
        return nonneg(self._lib.etd_septrain_workspace_bytes(self.h, int(B)), "etd_septrain_workspace_bytes")

    def step_flops(self, B: int) -> float:
        """convolution FLOPs of one forward + backward of ``B`` units"""
        return float(self._lib.etd_septrain_step_flops(self.h, int(B)))

    # ------------------------------------------------------------------ one batch
    def _batch(self, mix, target) -> Tuple[torch.Tensor, torch.Tensor, int]:
        cfg = self.config
        unit = (cfg.T, cfg.F, cfg.n_channels)
        ms, ts = tuple(getattr(mix, "shape", ())), tuple(getattr(target, "shape", ()))
        if len(ms) != 4 or ms[1:] != unit or ms[0] < 1:
            raise ValueError(f"mix must be [B][T][F][C] = [B]{list(unit)}, got shape {ms}")
        if ts != (len(cfg.instruments),) + ms:
            raise ValueError(f"target must be [I][B][T][F][C] = {[len(cfg.instruments)] + list(ms)}, got shape {ts}")
        if ms[0] > self.max_units:
            raise ValueError(f"a batch of {ms[0]} units, max_units is {self.max_units}")
        dev = self._device()
        mix = torch.as_tensor(mix).detach().to(dev, torch.float32).contiguous()
        target = torch.as_tensor(target).detach().to(dev, torch.float32).contiguous()
        bad = torch.stack([(~torch.isfinite(t)).any() | (t < 0).any() for t in (mix, target)]).tolist()      # (one host synchronisation for the call)
        for name, b in zip(("mix", "target"), bad):
            if b:
                raise ValueError(f"{name} holds a non-finite or negative value")
        return mix, target, ms[0]

    def _run(self, mix, target, loss_scale: float, frozen_stats: bool, backward: bool) -> float:
        mix, target, B = self._batch(mix, target)
        loss = C.c_double()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.etd_septrain_forward_backward(self.h, _p(mix), _p(target), B, float(loss_scale), int(bool(frozen_stats)), int(backward),
                                                               C.byref(loss), self._stream(self.device)), "etd_septrain_forward_backward")
        return float(loss.value)

    def loss_and_backward(self, mix, target, loss_scale: float = 1.0, frozen_stats: bool = False) -> float:
        """forward in training mode and backward of one batch: returns the loss; ``loss_scale`` times its gradient is ADDED to the accumulated gradients.  The
        running statistics move once, unless ``frozen_stats`` (the norms then use them)."""
        return self._run(mix, target, loss_scale, frozen_stats, True)

    def loss(self, mix, target, frozen_stats: bool = True) -> float:
        """the loss alone (by default on the running statistics, as ``StemSeparator`` will use the state); no gradient is touched"""
        return self._run(mix, target, 1.0, frozen_stats, False)

    def _step_call(self, norm_ref, stream) -> None:
        self._call("step", float(self.max_norm or 0.0), self.lr, self.betas[0], self.betas[1], self.eps, norm_ref if self.max_norm else None, stream)

    def step(self) -> Optional[float]:
        """``clip_grad_norm_`` (with ``max_norm``) + ``torch.optim.Adam.step`` + ``zero_grad``.  Returns the gradient norm before clipping, None without clipping."""
        norm = super().step()
        return norm if self.max_norm else None

    def train_step(self, mix, target) -> float:
        """one batch, one optimizer step: the batch's loss before the step"""
        loss = self.loss_and_backward(mix, target)
        self.step()
        return loss

    # ------------------------------------------------------------------ state (the reads and the moments: Trainer; they need no GPU before the first device call)
    def _moment_keys(self):
        return [k for k in self._shapes if k.endswith(TRAINABLE)]

    def state_dict(self) -> "OrderedDict[str, np.ndarray]":
        """the separator state (``expected_keys``), running statistics included"""
        return super().state_dict()

    def grads(self) -> "OrderedDict[str, np.ndarray]":
        """the accumulated gradient of every trainable tensor by its state key"""
        return super().grads()

    def optimizer_state_dict(self) -> Dict[str, object]:
        return dict(super().optimizer_state_dict(), dropout_calls=self.dropout_calls)

    def load_optimizer_state_dict(self, sd: Dict[str, object]) -> None:
        super().load_optimizer_state_dict(sd)
        _lib.check(self._lib.etd_septrain_set_dropout_calls(self.h, int(sd.get("dropout_calls", 0))), "etd_septrain_set_dropout_calls")

    def save(self, path) -> None:
        """what ``load_separator_state`` reads"""
        torch.save({k: torch.from_numpy(v) for k, v in self.state_dict().items()}, str(path))

    def to_separator(self, **kw) -> StemSeparator:
        """a ``StemSeparator`` over a copy of the current state"""
        kw.setdefault("device", self.device)
        return StemSeparator(self.config, self.state_dict(), **kw)

    # ------------------------------------------------------------------ stage taps (include/etude_hip_debug.h); units are [B][I], each with its instrument's weights
    def _enc_shape(self, l: int) -> tuple:
        cfg = self.config
        return (cfg.T >> l, cfg.F >> l, ((cfg.n_channels,) + tuple(cfg.conv_n_filters))[l])

    def _dec_shape(self, j: int) -> tuple:
        cfg = self.config
        return (cfg.T >> (6 - j), cfg.F >> (6 - j), cfg.conv_n_filters[5 - j] if j < LEVELS else 1)

    def debug_dx(self, kind: int, layer: int, dy: torch.Tensor):
        """the input gradient of one layer from dy [B][I][..]: kind 0 encoder (layer 2 .. 6) -> dx; 1 decoder -> (dskip, dup or None); 2 head -> dx"""
        dev = self._device()
        dy = dy.to(dev, torch.float32).contiguous()
        B, I = int(dy.shape[0]), len(self.config.instruments)
        new = lambda shp: torch.empty((B, I) + tuple(shp), dtype=torch.float32, device=dev)      # noqa: E731
        out1 = None
        if kind == 0:
            out0 = new(self._enc_shape(layer - 1))
        elif kind == 1:
            out0 = new(self._enc_shape(7 - layer))
            out1 = new(self._dec_shape(layer - 1)) if layer > 1 else None
        else:
            out0 = new((self.config.T, self.config.F, 1))
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_septrain_debug_dx(self.h, int(kind), int(layer), _p(dy), B, _p(out0), _p(out1), self._stream(dev)), "etd_septrain_debug_dx")
        return (out0, out1) if kind == 1 else out0

    def debug_dw(self, kind: int, layer: int, x0: torch.Tensor, x1: Optional[torch.Tensor], dy: torch.Tensor) -> torch.Tensor:
        """the weight gradient of one layer -> [I][the state tensor's shape]; x0 / x1 / dy are [B][I][..] (encoder 1: x0 is the mix [B][..])"""
        dev = self._device()
        x0, dy = x0.to(dev, torch.float32).contiguous(), dy.to(dev, torch.float32).contiguous()
        x1 = x1.to(dev, torch.float32).contiguous() if x1 is not None else None
        name = self.config.instruments[0]
        shp = self._shapes[f"{name}.head.weight" if kind == 2 else f"{name}.{'conv' if kind == 0 else 'deconv'}{layer}.weight"]
        dw = torch.zeros((len(self.config.instruments),) + tuple(shp), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_septrain_debug_dw(self.h, int(kind), int(layer), _p(x0), _p(x1), _p(dy), int(dy.shape[0]), _p(dw), self._stream(dev)),
                       "etd_septrain_debug_dw")
        return dw

    def debug_norm(self, n: int, x: torch.Tensor, dy: Optional[torch.Tensor] = None):
        """norm n on x [B][I][..] -> (y, stats [2][I][C] = batch mean and biased variance, dx or None)"""
        dev = self._device()
        x = x.to(dev, torch.float32).contiguous()
        dy = dy.to(dev, torch.float32).contiguous() if dy is not None else None
        y, dx = torch.empty_like(x), torch.empty_like(x) if dy is not None else None
        stats = torch.empty((2, len(self.config.instruments), x.shape[-1]), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_septrain_debug_norm(self.h, int(n), _p(x), int(x.shape[0]), _p(dy), _p(y), _p(dx), _p(stats), self._stream(dev)),
                       "etd_septrain_debug_norm")
        return y, stats, dx

    def debug_dropout(self, j: int, y: torch.Tensor, call: int, numel: int = 0) -> torch.Tensor:
        """the mask of decoder level j (1 .. 3) at call counter ``call`` on y [B][I][..]: keep ? y * s : 0.  ``numel`` > 0: only that many leading elements are
        written (a count that is no multiple of 4 ends inside a Philox block); the rest of the result keeps y."""
        dev = self._device()
        y = y.to(dev, torch.float32).contiguous()
        out = y.clone()
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_septrain_debug_dropout(self.h, int(j), _p(y), int(y.shape[0]), int(numel), int(call), _p(out), self._stream(dev)),
                       "etd_septrain_debug_dropout")
        return out

    def debug_loss(self, logits: torch.Tensor, mix: torch.Tensor, target: torch.Tensor, loss_scale: float = 1.0):
        """logits [B][I][T][F][C], mix [B][..], target [I][B][..] -> (loss, dlogits [B][I][..])"""
        dev = self._device()
        logits, mix, target = (t.to(dev, torch.float32).contiguous() for t in (logits, mix, target))
        d = torch.empty_like(logits)
        loss = C.c_double()
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_septrain_debug_loss(self.h, _p(logits), _p(mix), _p(target), int(mix.shape[0]), float(loss_scale), C.byref(loss), _p(d),
                                                         self._stream(dev)), "etd_septrain_debug_loss")
        return float(loss.value), d


def training_segments(separator: StemSeparator, mix_wav, stem_wavs: Sequence) -> Tuple[torch.Tensor, torch.Tensor]:
    """a song's mix [C][N] and its true stems (one [C][N] per instrument, in the config's order) -> (mix [segs][T][F][C], target [I][segs][T][F][C]): the magnitude
    segments of step 2 of DESIGN.md 4m by the separator's own STFT kernel.  The audio and the segments stay on the device."""
    cfg = separator.config
    if len(stem_wavs) != len(cfg.instruments):
        raise ValueError(f"training_segments: {len(stem_wavs)} stems for {len(cfg.instruments)} instruments")
    dev = separator._device()
    lib = _lib.lib()

    def one(i, x):
        shp = separator._song_shape(i, x)
        t = torch.as_tensor(x).detach().to(dev, torch.float32)
        if t.dim() == 1:
            t = t[None]
        if t.shape[0] == 1 and cfg.n_channels > 1:
            t = t.expand(cfg.n_channels, -1)
        return t.contiguous(), shp[-1]

    songs = [one(i, x) for i, x in enumerate([mix_wav] + list(stem_wavs))]
    N = songs[0][1]
    if any(n != N for _, n in songs):
        raise ValueError(f"training_segments: the mix and its stems must have one length, got {[n for _, n in songs]}")
    bad = torch.stack([torch.isfinite(t).all() for t, _ in songs]).logical_not().nonzero().flatten().tolist()      # (one host synchronisation)
    if bad:
        raise ValueError(f"training_segments: {'the mix' if bad[0] == 0 else f'stem {bad[0] - 1}'} holds a non-finite value")
    segs = -(-separator.num_frames(N) // cfg.T)
    out = torch.empty((len(songs), segs, cfg.T, cfg.F, cfg.n_channels), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for k, (t, _) in enumerate(songs):
            _lib.check(lib.etd_sep_magnitudes(separator.h, _p(t), N, _p(out[k]), separator._stream(dev)), "etd_sep_magnitudes")
    return out[0], out[1:]
