"""Training of the Beat-Transformer on the device (csrc/beat_train.hip, ``etd_btrain_*``).

``BeatTrainer`` owns fp32 master weights, gradients and AdamW's two moments on the GPU and mirrors ``DecoderTrainer``::

    tr = BeatTrainer(BeatDetectorModelConfig(), lr=1e-3, pos_weight=(4.0, 12.0))
    losses, norm = tr.train_step([(feats, beat_targets, tempo_targets), ...])      # accumulate over the batches, then one clipped AdamW step
    tr.save("beat.pt"); det = tr.to_detector(tracker="native")

The model is the one ``BeatDetector`` runs (csrc/beat.hip) and the trained arithmetic is the inference arithmetic: there is NO dropout, and a non-zero ``dropout``
is refused.  The loss is this project's own contract, modelled on Beat-Transformer's training script (parity with that script is unpinned)::

    loss = sum_c (1 / n_c) sum_{scored (f, c)} (1 + (pos_weight_c - 1) y) bce_with_logits(z, y)  +  tempo_weight * mean_{songs with a target} -sum_k p_k log_softmax(t)_k

``n_c`` counts the scored cells of class c in the call; a beat target of -1 leaves its (frame, class) cell unscored.  There is no data pipeline, epoch loop or
checkpointing here: batches come from the caller.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import i64
from ._trainer import Trainer
from .beat import BeatDetector, _check_range, expected_keys
from .config import BeatDetectorConfig, BeatDetectorModelConfig

TEMPO_CLASSES = 300


def init_beat_state(config: Optional[BeatDetectorModelConfig] = None, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """A fresh state with the keys and shapes of ``beat.expected_keys``: torch's default initialisers as distributions (uniform(+-1/sqrt(fan_in)) for conv and
    linear weights and biases, xavier-uniform in_proj with zero attention biases, LayerNorm 1 / 0, Er ~ N(0, 1)), drawn from numpy's generator."""
    cfg = config if config is not None else BeatDetectorModelConfig()
    rng = np.random.default_rng(seed)
    shapes = expected_keys(cfg)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in shapes.items():
        if ".norm" in k:
            out[k] = np.ones(shape, np.float32) if k.endswith("weight") else np.zeros(shape, np.float32)
        elif k.endswith("self_attn.Er"):
            out[k] = rng.standard_normal(shape).astype(np.float32)
        elif k.endswith("in_proj_weight"):
            b = math.sqrt(6.0 / (shape[0] + shape[1]))
            out[k] = rng.uniform(-b, b, shape).astype(np.float32)
        elif k.endswith("in_proj_bias") or k.endswith("out_proj.bias"):
            out[k] = np.zeros(shape, np.float32)
        else:
            w_shape = shape if k.endswith("weight") else shapes[k[:-len("bias")] + "weight"]
            b = 1.0 / math.sqrt(int(np.prod(w_shape[1:])))
            out[k] = rng.uniform(-b, b, shape).astype(np.float32)
    return out


def check_beat_train_config(cfg: BeatDetectorModelConfig, dropout: float = 0.0) -> None:
    """The limits of ``etd_btrain_create``, as a ValueError before any GPU is needed."""
    if float(dropout) != 0.0:
        raise ValueError(f"BeatTrainer: dropout = {dropout}; the trained arithmetic is the inference arithmetic -- dropout is not implemented and must be 0")
    if cfg.nhead != 8 or cfg.attn_len != 5 or cfg.dmodel != 256 or not cfg.norm_first:
        raise ValueError("BeatTrainer: nhead = 8, attn_len = 5, dmodel = 256 and norm_first only (the dilated head table is written for them)")
    if not 1 <= cfg.instr <= 8:
        raise ValueError(f"BeatTrainer: instr = {cfg.instr} (1 .. 8)")
    if cfg.d_hid < 256 or cfg.d_hid % 256 or cfg.d_hid > 8192:
        raise ValueError(f"BeatTrainer: d_hid = {cfg.d_hid} (a multiple of 256, <= 8192)")
    if not 1 <= cfg.nlayers <= 16:
        raise ValueError(f"BeatTrainer: nlayers = {cfg.nlayers} (1 .. 16)")
    if not 1 <= cfg.ntoken <= 64:
        raise ValueError(f"BeatTrainer: ntoken = {cfg.ntoken} (1 .. 64)")


def train_cfg(cfg: BeatDetectorModelConfig, max_rows: int, max_seqs: int, tempo_weight: float = 1.0, dropout: float = 0.0) -> "_lib.BeatTrainCfg":
    return _lib.BeatTrainCfg(attn_len=cfg.attn_len, instr=cfg.instr, ntoken=cfg.ntoken, dmodel=cfg.dmodel, nhead=cfg.nhead, d_hid=cfg.d_hid, nlayers=cfg.nlayers,
                             norm_first=1 if cfg.norm_first else 0, n_mels=128, tempo_out=TEMPO_CLASSES, max_rows=int(max_rows), max_seqs=int(max_seqs),
                             tempo_weight=float(tempo_weight), dropout=float(dropout))


def pack_targets(cfg: BeatDetectorModelConfig, Ts: Sequence[int], beat_targets: Sequence, tempo_targets: Optional[Sequence]):
    """per-song targets -> the contiguous host arrays of the C ABI: ``(beat [sum T][ntoken], tempo [n][300], has_tempo [n] int32)``; shapes are checked here, values
    by the library"""
    if len(beat_targets) != len(Ts) or (tempo_targets is not None and len(tempo_targets) != len(Ts)):
        raise ValueError("one beat target (and, if given, one tempo target or None) per song")
    ys = []
    for s, (T, y) in enumerate(zip(Ts, beat_targets)):
        a = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, np.float32)
        if a.shape != (T, cfg.ntoken):
            raise ValueError(f"song {s}: beat target of shape {a.shape}, expected {(T, cfg.ntoken)}")
        ys.append(a)
    tempo = np.zeros((len(Ts), TEMPO_CLASSES), np.float32)
    has = np.zeros(len(Ts), np.int32)
    for s, p in enumerate(tempo_targets or ()):
        if p is None:
            continue
        a = np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p, np.float32)
        if a.shape != (TEMPO_CLASSES,):
            raise ValueError(f"song {s}: tempo target of shape {a.shape}, expected {(TEMPO_CLASSES,)}")
        tempo[s], has[s] = a, 1
    return np.ascontiguousarray(np.concatenate(ys)), tempo, has


class BeatTrainer(Trainer):
    """fp32 training of the Beat-Transformer on the GPU.  ``state=None`` draws ``init_beat_state(config, seed)``; otherwise ``state`` maps the checkpoint's keys to
    arrays or tensors.  ``max_rows`` bounds instr x frames of one ``loss_and_backward`` call and sizes the activation workspace (a call above it is refused)."""
    _destroy = "etd_btrain_destroy"
    _abi = "etd_btrain"

    def __init__(self, config: Optional[BeatDetectorModelConfig] = None, state: Optional[Dict] = None, seed: int = 0, device: Union[str, torch.device] = "cuda",
                 max_rows: int = 5 * 1024, max_seqs: int = 64, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_norm: float = 0.5, pos_weight: Optional[Sequence[float]] = None, tempo_weight: float = 1.0, dropout: float = 0.0):
        self.config = config if config is not None else BeatDetectorModelConfig()
        check_beat_train_config(self.config, dropout)
        self.lr, self.betas, self.eps, self.weight_decay, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay), float(max_norm)
        self.max_rows, self.max_seqs = int(max_rows), int(max_seqs)
        self.pos_weight = np.ones(self.config.ntoken, np.float32) if pos_weight is None else np.ascontiguousarray(pos_weight, np.float32)
        if self.pos_weight.shape != (self.config.ntoken,):
            raise ValueError(f"pos_weight needs {self.config.ntoken} entries")
        self.tempo_weight = float(tempo_weight)
        self._shapes = OrderedDict(expected_keys(self.config))
        if state is None:
            state = init_beat_state(self.config, seed)
        sd = {}
        for k, shape in self._shapes.items():
            if k not in state:
                raise ValueError(f"state lacks '{k}'")
            v = state[k]
            sd[k] = np.ascontiguousarray(v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32))
            if sd[k].shape != tuple(shape):
                raise ValueError(f"state['{k}'] has shape {sd[k].shape}, expected {tuple(shape)}")
        if device == "auto":
            device = "cuda"
        self.device = torch.device(device)
        self._device()
        self._cfg = train_cfg(self.config, self.max_rows, self.max_seqs, self.tempo_weight, dropout)
        names, ptrs, numels, n, keep = _lib.weights_arrays(sd)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().etd_btrain_create(C.byref(self._cfg), names, ptrs, numels, n, self.pos_weight.ctypes.data, C.byref(h)), "etd_btrain_create")
        del keep
        self._adopt(h)
        self.global_step = 0
        self._last = (0, 0)      # rows, frames of the last batch that ran

    # ------------------------------------------------------------------ one batch
    def _songs_to_device(self, feats: Sequence) -> Tuple[torch.Tensor, List[int]]:
        ts = []
        for i, f in enumerate(feats):
            t = torch.as_tensor(f)
            if t.dim() != 3 or t.shape[0] != self.config.instr or t.shape[2] != 128 or t.shape[1] < 1:
                raise ValueError(f"song {i}: features must be [instr={self.config.instr}][T >= 1][128], got {tuple(t.shape)}")
            _check_range(t, f"song {i}")
            ts.append(t)
        return torch.cat([t.to(torch.float32).reshape(-1) for t in ts]).to(self.device).contiguous(), [int(t.shape[1]) for t in ts]

    def loss_and_backward(self, feats: Sequence, beat_targets: Sequence, tempo_targets: Optional[Sequence] = None, loss_scale: float = 1.0) -> Tuple[float, int, bool]:
        """Forward, loss and backward of one ragged batch: ``(loss_scale * loss, scored beat cells, skipped)``; ``loss_scale`` times the gradient is added to the
        accumulated gradients.  A batch with no scored cell and no tempo target has loss nan, is skipped and launches nothing."""
        if len(feats) == 0:
            return float("nan"), 0, True
        Ts = [int(np.shape(f)[1]) if len(np.shape(f)) == 3 else -1 for f in feats]
        y, tempo, has = pack_targets(self.config, Ts, beat_targets, tempo_targets)
        feat, Ts = self._songs_to_device(feats)
        loss, n_scored, skipped = C.c_float(), C.c_int32(), C.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().etd_btrain_loss_backward(self.h, C.c_void_p(feat.data_ptr()), len(Ts), i64(Ts), y.ctypes.data, tempo.ctypes.data, has.ctypes.data,
                                                           float(loss_scale), C.byref(loss), C.byref(n_scored), C.byref(skipped), self._stream(self.device)),
                       "etd_btrain_loss_backward")
        if not skipped.value:
            self._last = (self.config.instr * sum(Ts), sum(Ts))
        return float(loss.value), int(n_scored.value), bool(skipped.value)

    def _step_call(self, norm_ref, stream) -> None:
        self._call("step", self.max_norm, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, norm_ref, stream)

    def step(self) -> float:
        """``clip_grad_norm_`` + ``AdamW.step`` + ``zero_grad``, as ``DecoderTrainer.step``.  Returns the gradient norm before clipping."""
        return super().step()

    def train_step(self, batches: Sequence[Tuple]) -> Tuple[List[float], float]:
        """Each batch is ``(feats, beat_targets)`` or ``(feats, beat_targets, tempo_targets)``; their gradients are accumulated with ``loss_scale = 1 / len(batches)``,
        then one optimizer step: ``(the batches' unscaled losses, gradient norm before clipping)``."""
        if len(batches) < 1:
            raise ValueError("train_step needs at least one batch")
        k = len(batches)
        losses = [self.loss_and_backward(*b, loss_scale=1.0 / k)[0] * k for b in batches]
        return losses, self.step()

    # ------------------------------------------------------------------ state (state_dict, grads and the optimizer's state: Trainer)
    def _write_entry(self, second: int):
        return "write", (2 + second,)

    def debug_read_rows(self, what: int) -> np.ndarray:
        """test hook (etd_debug_btrain_read_rows): per-row results of the last ``loss_and_backward`` that ran -- 0: the gradient of the front end's tokens
        [rows][256], 1: the logits [frames][ntoken], 2: the gradient of conv1's pooled output [rows][1344]"""
        rows, frames = self._last
        shape = ((rows, 256), (frames, self.config.ntoken), (rows, 42 * 32))[what]
        a = np.empty(shape, np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().etd_debug_btrain_read_rows(self.h, int(what), a.ctypes.data, a.size, self._stream(self.device)), "etd_debug_btrain_read_rows")
        return a

    def workspace_bytes(self) -> int:
        return int(_lib.lib().etd_btrain_bytes(self.h, 0))

    def save(self, path: Union[str, Path]) -> None:
        """``{"state_dict": ...}``: what ``beat.load_state_dict`` (and the reference's BeatDetector) reads"""
        torch.save({"state_dict": OrderedDict((k, torch.from_numpy(v)) for k, v in self.state_dict().items())}, str(path))

    def to_detector(self, detector_config: Optional[BeatDetectorConfig] = None, **kwargs) -> BeatDetector:
        """An inference ``BeatDetector`` over a copy of the current weights, with no file in between"""
        cfg = detector_config if detector_config is not None else BeatDetectorConfig(model=self.config)
        return BeatDetector(cfg, device=self.device, state_dict=self.state_dict(), **kwargs)
