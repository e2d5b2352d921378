"""Training data and the training loop of the source separator on the MI355X: ``SegmentSampler`` keeps the magnitudes of every track of a corpus on the device
(csrc/separator_data.hip, ``etd_sepdata_*``) and cuts augmented batches from them in one launch; ``fit`` runs epochs of them through a ``SeparatorTrainer``::

    tr = SeparatorTrainer(config, max_units=8, lr=1e-4, dropout=0.5)
    sampler = SegmentSampler(config, seed=0)
    for stems in corpus:                                   # one [C][N] array per instrument, in the config's order; the audio is uploaded once and dropped
        sampler.add_track(stems)
    held_out = sampler.draw(8, epoch=10 ** 6, index=0, augment=False)
    cursor = fit(tr, sampler, epochs=10, steps_per_epoch=1000, batch_units=8, on_step=lambda e, s, loss: ...)
    print(validate(tr, sampler, held_out)); save_checkpoint("sep.ckpt", tr, *cursor)
    tr, cursor = load_checkpoint("sep.ckpt")               # ... and fit(tr, sampler, ..., start=cursor) goes on with the bits of an uninterrupted run

A unit is a draw ``(track, t0, a, q)``: the start frame, the time-stretch factor and the frequency factor ``q = 2 ** (semitones / 12)``, after Spleeter's random time
crop, time stretch and pitch shift of the spectrograms.  The draws are made on the host (``draw``) or passed in (``batch``); the device never sees a random number,
and no segment visits the host.  Modelled on Spleeter's dataset.py and not pinned to it.  DESIGN.md 4o is the contract; tests/separator_data_np.py restates it.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, nonneg
from .separator import LEVELS, SeparatorConfig, StemSeparator
from .separator_train import SeparatorTrainer

Draw = Tuple[int, int, float, float]


def stretched_sizes(T: int, F: int, a: float, q: float) -> Tuple[int, int]:
    """(T', F') = (floor(T a), floor(F q)), the products formed in double"""
    return int(math.floor(T * float(a))), int(math.floor(F * float(q)))


def check_draws(draws: Sequence[Draw], frames: Sequence[int], T: int, F: int) -> None:
    """ValueError naming the first unit whose draw lies outside its track (``frames[k]`` = Tf of track k) or shrinks an axis below two points"""
    if len(draws) < 1:
        raise ValueError("a batch needs at least one draw")
    for u, d in enumerate(draws):
        if len(d) != 4:
            raise ValueError(f"unit {u}: a draw is (track, t0, a, q), got {d!r}")
        k, t0, a, q = d
        if int(k) != k or not 0 <= k < len(frames):
            raise ValueError(f"unit {u}: track {k}, the sampler holds {len(frames)}")
        if int(t0) != t0 or not 0 <= t0 < frames[int(k)]:
            raise ValueError(f"unit {u}: t0 = {t0} outside 0 .. {frames[int(k)] - 1} of track {k}")
        if not (math.isfinite(a) and math.isfinite(q) and 0.0 < a <= 64.0 and 0.0 < q <= 64.0):
            raise ValueError(f"unit {u}: a = {a} and q = {q} must be finite and in (0, 64]")
        Tp, Fp = stretched_sizes(T, F, a, q)
        if Tp < 2:
            raise ValueError(f"unit {u}: T' = floor({T} x {a}) = {Tp} is below 2")
        if Fp < 2:
            raise ValueError(f"unit {u}: F' = floor({F} x {q}) = {Fp} is below 2")


def _range(name: str, r) -> Optional[Tuple[float, float]]:
    if r is None:
        return None
    lo, hi = float(r[0]), float(r[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"SegmentSampler: {name} must be None or a finite (low, high) with low <= high, got {r}")
    return lo, hi


class SegmentSampler(Engine):
    """Tracks -> training batches ``(mix [B][T][F][C], target [I][B][T][F][C])`` on the device, the shapes ``SeparatorTrainer`` takes.

    ``stretch`` is the range of the time-stretch factor, ``pitch`` the range of the shift in semitones; either may be ``None`` (identity).  ``max_bytes`` bounds
    the device memory of the tracks' magnitudes: a track that does not fit is refused with the bytes it needs.  A unit's output depends on its draw and its track
    alone, not on the batch around it.  Constructing needs no GPU; adding a track does: there is no CPU path."""
    _destroy = "etd_sepdata_destroy"

    def __init__(self, config: Optional[SeparatorConfig] = None, seed: int = 0, stretch: Optional[Tuple[float, float]] = (0.9, 1.1),
                 pitch: Optional[Tuple[float, float]] = (-1.0, 1.0), device: Union[str, torch.device] = "cuda", max_bytes: int = 16 << 30):
        self.config = cfg = config or SeparatorConfig()
        cfg.check()
        if max_bytes < 1:
            raise ValueError(f"SegmentSampler: max_bytes must be positive, got {max_bytes}")
        if int(seed) != seed or seed < 0:
            raise ValueError(f"SegmentSampler: seed must be a non-negative integer, got {seed}")
        self.seed, self.stretch, self.pitch = int(seed), _range("stretch", stretch), _range("pitch", pitch)
        if self.stretch is not None and not self.stretch[0] > 0:
            raise ValueError(f"SegmentSampler: stretch factors must be positive, got {stretch}")
        self.device = torch.device("cuda" if device == "auto" else device)
        self.max_bytes = int(max_bytes)
        self.frames: List[int] = []                    # Tf of every track
        self._stft: Optional[StemSeparator] = None
        self._lib = _lib.lib()
        ccfg = _lib.SepDataCfg(n_instr=len(cfg.instruments), n_channels=cfg.n_channels, T=cfg.T, F=cfg.F, max_bytes=self.max_bytes)
        h = C.c_void_p()
        _lib.check(self._lib.etd_sepdata_create(C.byref(ccfg), C.byref(h)), "etd_sepdata_create")
        self._adopt(h)

    def close(self) -> None:
        if getattr(self, "_stft", None) is not None:
            self._stft.close()
            self._stft = None
        super().close()

    # ------------------------------------------------------------------ host arithmetic
    @property
    def num_tracks(self) -> int:
        return len(self.frames)

    @property
    def held_bytes(self) -> int:
        return nonneg(self._lib.etd_sepdata_bytes(self.h), "etd_sepdata_bytes")

    def track_bytes(self, Tf: int) -> int:
        return nonneg(self._lib.etd_sepdata_track_bytes(self.h, int(Tf)), "etd_sepdata_track_bytes")

    def _front(self) -> StemSeparator:
        """the STFT of ``training_segments``: a separator of this config with one filter per level (its U-Nets never run)"""
        if self._stft is None:
            cfg = dataclasses.replace(self.config, conv_n_filters=(1,) * LEVELS)
            self._stft = StemSeparator(cfg, seed=0, device=self.device)
        return self._stft

    # ------------------------------------------------------------------ tracks
    def add_track(self, stem_wavs: Sequence, mix_wav=None) -> int:
        """one [C][N] (or mono [N]) per instrument, in the config's order, host or device; ``mix_wav=None``: the mix is the fp32 sum of the stems in instrument
        order, formed on the device.  Returns the track's id.  The magnitudes stay on the device, the audio is dropped."""
        cfg, k = self.config, len(self.frames)
        ni, nc = len(cfg.instruments), cfg.n_channels
        if len(stem_wavs) != ni:
            raise ValueError(f"track {k}: {len(stem_wavs)} stems for {ni} instruments")
        wavs = list(stem_wavs) + ([mix_wav] if mix_wav is not None else [])
        what = [f"stem {i}" for i in range(ni)] + ["the mix"]
        front = self._front()
        try:
            Ns = [front._song_shape(i, x)[-1] for i, x in enumerate(wavs)]
        except ValueError as e:
            raise ValueError(f"track {k}: {e}") from None
        if any(n != Ns[0] for n in Ns):
            raise ValueError(f"track {k}: the stems{' and the mix' if mix_wav is not None else ''} must have one length, got {Ns}")
        N = Ns[0]
        dev = self._device()

        def up(x):
            t = torch.as_tensor(x).detach().to(dev, torch.float32)
            if t.dim() == 1:
                t = t[None]
            if t.shape[0] == 1 and nc > 1:
                t = t.expand(nc, -1)
            return t.contiguous()

        songs = [up(x) for x in wavs]
        bad = torch.stack([torch.isfinite(t).all() for t in songs]).logical_not().nonzero().flatten().tolist()      # (one host synchronisation)
        if bad:
            raise ValueError(f"track {k}: {what[bad[0]]} holds a non-finite value")
        Tf = front.num_frames(N)
        with torch.cuda.device(dev):
            st = self._stream(dev)
            if mix_wav is None:
                mix = torch.empty_like(songs[0])
                ptrs = (C.c_void_p * ni)(*[t.data_ptr() for t in songs])
                _lib.check(self._lib.etd_sepdata_sum_stems(self.h, ptrs, nc * N, C.c_void_p(mix.data_ptr()), st), "etd_sepdata_sum_stems")
            else:
                mix = songs[ni]
            mag, tid = C.c_void_p(), C.c_int()
            _lib.check(self._lib.etd_sepdata_add_track(self.h, Tf, C.byref(mag), C.byref(tid)), "etd_sepdata_add_track")
            self.frames.append(Tf)
            per = -(-Tf // cfg.T) * cfg.T * cfg.F * nc * 4
            for j, t in enumerate([mix] + songs[:ni]):
                _lib.check(self._lib.etd_sep_magnitudes(front.h, C.c_void_p(t.data_ptr()), N, C.c_void_p(mag.value + j * per), st), "etd_sep_magnitudes")
            torch.cuda.current_stream(dev).synchronize()      # the audio is dropped on return
        return int(tid.value)

    # ------------------------------------------------------------------ draws
    def draw(self, B: int, epoch: int, index: int, augment: bool = True) -> List[Draw]:
        """``B`` draws from ``numpy.random.default_rng([seed, epoch, index])``, unit by unit in the order track (uniform over the tracks), t0 (uniform in
        0 .. max(0, Tf - T)), a (uniform in ``stretch``), semitones (uniform in ``pitch``).  ``augment=False``: a = q = 1, the same tracks and starts."""
        if not self.frames:
            raise ValueError("SegmentSampler.draw: the sampler holds no track")
        if B < 1 or epoch < 0 or index < 0:
            raise ValueError(f"SegmentSampler.draw: B >= 1 and epoch, index >= 0, got {B}, {epoch}, {index}")
        rng = np.random.default_rng([self.seed, int(epoch), int(index)])
        out = []
        for _ in range(B):
            k = int(rng.integers(len(self.frames)))
            t0 = int(rng.integers(0, max(0, self.frames[k] - self.config.T) + 1))
            a = float(rng.uniform(*self.stretch)) if self.stretch is not None else 1.0
            q = float(2.0 ** (rng.uniform(*self.pitch) / 12.0)) if self.pitch is not None else 1.0
            out.append((k, t0, a, q) if augment else (k, t0, 1.0, 1.0))
        return out

    def batch(self, draws: Sequence[Draw]) -> Tuple[torch.Tensor, torch.Tensor]:
        """explicit draws -> (mix [B][T][F][C], target [I][B][T][F][C]) on the device, all units in one launch"""
        cfg = self.config
        check_draws(draws, self.frames, cfg.T, cfg.F)
        dev = self._device()
        B, ni = len(draws), len(cfg.instruments)
        mix = torch.empty((B, cfg.T, cfg.F, cfg.n_channels), dtype=torch.float32, device=dev)
        target = torch.empty((ni,) + tuple(mix.shape), dtype=torch.float32, device=dev)
        track = (C.c_int32 * B)(*[int(d[0]) for d in draws])
        t0 = (C.c_int64 * B)(*[int(d[1]) for d in draws])
        a = (C.c_double * B)(*[float(d[2]) for d in draws])
        q = (C.c_double * B)(*[float(d[3]) for d in draws])
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_sepdata_gather(self.h, B, track, t0, a, q, C.c_void_p(mix.data_ptr()), C.c_void_p(target.data_ptr()), self._stream(dev)),
                       "etd_sepdata_gather")
        return mix, target


# ---------------------------------------------------------------------------------------------- the loop
def fit(trainer: SeparatorTrainer, sampler: SegmentSampler, epochs: int, steps_per_epoch: int, batch_units: int, accumulate: int = 1,
        on_step: Optional[Callable[[int, int, float], None]] = None, start: Tuple[int, int] = (0, 0)) -> Tuple[int, int]:
    """Optimizer steps ``start = (epoch, step)`` up to ``(epochs, 0)``: step ``s`` of epoch ``e`` draws the batches ``(e, s * accumulate + k)``, k < ``accumulate``,
    adds each one's gradient with ``loss_scale = 1 / accumulate`` and steps once.  ``on_step(e, s, loss)`` gets the mean loss of the step's batches.  Returns the
    cursor of the next step, what ``save_checkpoint`` stores: a run resumed from it continues with the bits of an uninterrupted one."""
    if epochs < 0 or steps_per_epoch < 1 or batch_units < 1 or accumulate < 1:
        raise ValueError(f"fit: epochs >= 0 and steps_per_epoch, batch_units, accumulate >= 1, got {epochs}, {steps_per_epoch}, {batch_units}, {accumulate}")
    e0, s0 = int(start[0]), int(start[1])
    if e0 < 0 or not 0 <= s0 < steps_per_epoch:
        raise ValueError(f"fit: start = {start} is not an (epoch >= 0, step in 0 .. {steps_per_epoch - 1})")
    for e in range(e0, epochs):
        for s in range(s0 if e == e0 else 0, steps_per_epoch):
            loss = 0.0
            for k in range(accumulate):
                mix, target = sampler.batch(sampler.draw(batch_units, e, s * accumulate + k))
                loss += trainer.loss_and_backward(mix, target, loss_scale=1.0 / accumulate)
            trainer.step()
            if on_step is not None:
                on_step(e, s, loss / accumulate)
    return (epochs, 0) if e0 < epochs else (e0, s0)


def validate(trainer: SeparatorTrainer, sampler: SegmentSampler, draws: Sequence[Draw]) -> float:
    """the mean ``trainer.loss()`` (running statistics, no dropout) over un-augmented draws, in batches of at most ``trainer.max_units``"""
    if any(d[2] != 1.0 or d[3] != 1.0 for d in draws):
        raise ValueError("validate: the draws must be un-augmented (a = q = 1); sampler.draw(..., augment=False) makes such")
    tot = 0.0
    for b in range(0, len(draws), trainer.max_units):
        part = draws[b:b + trainer.max_units]
        mix, target = sampler.batch(part)
        tot += trainer.loss(mix, target) * len(part)
    return tot / len(draws)


_HYPER = ("max_units", "workspace_bytes", "lr", "betas", "eps", "max_norm", "dropout", "dropout_seed")


def save_checkpoint(path, trainer: SeparatorTrainer, epoch: int, step: int) -> None:
    """the state, the optimizer's state (moments, step and the dropout counter), the trainer's config and hyperparameters and the cursor ``(epoch, step)``"""
    opt = trainer.optimizer_state_dict()
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}      # noqa: E731
    torch.save({"format": "etude_amd.separator_checkpoint.1", "config": dataclasses.asdict(trainer.config),
                "hyper": {k: getattr(trainer, k) for k in _HYPER}, "state": t(trainer.state_dict()),
                "optimizer": {"step": int(opt["step"]), "dropout_calls": int(opt["dropout_calls"]), "exp_avg": t(opt["exp_avg"]), "exp_avg_sq": t(opt["exp_avg_sq"])},
                "cursor": (int(epoch), int(step))}, str(path))


def read_checkpoint(path) -> dict:
    """what ``save_checkpoint`` wrote, the arrays as float32 numpy arrays and the config as a ``SeparatorConfig``; needs no GPU"""
    ck = torch.load(str(path), map_location="cpu")
    if not isinstance(ck, dict) or ck.get("format") != "etude_amd.separator_checkpoint.1":
        raise ValueError(f"{path}: not a separator training checkpoint")
    n = lambda d: {k: np.ascontiguousarray(v.numpy(), np.float32) for k, v in d.items()}      # noqa: E731
    cfg = dict(ck["config"])
    cfg["instruments"], cfg["conv_n_filters"] = tuple(cfg["instruments"]), tuple(cfg["conv_n_filters"])
    hyper = dict(ck["hyper"])
    hyper["betas"] = tuple(hyper["betas"])
    opt = ck["optimizer"]
    return {"config": SeparatorConfig(**cfg), "hyper": hyper, "state": n(ck["state"]),
            "optimizer": {"step": int(opt["step"]), "dropout_calls": int(opt.get("dropout_calls", 0)), "exp_avg": n(opt["exp_avg"]), "exp_avg_sq": n(opt["exp_avg_sq"])},
            "cursor": (int(ck["cursor"][0]), int(ck["cursor"][1]))}


def load_checkpoint(path, device: Union[str, torch.device] = "cuda", **overrides) -> Tuple[SeparatorTrainer, Tuple[int, int]]:
    """-> (a trainer as the saved one was: state, moments, step, dropout counter and hyperparameters; the cursor to pass to ``fit`` as ``start``).  ``overrides``
    replace saved hyperparameters (``lr=...``)."""
    ck = read_checkpoint(path)
    hyper = dict(ck["hyper"], **overrides)
    tr = SeparatorTrainer(ck["config"], ck["state"], device=device, **hyper)
    tr.load_optimizer_state_dict(ck["optimizer"])
    return tr, ck["cursor"]
