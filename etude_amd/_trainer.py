"""What every trainer's Python side shares (``Trainer``): the optimizer front and the host's access to the flat parameter, gradient and moment buffers of one
``etd_*train`` handle.  DESIGN.md 4a ("trainer skeleton") says what a new trainer inherits and what it writes itself."""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import numpy as np
import torch

from . import _lib
from ._engine import Engine


class Trainer(Engine):
    """An ``Engine`` over a training handle.  A subclass names its symbol prefix in ``_abi`` (``etd_btrain``: ``etd_btrain_zero_grad``, ...), fills ``self._shapes``
    (state key -> shape), sets ``self.global_step = 0`` and writes ``_step_call(norm_ref, stream)``, its clip-and-step entry with its hyper-parameters; where its
    C ABI spells the read and write entries differently from ``read(key, which, ...)`` / ``write_moment(key, second, ...)`` it overrides ``_read_entry`` /
    ``_write_entry``."""
    _abi = ""

    def _call(self, name: str, *args) -> None:
        _lib.check(getattr(_lib.lib(), f"{self._abi}_{name}")(self.h, *args), f"{self._abi}_{name}")

    @contextlib.contextmanager
    def _launch(self, host_ok: bool = False):
        """the device context of one call; yields its stream.  ``host_ok``: without a GPU, yield None instead of raising (an entry that is answered on the host)"""
        if host_ok and not (self.device.type == "cuda" and torch.cuda.is_available()):
            yield None
            return
        dev = self._device()
        with torch.cuda.device(dev):
            yield self._stream(dev)

    # ------------------------------------------------------------------ the optimizer
    def zero_grad(self) -> None:
        with self._launch() as st:
            self._call("zero_grad", st)

    def grad_norm(self) -> float:
        v = C.c_double()
        with self._launch() as st:
            self._call("grad_norm", C.byref(v), st)
        return float(v.value)

    def step(self) -> float:
        """clip, the optimizer's step, ``zero_grad``.  Returns the gradient norm before clipping."""
        v = C.c_double()
        with self._launch() as st:
            self._step_call(C.byref(v), st)
        self.global_step += 1
        self.zero_grad()
        return float(v.value)

    # ------------------------------------------------------------------ state
    def _read_entry(self, which: int) -> Tuple[str, tuple]:
        """(entry, the arguments between the key and the buffer) that reads buffer ``which``: 0 state, 1 gradient, 2 exp_avg, 3 exp_avg_sq"""
        return "read", (which,)

    def _write_entry(self, second: int) -> Tuple[str, tuple]:
        """... that writes exp_avg (``second`` = 0) or exp_avg_sq (1)"""
        return "write_moment", (second,)

    def _moment_keys(self) -> Iterable[str]:      # the keys that have a gradient and moments
        return self._shapes

    def _read(self, which: int, keys: Iterable[str]) -> "OrderedDict[str, np.ndarray]":
        entry, mid = self._read_entry(which)
        out = OrderedDict()
        with self._launch(host_ok=True) as st:      # (an engine that is constructed without a GPU answers reads from the host's copy until its first device call)
            for k in keys:
                a = np.empty(self._shapes[k], np.float32)
                self._call(entry, k.encode(), *mid, a.ctypes.data, a.size, st)
                out[k] = a
        return out

    def state_dict(self) -> "OrderedDict[str, np.ndarray]":
        return self._read(0, self._shapes)

    def grads(self) -> "OrderedDict[str, np.ndarray]":
        return self._read(1, self._moment_keys())

    def optimizer_state_dict(self) -> Dict[str, object]:
        return {"step": self.global_step, "exp_avg": self._read(2, self._moment_keys()), "exp_avg_sq": self._read(3, self._moment_keys())}

    def load_optimizer_state_dict(self, sd: Dict[str, object]) -> None:
        with self._launch() as st:
            for second, key in ((0, "exp_avg"), (1, "exp_avg_sq")):
                entry, mid = self._write_entry(second)
                for k in self._moment_keys():
                    a = np.ascontiguousarray(sd[key][k], np.float32)
                    if a.shape != tuple(self._shapes[k]):
                        raise ValueError(f"{key}['{k}'] has shape {a.shape}, expected {tuple(self._shapes[k])}")
                    self._call(entry, k.encode(), *mid, a.ctypes.data, a.size, st)
            self._call("set_step", int(sd["step"]))
        self.global_step = int(sd["step"])
