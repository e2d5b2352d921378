"""What every batch engine's Python side shares: the owner of one C handle (``Engine``), the ctypes array builders, and the upload-and-check of mono songs.
DESIGN.md "The engine skeleton" says what a new engine inherits and what it writes itself."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import torch

from . import _lib


class Engine:
    """Owns ``self.h``, one handle of the C ABI.  A subclass names its destroy symbol in ``_destroy``, sets ``self.device`` and, after a successful create, calls
    ``self._adopt(h)``."""
    _destroy = ""

    def _adopt(self, h: C.c_void_p) -> None:
        self._destroy_fn = getattr(_lib.lib(), self._destroy)
        self.h = h

    @property
    def _h(self):
        """read-only: the handle under the name ``FrontEnd``, ``DTWEngine`` and others gave it before they shared this base, for callers written against that name
        (the GPU tests of the commit before this one read ``fe._h`` / ``eng._h`` and must pass on this library too).  Engines write ``self._adopt(h)``, never ``_h``."""
        return self.h

    def close(self) -> None:
        """idempotent; harmless on an object whose ``__init__`` raised before ``_adopt``"""
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self._destroy_fn(h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001  (interpreter shutdown: the library or this module may already be gone)
            pass

    def _device(self) -> torch.device:
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.EtudeHipError(f"etude_amd.{type(self).__name__} needs a ROCm GPU (device='cuda'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _stream(self, dev) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def i64(xs):
    return (C.c_int64 * len(xs))(*[int(x) for x in xs])


def i32(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def nonneg(rc: int, what: str) -> int:
    """a ``*_bytes`` / ``*_frames`` result: the value, or the library's error for a negative one"""
    if rc < 0:
        _lib.check(rc, what)
    return int(rc)


def hold(tensors, dev) -> None:
    """an uploaded copy may be freed right after the call that read it: its memory stays valid for the work queued on this stream"""
    st = torch.cuda.current_stream(dev)
    for t in tensors:
        t.record_stream(st)


def mono_songs_to_device(wavs: Sequence, dev, min_n: int, max_n: int, short_msg: str = "") -> List[torch.Tensor]:
    """the input checks of a batch of mono songs (1-d, min_n <= N <= max_n, finite with ONE host synchronisation) -> contiguous float32 tensors on ``dev()``.
    dev: a callable (an engine's ``_device``), asked only once every shape has passed.  short_msg: what "song i: N = n" is followed by for a song below min_n;
    without one such a song is refused with the shape message."""
    need = "[N]" if short_msg else f"[N >= {min_n}]"
    for i, x in enumerate(wavs):
        shp = tuple(x.shape) if hasattr(x, "shape") else None
        if shp is None or len(shp) != 1 or (shp[0] < min_n and not short_msg):
            raise ValueError(f"song {i}: need mono samples {need}, got shape {shp}")
        if shp[0] < min_n:
            raise ValueError(f"song {i}: N = {shp[0]} {short_msg}")
        if shp[0] > max_n:
            raise ValueError(f"song {i}: N = {shp[0]} is above the engine's {max_n} samples")
    dev = dev()
    songs = [torch.as_tensor(x).detach().to(dev, torch.float32).contiguous() for x in wavs]
    bad = torch.stack([torch.isfinite(t).all() for t in songs]).logical_not().nonzero().flatten().tolist()      # (one host synchronisation for the call)
    if bad:
        raise ValueError(f"song {bad[0]}: holds a non-finite sample")
    return songs
