"""Notes to audio on the MI355X: ``NoteRenderer`` -- a ragged batch of note lists -> mono float32 waveforms (22 050 Hz by default) of this project's own piano
voice, laid out so that ``AlignFeatures.features_many`` consumes them without a host copy.  It closes the loop from ``ClipBatchPipeline`` / ``generate_many`` (note
arrays) to WPD, the alignment metric, which needs the cover as audio.

The voice (``PianoVoice``: inharmonic partials, per-partial exponential decay, a 4 ms attack, a release of finite support) is a contract of this project, DESIGN.md
4l, restated in fp64 numpy in tests/render_np.py.  Parity with ``pretty_midi.synthesize`` or a SoundFont player is not claimed: the reference never rendered its
covers itself.  csrc/render.hip: gather, one workgroup per 1 024 samples, the phase in fp64, everything else fp32, no atomics.
"""
from __future__ import annotations

import ctypes as C
import json
import math
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, nonneg

NOTE_DTYPE = np.dtype([("onset", "<f8"), ("offset", "<f8"), ("pitch", "<i4"), ("velocity", "<i4")])   # == etd_note (extractor.NOTE_DTYPE)
DEFAULT_WORKSPACE_BUDGET = 8 << 30
ALIGN = 64          # RN_ALIGN of csrc/render.h: a cover's first sample in its flat buffer is a multiple of this many floats


@dataclass(frozen=True)
class PianoVoice:
    """Every parameter of the voice; the defaults are the contract the tests use."""
    partials: int = 8                   # K: partials k = 1 .. K, at most 16
    inharmonicity: float = 3.5e-4       # B at pitch 60; f_k = k f0 sqrt(1 + B k^2)
    inharmonicity_step: float = 10.0    # B doubles every so many semitones
    partial_rolloff: float = 1.5        # A_k = (velocity / 127)^velocity_power k^-partial_rolloff
    velocity_power: float = 2.0
    attack: float = 0.004               # s: min(tau / attack, 1)
    decay_base: float = 3.0             # s: T at pitch 21
    decay_halving: float = 24.0         # T halves every so many semitones
    decay_partial: float = 0.25         # T_k = T / (1 + decay_partial (k - 1))
    release_tau: float = 0.06           # s: behind the offset, exp(-u / release_tau) (1 - u / release_len)
    release_len: float = 0.48           # s: R; a note is exactly 0 from offset + R on
    gain: float = 0.1
    nyquist_fraction: float = 0.45      # a partial with f_k >= nyquist_fraction * sr does not exist
    decay: bool = True                  # False: no exp(-tau / T_k)
    release: bool = True                # False: a note ends at its offset (R = 0)

    @property
    def support(self) -> float:
        """R: seconds a note sounds behind its offset"""
        return float(self.release_len) if self.release else 0.0


def limits() -> dict:
    """Host only: the constants of the built library"""
    a, p, c, b = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    s = C.c_longlong()
    _lib.check(_lib.lib().etd_render_limits(C.byref(a), C.byref(s), C.byref(p), C.byref(c), C.byref(b)), "etd_render_limits")
    return dict(max_notes=a.value, max_samples=s.value, max_partials=p.value, max_covers=c.value, block=b.value)


def num_samples_for(notes: np.ndarray, sample_rate: int, voice: PianoVoice = PianoVoice()) -> int:
    """N = ceil((max offset + R) sr) + 1; 0 for a cover with no notes"""
    if len(notes) == 0:
        return 0
    return int(math.ceil((float(np.max(notes["offset"])) + voice.support) * sample_rate)) + 1


def as_note_array(x) -> np.ndarray:
    """A cover in any accepted form -> a NOTE_DTYPE array in the caller's order: a NOTE_DTYPE array (what ``notes_stage`` and ``extract`` produce), a list of
    {onset, offset, pitch, velocity} dicts (the ``extract.json`` form), or a ``.json`` / ``.mid`` path."""
    if isinstance(x, (str, Path)):
        p = Path(x)
        if p.suffix.lower() == ".mid":
            from .rhythm import read_midi_notes
            return read_midi_notes(p)
        if p.suffix.lower() == ".json":
            with open(p, "r", encoding="utf-8") as f:
                return as_note_array(json.load(f))
        raise ValueError(f"{p}: a cover file is .mid or .json")
    if isinstance(x, np.ndarray):
        if x.dtype != NOTE_DTYPE:
            raise ValueError(f"a note array has dtype NOTE_DTYPE (onset, offset, pitch, velocity), got {x.dtype}")
        return np.ascontiguousarray(x.reshape(-1))
    out = np.empty(len(x), NOTE_DTYPE)
    for i, nd in enumerate(x):
        p, v = nd["pitch"], nd["velocity"]
        if int(p) != p or int(v) != v:
            raise ValueError(f"note {i}: pitch {p!r} and velocity {v!r} must be integers")
        out[i] = (float(nd["onset"]), float(nd["offset"]), int(p), int(v))
    return out


@dataclass
class Packed:
    """the host side of one ``render_many`` call: every cover checked and stably sorted by onset"""
    notes: np.ndarray            # NOTE_DTYPE, cover after cover
    note_offsets: np.ndarray     # int64 [B + 1]
    cents: np.ndarray            # float64 [B]
    num_samples: np.ndarray      # int64 [B]

    def __len__(self) -> int:
        return len(self.cents)


class NoteRenderer(Engine):
    """Note lists -> 1-d float32 device tensors.  ``workspace_budget`` bytes bound the samples plus the device workspace of one launch sequence: ``render_many``
    splits a call into sub-batches under it, which changes no cover's bits.  Constructing and ``pack`` need no GPU; rendering does: there is no CPU path."""
    _destroy = "etd_render_destroy"

    def __init__(self, sample_rate: int = 22050, voice: PianoVoice = PianoVoice(), device: Union[str, torch.device] = "cuda",
                 workspace_budget: int = DEFAULT_WORKSPACE_BUDGET):
        self.device = torch.device("cuda" if device == "auto" else device)
        self.sample_rate = int(sample_rate)
        self.voice = voice
        self.workspace_budget = int(workspace_budget)
        self._lib = _lib.lib()
        self.limits = limits()
        from .alignfeat import limits as af_limits
        assert self.limits["max_samples"] <= af_limits()["max_samples"]
        if self.sample_rate != sample_rate or not 8000 <= self.sample_rate <= 48000:
            raise ValueError(f"NoteRenderer: sample_rate must be an integer in 8000 .. 48000, got {sample_rate}")
        if not 1 <= int(voice.partials) <= self.limits["max_partials"]:
            raise ValueError(f"NoteRenderer: voice.partials must be in 1 .. {self.limits['max_partials']}, got {voice.partials}")
        d = asdict(voice)
        cfg = _lib.RenderCfg(sample_rate=self.sample_rate, partials=int(d.pop("partials")), flags=(1 if d.pop("decay") else 0) | (2 if d.pop("release") else 0),
                             **{k: float(v) for k, v in d.items()})
        h = C.c_void_p()
        try:
            _lib.check(self._lib.etd_render_create(C.byref(cfg), C.byref(h)), "etd_render_create")
        except _lib.EtudeHipError as e:
            raise ValueError(str(e)) from None
        self._adopt(h)

    # ---- host
    def pack(self, notes_list: Sequence, tuning_cents: Optional[Sequence[float]] = None, num_samples: Union[None, int, Sequence[Optional[int]]] = None) -> Packed:
        """host: every cover read, checked (``ValueError`` naming the cover and the note, in the caller's order) and stably sorted by onset.  num_samples: one
        length for all covers or one per cover (None = the cover's own: ``num_samples_for``)."""
        B = len(notes_list)
        if tuning_cents is None:
            tuning_cents = [0.0] * B
        if len(tuning_cents) != B:
            raise ValueError(f"pack: {B} covers but {len(tuning_cents)} tuning offsets")
        if num_samples is None or isinstance(num_samples, (int, np.integer)):
            num_samples = [num_samples] * B
        if len(num_samples) != B:
            raise ValueError(f"pack: {B} covers but {len(num_samples)} lengths")
        covers, Ns = [], []
        for b, x in enumerate(notes_list):
            try:
                a = as_note_array(x)
            except (ValueError, KeyError, TypeError) as e:
                raise ValueError(f"cover {b}: {e}") from None
            c = float(tuning_cents[b])
            if not abs(c) <= 50.0:
                raise ValueError(f"cover {b}: tuning must be within +-50 cents, got {tuning_cents[b]}")
            if len(a) > self.limits["max_notes"]:
                raise ValueError(f"cover {b}: {len(a)} notes, the engine takes {self.limits['max_notes']}")
            on, off = a["onset"], a["offset"]
            for bad, what in ((~(np.isfinite(on) & np.isfinite(off)), "a non-finite time"), (on < 0, "a negative onset"), (off <= on, "offset <= onset"),
                              ((a["pitch"] < 21) | (a["pitch"] > 108), "a pitch outside 21 .. 108"), ((a["velocity"] < 1) | (a["velocity"] > 127), "a velocity outside 1 .. 127")):
                if bad.any():
                    i = int(np.argmax(bad))
                    raise ValueError(f"cover {b}, note {i}: {what} (onset {on[i]}, offset {off[i]}, pitch {a['pitch'][i]}, velocity {a['velocity'][i]})")
            n = num_samples[b]
            own = num_samples_for(a, self.sample_rate, self.voice)
            N = own if n is None else int(n)
            if N < 0:
                raise ValueError(f"cover {b}: num_samples = {n} is negative")
            if N > self.limits["max_samples"]:
                raise ValueError(f"cover {b}: {N} samples ({N / self.sample_rate:.1f} s), the engine takes {self.limits['max_samples']}")
            covers.append(a[np.argsort(on, kind="stable")])
            Ns.append(N)
        offsets = np.zeros(B + 1, np.int64)
        np.cumsum([len(a) for a in covers], out=offsets[1:])
        notes = np.concatenate(covers) if covers else np.zeros(0, NOTE_DTYPE)
        return Packed(np.ascontiguousarray(notes, NOTE_DTYPE), offsets, np.asarray([float(c) for c in tuning_cents], np.float64), np.asarray(Ns, np.int64))

    def _sub(self, p: Packed, idx: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """the covers idx of a packed call as a call of their own: (notes, note offsets, cents, N, sample offsets)"""
        parts = [p.notes[p.note_offsets[i]: p.note_offsets[i + 1]] for i in idx]
        off = np.zeros(len(idx) + 1, np.int64)
        np.cumsum([len(a) for a in parts], out=off[1:])
        N = np.ascontiguousarray(p.num_samples[list(idx)])
        soff = np.zeros(len(idx) + 1, np.int64)
        np.cumsum((N + ALIGN - 1) // ALIGN * ALIGN, out=soff[1:])
        notes = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, NOTE_DTYPE)
        return notes, off, np.ascontiguousarray(p.cents[list(idx)]), N, soff

    def bytes_for(self, note_offsets: np.ndarray, N: np.ndarray) -> int:
        """host only: device workspace of one launch sequence"""
        return nonneg(self._lib.etd_render_bytes(self.h, len(N), note_offsets.ctypes.data_as(_lib.c_i64_p), N.ctypes.data_as(_lib.c_i64_p)), "etd_render_bytes")

    def batches(self, p: Packed) -> List[List[int]]:
        """consecutive covers grouped so that every group's samples and workspace fit the budget (a cover that alone exceeds it is refused) and no group holds
        more covers than one call takes"""
        groups, cur, cost = [], [], 0
        for i in range(len(p)):
            N = p.num_samples[i: i + 1]
            one = 4 * int((N[0] + ALIGN - 1) // ALIGN * ALIGN) + self.bytes_for(np.asarray([0, p.note_offsets[i + 1] - p.note_offsets[i]], np.int64), np.ascontiguousarray(N))
            if one > self.workspace_budget:
                raise ValueError(f"cover {i}: {int(N[0])} samples need {one} bytes of samples and workspace, the budget is {self.workspace_budget}")
            if cur and (len(cur) >= self.limits["max_covers"] or cost + one > self.workspace_budget):
                groups.append(cur)
                cur, cost = [], 0
            cur.append(i)
            cost += one
        if cur:
            groups.append(cur)
        return groups

    def plan(self, p: Packed) -> Tuple[np.ndarray, np.ndarray]:
        """test hook (host arithmetic): -> (int64 [notes][2]: per note the first sample it sounds on and the first it no longer does; int32 [blocks][2]: per block
        of ``limits["block"]`` samples, cover after cover, the candidate notes [lo, hi) of its cover)"""
        blocks = int(((p.num_samples + self.limits["block"] - 1) // self.limits["block"]).sum())
        fe, rg = np.zeros((len(p.notes), 2), np.int64), np.zeros((blocks, 2), np.int32)
        _lib.check(self._lib.etd_render_debug_plan(self.h, p.notes.ctypes.data, p.note_offsets.ctypes.data_as(_lib.c_i64_p), len(p),
                                                   p.num_samples.ctypes.data_as(_lib.c_i64_p), fe.ctypes.data, rg.ctypes.data), "etd_render_debug_plan")
        return fe, rg

    # ---- device
    def run_raw(self, notes: np.ndarray, note_offsets: np.ndarray, cents: np.ndarray, N: np.ndarray, sample_offsets: np.ndarray, out: torch.Tensor,
                ws: Optional[torch.Tensor] = None) -> None:
        """one launch sequence into the caller's flat float32 buffer (tests fill it with a pattern first); cover b lands at out[sample_offsets[b]:][:N[b]]"""
        dev = self._device()
        with torch.cuda.device(dev):
            if ws is None:
                ws = torch.empty(self.bytes_for(note_offsets, N), dtype=torch.uint8, device=dev)
            _lib.check(self._lib.etd_render_run(self.h, notes.ctypes.data, note_offsets.ctypes.data_as(_lib.c_i64_p), cents.ctypes.data, len(N),
                                                N.ctypes.data_as(_lib.c_i64_p), sample_offsets.ctypes.data_as(_lib.c_i64_p), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), ws.numel(), self._stream(dev)), "etd_render_run")
            ws.record_stream(torch.cuda.current_stream(dev))

    def iter_rendered(self, p: Packed) -> Iterator[Tuple[List[int], List[torch.Tensor]]]:
        """sub-batch after sub-batch: (the covers' indices, their samples as views of one flat buffer).  A caller that drops a sub-batch's tensors before it takes the
        next never holds more than one budget of samples."""
        dev = self._device()
        for idx in self.batches(p):
            notes, off, cents, N, soff = self._sub(p, idx)
            with torch.cuda.device(dev):
                flat = torch.empty(int(soff[-1]), dtype=torch.float32, device=dev)
                if int(N.sum()):
                    self.run_raw(notes, off, cents, N, soff, flat)
            yield idx, [flat[int(soff[j]): int(soff[j]) + int(N[j])] for j in range(len(idx))]

    def render_many(self, notes_list: Sequence, tuning_cents: Optional[Sequence[float]] = None,
                    num_samples: Union[None, int, Sequence[Optional[int]]] = None) -> List[torch.Tensor]:
        """covers -> their samples, 1-d float32 device tensors of ceil((max offset + R) sr) + 1 samples each (``num_samples``: zero-padded or truncated to that; a
        cover with no notes gives ``num_samples`` zeros, or an empty tensor).  A cover's samples depend on its notes, tuning and rate alone: bit-identical alone, in
        any batch, in any order, under any workspace budget and from run to run."""
        p = self.pack(notes_list, tuning_cents, num_samples)
        if len(p) == 0:
            return []
        out: List[Optional[torch.Tensor]] = [None] * len(p)
        for idx, tensors in self.iter_rendered(p):
            for i, t in zip(idx, tensors):
                out[i] = t
        return out      # type: ignore[return-value]

    def render(self, notes, tuning_cents: float = 0.0, num_samples: Optional[int] = None) -> torch.Tensor:
        return self.render_many([notes], [tuning_cents], num_samples)[0]

    def peaks_many(self, samples: Sequence[torch.Tensor]) -> np.ndarray:
        """max |x| of each 1-d float32 device tensor (what ``save_wav`` scales by), float32 [B] on the host: one launch per 4 096 tensors, 0 for an empty one"""
        dev = self._device()
        B = len(samples)
        if B == 0:
            return np.zeros(0, np.float32)
        for i, t in enumerate(samples):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                raise ValueError(f"peaks_many: tensor {i} must be a contiguous 1-d float32 tensor on {dev}")
        ptrs = np.asarray([t.data_ptr() if t.numel() else 0 for t in samples], np.int64)
        live = ptrs[ptrs != 0]
        base = int(live.min()) if live.size else 0
        offs = np.where(ptrs != 0, (ptrs - base) // 4, 0).astype(np.int64)
        Ns = np.asarray([t.numel() for t in samples], np.int64)
        cap = self.limits["max_covers"]
        with torch.cuda.device(dev):
            meta = torch.from_numpy(np.concatenate([offs, Ns])).to(dev)
            peaks = torch.empty(B, dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for b0 in range(0, B, cap):
                n = min(cap, B - b0)
                _lib.check(self._lib.etd_render_peaks(self.h, C.c_void_p(base), C.c_void_p(meta.data_ptr() + 8 * b0), C.c_void_p(meta.data_ptr() + 8 * (B + b0)), n,
                                                      C.c_void_p(peaks.data_ptr() + 4 * b0), C.c_void_p(st)), "etd_render_peaks")
            return peaks.cpu().numpy()


_default: Dict[str, NoteRenderer] = {}


def default_note_renderer(device="cuda") -> NoteRenderer:
    """one ``NoteRenderer`` (22 050 Hz, the default voice) per device, made once"""
    key = str(torch.device(device))
    if key not in _default:
        _default[key] = NoteRenderer(device=device)
    return _default[key]
