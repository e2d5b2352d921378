"""Separation quality on the MI355X: ``BSSEval`` takes reference and estimated stems to the BSS Eval v4 figures -- SDR, ISR, SIR, SAR per source on windows -- and the
plain SDR.

This project's own contract (tests/bss_np.py restates it), modelled on museval's ``bss_eval`` (v4, images, time-invariant distortion filters of 512
taps, 1-second windows): museval and mir_eval are not dependencies and parity with them is unpinned; museval's ``lstsq`` fallback for a singular system, its
framewise filters and its permutation search are not restated.  The device (csrc/bss.hip, fp64 on the fp64 matrix cores) returns eight energies per (source, window),
a silent flag per window and a status per track; the decibels and the medians are numpy fp64 here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i32, i64, nonneg, ptrs

MAX_SOURCES = 8
MAX_CHANNELS = 2
MAX_ORDER = 8192          # S L
METRICS = ("sdr", "isr", "sir", "sar", "sdr_plain")
_PAIRS = dict(sdr=(0, 1), isr=(0, 2), sir=(3, 4), sar=(5, 6), sdr_plain=(0, 7))


@dataclass
class BSSEvalConfig:
    filters_len: int = 512            # L: taps of the distortion filters
    window: int = 44100               # samples of a window
    hop: int = 44100
    workspace_bytes: int = 4 << 30    # budget of the device workspace

    def check(self) -> None:
        """ValueError for anything the engine refuses; needs no GPU"""
        L = self.filters_len
        if int(L) != L or L < 16 or L > 512 or L % 16:
            raise ValueError(f"BSSEvalConfig: filters_len must be a multiple of 16 in 16 .. 512, got {L}")
        if int(self.window) != self.window or self.window < L:
            raise ValueError(f"BSSEvalConfig: window must be >= filters_len = {L}, got {self.window}")
        if int(self.hop) != self.hop or not 1 <= self.hop <= self.window:
            raise ValueError(f"BSSEvalConfig: hop must be in 1 .. window = {self.window}, got {self.hop}")
        if int(self.workspace_bytes) != self.workspace_bytes or self.workspace_bytes < 1:
            raise ValueError(f"BSSEvalConfig: workspace_bytes must be positive, got {self.workspace_bytes}")


def decibels(num, den) -> np.ndarray:
    """10 log10(num / den) in fp64; den == 0 gives +inf; NaN stays NaN"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(num / den)
    out = np.where(den == 0, np.inf, out)
    return np.where(np.isnan(num) | np.isnan(den), np.nan, out)


def metrics_from_energies(E: np.ndarray) -> Dict[str, np.ndarray]:
    """E [J][nwin][8] -> the five [J][nwin] arrays in dB (step 6 of DESIGN.md 4p)"""
    E = np.asarray(E, np.float64)
    return {k: decibels(E[..., a], E[..., b]) for k, (a, b) in _PAIRS.items()}


def nanmedian_rows(v: np.ndarray) -> np.ndarray:
    """the median over the last axis of the entries that are not NaN; NaN for a row of NaNs"""
    out = np.full(v.shape[0], np.nan)
    for j in range(v.shape[0]):
        ok = ~np.isnan(v[j])
        if ok.any():
            out[j] = np.median(v[j][ok])
    return out


def aggregate(results: Sequence[Dict]) -> Dict:
    """track results of ``evaluate_many`` -> the corpus score: per metric the median over the tracks of the per-source track scores.  A track whose windows are all NaN
    (for a source: for that source) is left out; ``n_skipped`` counts the tracks left out of every source."""
    if not results:
        return dict({k: np.zeros(0) for k in METRICS}, n_tracks=0, n_skipped=0)
    J = {len(r["scores"]["sdr"]) for r in results}
    if len(J) != 1:
        raise ValueError(f"aggregate: the tracks have different numbers of sources: {sorted(J)}")
    out: Dict = {}
    for k in METRICS:
        out[k] = nanmedian_rows(np.stack([r["scores"][k] for r in results], axis=1))
    skipped = sum(1 for r in results if all(np.isnan(r["scores"][k]).all() for k in METRICS))
    out["n_tracks"], out["n_skipped"] = len(results), skipped
    return out


def check_shapes(cfg: BSSEvalConfig, refs_list: Sequence, ests_list: Sequence) -> List[tuple]:
    """ValueError naming the track for anything ``evaluate_many`` refuses about shapes; needs no GPU.  -> [(J, C, N)]"""
    if len(refs_list) != len(ests_list):
        raise ValueError(f"BSSEval: {len(refs_list)} reference tracks and {len(ests_list)} estimate tracks")
    shapes = []
    for i, (a, b) in enumerate(zip(refs_list, ests_list)):
        sa, sb = (tuple(x.shape) if hasattr(x, "shape") else None for x in (a, b))
        if sa is None or len(sa) != 3:
            raise ValueError(f"track {i}: references must be [sources][channels][N], got shape {sa}")
        if sa != sb:
            raise ValueError(f"track {i}: references have shape {sa}, estimates {sb}")
        J, Cn, N = sa
        if not 1 <= J <= MAX_SOURCES:
            raise ValueError(f"track {i}: {J} sources (need 1 .. {MAX_SOURCES})")
        if Cn not in (1, 2):
            raise ValueError(f"track {i}: {Cn} channels (need 1 or 2)")
        if N < cfg.filters_len:
            raise ValueError(f"track {i}: N = {N} is below filters_len = {cfg.filters_len}")
        if J * Cn * cfg.filters_len > MAX_ORDER:
            raise ValueError(f"track {i}: S L = {J * Cn * cfg.filters_len} is above {MAX_ORDER}")
        shapes.append((J, Cn, N))
    return shapes


class BSSEval(Engine):
    """References and estimates, per track [sources][channels][N] float32 (device tensors are used in place, host arrays are uploaded) -> the BSS Eval v4 figures.
    A track gives the same bits alone, at any place in a batch, under any ``workspace_bytes`` that admits it and from run to run.  Constructing needs no GPU;
    evaluating does: there is no CPU path."""
    _destroy = "etd_bss_destroy"

    def __init__(self, config: Optional[BSSEvalConfig] = None, device: Union[str, torch.device] = "cuda"):
        self.config = cfg = config or BSSEvalConfig()
        cfg.check()
        self.device = torch.device("cuda" if device == "auto" else device)
        self._lib = _lib.lib()
        ccfg = _lib.BssCfg(filters_len=int(cfg.filters_len), window=int(cfg.window), hop=int(cfg.hop), workspace_bytes=int(cfg.workspace_bytes))
        h = C.c_void_p()
        _lib.check(self._lib.etd_bss_create(C.byref(ccfg), C.byref(h)), "etd_bss_create")
        self._adopt(h)
        self.guard = 0                 # test hook: elements of guard values on both sides of every output buffer
        self._guards: List[tuple] = []

    # ------------------------------------------------------------------ host arithmetic
    def num_windows(self, N: int) -> int:
        return nonneg(self._lib.etd_bss_num_windows(self.h, int(N)), "etd_bss_num_windows")

    def workspace_bytes(self, J: int, Cn: int, N: int) -> int:
        """bytes of device workspace a track needs at the least"""
        return nonneg(self._lib.etd_bss_workspace_bytes(self.h, int(J), int(Cn), int(N)), "etd_bss_workspace_bytes")

    def window_bounds(self, N: int) -> List[tuple]:
        nw, cfg = self.num_windows(N), self.config
        return [(w * cfg.hop, N if w == nw - 1 else w * cfg.hop + cfg.window) for w in range(nw)]

    # ------------------------------------------------------------------ buffers
    def _out(self, shape, dtype, dev) -> torch.Tensor:
        n = int(np.prod(shape))
        if not self.guard:
            return torch.empty(shape, dtype=dtype, device=dev)
        g = int(self.guard)
        sentinel = 12345.678 if dtype.is_floating_point else 0x5A5A5A5A
        flat = torch.full((n + 2 * g,), sentinel, dtype=dtype, device=dev)
        self._guards.append((flat, g, n, sentinel))
        return flat[g:g + n].view(shape)

    def guards_intact(self) -> bool:
        """test hook: the guard values around every output buffer allocated since the last call are untouched"""
        ok = True
        for flat, g, n, sentinel in self._guards:
            ok = ok and bool((flat[:g] == sentinel).all()) and bool((flat[g + n:] == sentinel).all())
        self._guards = []
        return ok

    def _tracks(self, refs_list: Sequence, ests_list: Sequence):
        shapes = check_shapes(self.config, refs_list, ests_list)
        for i, (J, Cn, N) in enumerate(shapes):
            need = self.workspace_bytes(J, Cn, N)
            if need > self.config.workspace_bytes:
                raise ValueError(f"track {i}: needs {need} bytes of workspace, workspace_bytes is {self.config.workspace_bytes}")
        dev = self._device()
        refs = [torch.as_tensor(x).to(dev, torch.float32).contiguous() for x in refs_list]
        ests = [torch.as_tensor(x).to(dev, torch.float32).contiguous() for x in ests_list]
        if refs:
            bad = torch.stack([torch.isfinite(a).all() & torch.isfinite(b).all() for a, b in zip(refs, ests)]).logical_not().nonzero().flatten().tolist()
            if bad:
                raise ValueError(f"track {bad[0]}: holds a non-finite sample")
        return shapes, refs, ests, dev

    # ------------------------------------------------------------------ device
    def energies_many(self, refs_list: Sequence, ests_list: Sequence) -> List[Dict]:
        """-> per track ``{"E": float64 [J][nwin][8], "silent": bool [nwin], "status": int}`` (status 1: singular, E is NaN)"""
        shapes, refs, ests, dev = self._tracks(refs_list, ests_list)
        if not shapes:
            return []
        n = len(shapes)
        nw = [self.num_windows(N) for _, _, N in shapes]
        Es = [self._out((J, w, 8), torch.float64, dev) for (J, _, _), w in zip(shapes, nw)]
        sil = [self._out((w,), torch.int32, dev) for w in nw]
        status = self._out((n,), torch.int32, dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_bss_run(self.h, n, ptrs(refs), ptrs(ests), i32([s[0] for s in shapes]), i32([s[1] for s in shapes]), i64([s[2] for s in shapes]),
                                             ptrs(Es), ptrs(sil), C.c_void_p(status.data_ptr()), self._stream(dev)), "etd_bss_run")
            hold(refs + ests, dev)
        st = status.cpu().numpy()
        return [dict(E=Es[b].cpu().numpy(), silent=sil[b].cpu().numpy() != 0, status=int(st[b])) for b in range(n)]

    def evaluate_many(self, refs_list: Sequence, ests_list: Sequence) -> List[Dict]:
        """-> per track the five ``[J][nwin]`` arrays in dB (``sdr``, ``isr``, ``sir``, ``sar``, ``sdr_plain``), ``silent`` [nwin], ``status``, ``E`` and ``scores``:
        per metric the nanmedian over the windows, [J]"""
        out = []
        for res in self.energies_many(refs_list, ests_list):
            m = metrics_from_energies(res["E"])
            res.update(m)
            res["scores"] = {k: nanmedian_rows(v) for k, v in m.items()}
            out.append(res)
        return out

    aggregate = staticmethod(aggregate)

    # ------------------------------------------------------------------ test hooks (include/etude_hip_debug.h)
    def _one(self, ref, est):
        shapes, refs, ests, dev = self._tracks([ref], [est])
        return shapes[0], refs[0], ests[0], dev

    def debug_corr(self, ref, est):
        """-> r [S][S][L], d [S][S][L] float64"""
        (J, Cn, N), ref, est, dev = self._one(ref, est)
        S, L = J * Cn, self.config.filters_len
        r, d = self._out((S, S, L), torch.float64, dev), self._out((S, S, L), torch.float64, dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_bss_debug_corr(self.h, C.c_void_p(ref.data_ptr()), C.c_void_p(est.data_ptr()), J, Cn, N, C.c_void_p(r.data_ptr()),
                                                    C.c_void_p(d.data_ptr()), self._stream(dev)), "etd_bss_debug_corr")
            hold([ref, est], dev)
        return r.cpu().numpy(), d.cpu().numpy()

    def debug_solve(self, G, rhs):
        """a caller's SPD matrix [n][n] and right-hand sides [n][m <= 16] -> (x [n][m], status)"""
        dev = self._device()
        G = torch.as_tensor(np.ascontiguousarray(G, np.float64)).to(dev)
        rhs = torch.as_tensor(np.ascontiguousarray(rhs, np.float64)).to(dev)
        n, m = int(rhs.shape[0]), int(rhs.shape[1])
        if tuple(G.shape) != (n, n):
            raise ValueError(f"debug_solve: G has shape {tuple(G.shape)}, the right-hand sides {tuple(rhs.shape)}")
        x, status = self._out((n, m), torch.float64, dev), self._out((1,), torch.int32, dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_bss_debug_solve(self.h, C.c_void_p(G.data_ptr()), C.c_void_p(rhs.data_ptr()), n, m, C.c_void_p(x.data_ptr()),
                                                     C.c_void_p(status.data_ptr()), self._stream(dev)), "etd_bss_debug_solve")
            hold([G, rhs], dev)
        return x.cpu().numpy(), int(status.cpu()[0])

    def debug_filters(self, ref, est):
        """-> (A [S L][S], B [J][C L][C], status)"""
        (J, Cn, N), ref, est, dev = self._one(ref, est)
        S, L = J * Cn, self.config.filters_len
        A, B, status = self._out((S * L, S), torch.float64, dev), self._out((J, Cn * L, Cn), torch.float64, dev), self._out((1,), torch.int32, dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_bss_debug_filters(self.h, C.c_void_p(ref.data_ptr()), C.c_void_p(est.data_ptr()), J, Cn, N, C.c_void_p(A.data_ptr()),
                                                       C.c_void_p(B.data_ptr()), C.c_void_p(status.data_ptr()), self._stream(dev)), "etd_bss_debug_filters")
            hold([ref, est], dev)
        return A.cpu().numpy(), B.cpu().numpy(), int(status.cpu()[0])

    def debug_project(self, ref, window_index: int, A, B):
        """window ``window_index`` of the references with a caller's filters -> (ps [J][C][Wout], pa [J][C][Wout])"""
        (J, Cn, N), ref, _, dev = self._one(ref, ref)
        S, L = J * Cn, self.config.filters_len
        A = torch.as_tensor(np.ascontiguousarray(A, np.float64)).to(dev)
        B = torch.as_tensor(np.ascontiguousarray(B, np.float64)).to(dev)
        if tuple(A.shape) != (S * L, S) or tuple(B.shape) != (J, Cn * L, Cn):
            raise ValueError(f"debug_project: A has shape {tuple(A.shape)}, B {tuple(B.shape)}")
        bounds = self.window_bounds(N)
        if not 0 <= window_index < len(bounds):
            raise ValueError(f"debug_project: window {window_index} of {len(bounds)}")
        wout = bounds[window_index][1] - bounds[window_index][0] + L - 1
        ps, pa = self._out((J, Cn, wout), torch.float64, dev), self._out((J, Cn, wout), torch.float64, dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_bss_debug_project(self.h, C.c_void_p(ref.data_ptr()), J, Cn, N, int(window_index), C.c_void_p(A.data_ptr()),
                                                       C.c_void_p(B.data_ptr()), C.c_void_p(ps.data_ptr()), C.c_void_p(pa.data_ptr()), self._stream(dev)),
                       "etd_bss_debug_project")
            hold([ref, A, B], dev)
        return ps.cpu().numpy(), pa.cpu().numpy()

    def timing(self, on: bool) -> np.ndarray:
        """tools/bench_bss.py: turn the stage timers on or off -> the last timed run's milliseconds (correlations, factorisations, substitutions, projections, energies)"""
        ms = (C.c_double * 5)()
        _lib.check(self._lib.etd_bss_debug_timing(self.h, int(bool(on)), ms), "etd_bss_debug_timing")
        return np.array(list(ms))
