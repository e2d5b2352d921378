"""Alignment features on the MI355X: ``AlignFeatures`` -- mono audio at 22 050 Hz -> (quantised chroma [12][T], DLNCO [12][T]) at 50 Hz, the input of the DTW.

Modelled on synctoolbox's published pipeline (audio_to_pitch_features, pitch_to_chroma, quantize_chroma, audio_to_pitch_onset_features,
pitch_onset_features_to_DLNCO): three rate tiers, 88 zero-phase elliptic band-passes (the hot path: csrc/alignfeat.hip splits the recurrence's time axis
exactly into chunks), pitch energy, chroma, onset novelty, peaks, DLNCO.  DESIGN.md 4f is the contract; tests/alignfeat_np.py restates it in fp64 numpy.
synctoolbox is not a dependency and parity with it is unpinned; ``tuning_offsets="estimate"`` takes each song's offset from ``etude_amd.tuning``;
WAV files of any rate come in through ``etude_amd.audio.AudioLoader``; decoding other formats stays the caller's.

The filter design (``ellip_bandpass_sos``) is numpy fp64 of its own -- the package does not depend on scipy; tests/test_alignfeat_cpu.py holds it to
``scipy.signal.ellipord`` / ``ellip``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine, hold, i32, i64, mono_songs_to_device, nonneg, ptrs

FS = 22050
HOP = 441                      # 50 Hz features
PITCHES = tuple(range(21, 109))
N_BANDS = 88
MAX_SECTIONS = 6
FIR_HALF = 240
DECIM = 5
TIER_FS = (22050, 4410, 882)
DEFAULT_WORKSPACE_BUDGET = 8 << 30


def tier_of_pitch(p: int) -> int:
    """21..59 read x2 (882 Hz), 60..95 read x1 (4 410 Hz), 96..108 read x0 (22 050 Hz)"""
    return 2 if p <= 59 else (1 if p <= 95 else 0)


def decimation_fir() -> np.ndarray:
    """h[n] = (1/5) sinc(n / 5) kaiser_481(beta = 8)[n + 240], n = -240 .. 240, divided by its sum; formed in fp64, returned as float32 [481]"""
    n = np.arange(-FIR_HALF, FIR_HALF + 1, dtype=np.float64)
    h = (1.0 / DECIM) * np.sinc(n / DECIM) * np.kaiser(2 * FIR_HALF + 1, 8.0)
    return (h / h.sum()).astype(np.float32)


# ---------------------------------------------------------------------------------------------- elliptic design
def _ellipk(m: float) -> float:
    """complete elliptic integral K(m) (parameter m = k^2 < 1) by the arithmetic-geometric mean"""
    a, b = 1.0, math.sqrt(1.0 - m)
    for _ in range(64):
        if abs(a - b) <= 1e-17 * a:
            break
        a, b = 0.5 * (a + b), math.sqrt(a * b)
    return math.pi / (2.0 * a)


def _ellipkm1(p: float) -> float:
    """K(1 - p), accurate for tiny p (the AGM starts from sqrt(p), no cancellation)"""
    a, b = 1.0, math.sqrt(p)
    for _ in range(64):
        if abs(a - b) <= 1e-17 * a:
            break
        a, b = 0.5 * (a + b), math.sqrt(a * b)
    return math.pi / (2.0 * a)


def _ellipj(u: float, m: float) -> Tuple[float, float, float]:
    """Jacobi sn, cn, dn of real u for parameter 0 <= m < 1: arithmetic-geometric scale, then the descending Landen recurrence on the amplitude"""
    a, b, c = [1.0], math.sqrt(1.0 - m), [math.sqrt(m)]
    while abs(c[-1]) > 1e-17 * a[-1] and len(a) < 40:
        a_n, c_n = 0.5 * (a[-1] + b), 0.5 * (a[-1] - b)
        b = math.sqrt(a[-1] * b)
        a.append(a_n); c.append(c_n)
    phi = (2.0 ** (len(a) - 1)) * a[-1] * u
    for i in range(len(a) - 1, 0, -1):
        phi = 0.5 * (phi + math.asin(c[i] * math.sin(phi) / a[i]))
    sn, cn = math.sin(phi), math.cos(phi)
    return sn, cn, math.sqrt(1.0 - m * sn * sn)


def _carlson_rf(x: float, y: float, z: float) -> float:
    """Carlson's symmetric integral R_F by duplication"""
    for _ in range(100):
        lam = math.sqrt(x * y) + math.sqrt(y * z) + math.sqrt(z * x)
        x, y, z = 0.25 * (x + lam), 0.25 * (y + lam), 0.25 * (z + lam)
        mu = (x + y + z) / 3.0
        dx, dy, dz = 1.0 - x / mu, 1.0 - y / mu, 1.0 - z / mu
        if max(abs(dx), abs(dy), abs(dz)) < 1e-9:          # (the series below is good to the 6th power of this)
            break
    e2, e3 = dx * dy - dz * dz, dx * dy * dz
    return (1.0 + (e2 / 24.0 - 0.1 - 3.0 * e3 / 44.0) * e2 + e3 / 14.0) / math.sqrt(mu)


def _arc_sc(w: float, m: float) -> float:
    """the real u with sc(u | m) = w: the incomplete integral F(atan w | m) = sin(phi) R_F(cos^2 phi, 1 - m sin^2 phi, 1)"""
    phi = math.atan(w)
    s, c = math.sin(phi), math.cos(phi)
    return s * _carlson_rf(c * c, 1.0 - m * s * s, 1.0)


def _ellip_degree(n: int, m1: float) -> float:
    """the parameter m with K'(m) / K(m) = (K'(m1) / K(m1)) / n: the nome q = q1^(1/n), then m from its theta series"""
    q = math.exp(-math.pi * _ellipkm1(m1) / _ellipk(m1)) ** (1.0 / n)
    num = sum(q ** (i * (i + 1)) for i in range(12))
    den = 1.0 + 2.0 * sum(q ** (i * i) for i in range(1, 13))
    return 16.0 * q * (num / den) ** 4


def ellip_order(wp: Sequence[float], ws: Sequence[float], rp: float, rs: float) -> int:
    """the minimal elliptic order of a digital band-pass with pass band wp and stop band ws (both as fractions of Nyquist): ``scipy.signal.ellipord``"""
    pb = [math.tan(0.5 * math.pi * w) for w in wp]
    sb = [math.tan(0.5 * math.pi * w) for w in ws]
    nat = min(abs((s * s - pb[0] * pb[1]) / (s * (pb[0] - pb[1]))) for s in sb)
    arg1 = (10.0 ** (0.1 * rp) - 1.0) / (10.0 ** (0.1 * rs) - 1.0)
    arg0 = (1.0 / nat) ** 2
    return int(math.ceil(_ellipk(arg0) * _ellipkm1(arg1) / (_ellipkm1(arg0) * _ellipk(arg1))))


def _ellip_prototype(n: int, rp: float, rs: float):
    """the analog low-pass prototype of order n (pass-band edge 1): zeros, poles, gain -- ``scipy.signal.ellipap``"""
    eps_sq = 10.0 ** (0.1 * rp) - 1.0
    eps = math.sqrt(eps_sq)
    ck1_sq = eps_sq / (10.0 ** (0.1 * rs) - 1.0)
    m = _ellip_degree(n, ck1_sq)
    capk = _ellipk(m)
    v0 = capk * _arc_sc(1.0 / eps, 1.0 - ck1_sq) / (n * _ellipk(ck1_sq))
    sv, cv, dv = _ellipj(v0, 1.0 - m)
    zeros, poles = [], []
    for j in range(1 - n % 2, n, 2):
        s, c, d = _ellipj(j * capk / n, m)
        p = -(c * d * sv * cv + 1j * s * dv) / (1.0 - (d * sv) ** 2)
        if j == 0:
            poles.append(complex(p.real, 0.0))
        else:
            zeros += [1j / (math.sqrt(m) * s), -1j / (math.sqrt(m) * s)]
            poles += [p, p.conjugate()]
    z, p = np.array(zeros, np.complex128), np.array(poles, np.complex128)
    k = (np.prod(-p) / np.prod(-z)).real
    if n % 2 == 0:
        k /= math.sqrt(1.0 + eps_sq)
    return z, p, float(k)


def ellip_bandpass_zpk(fc: float, fs: float, Q: float = 25.0, stop: float = 2.0, rp: float = 1.0, rs: float = 50.0):
    """-> (order of the prototype, zeros, poles, gain) of the digital filter"""
    half = 0.5 / Q
    wp = [fc * (1.0 - half) / (0.5 * fs), fc * (1.0 + half) / (0.5 * fs)]
    ws = [fc * (1.0 - stop * half) / (0.5 * fs), fc * (1.0 + stop * half) / (0.5 * fs)]
    if not (0.0 < ws[0] < wp[0] < wp[1] < ws[1] < 1.0):
        raise ValueError(f"ellip_bandpass_sos: band edges {ws[0]}, {wp[0]}, {wp[1]}, {ws[1]} (fractions of Nyquist) are not increasing inside (0, 1)")
    n = ellip_order(wp, ws, rp, rs)
    z, p, k = _ellip_prototype(n, rp, rs)
    warped = [4.0 * math.tan(0.5 * math.pi * w) for w in wp]          # (bilinear with fs = 2)
    bw, wo = warped[1] - warped[0], math.sqrt(warped[0] * warped[1])
    # low-pass -> band-pass
    degree = len(p) - len(z)
    zl, pl = z * (0.5 * bw), p * (0.5 * bw)
    zb = np.concatenate([zl + np.sqrt(zl * zl - wo * wo), zl - np.sqrt(zl * zl - wo * wo), np.zeros(degree, np.complex128)])
    pb = np.concatenate([pl + np.sqrt(pl * pl - wo * wo), pl - np.sqrt(pl * pl - wo * wo)])
    kb = k * bw ** degree
    # bilinear map
    zd = np.concatenate([(4.0 + zb) / (4.0 - zb), -np.ones(len(pb) - len(zb), np.complex128)])
    pd = (4.0 + pb) / (4.0 - pb)
    kd = kb * (np.prod(4.0 - zb) / np.prod(4.0 - pb)).real
    return n, zd, pd, float(kd)


def ellip_bandpass_sos(fc: float, fs: float, Q: float = 25.0, stop: float = 2.0, rp: float = 1.0, rs: float = 50.0) -> np.ndarray:
    """The minimal-order elliptic band-pass around fc (pass band fc (1 -+ 1 / 2Q), stop band fc (1 -+ stop / 2Q), rp dB ripple, rs dB rejection) as second-order
    sections [n][6] = (b0, b1, b2, 1, a1, a2) in fp64 -- what ``ellipord`` then ``ellip(..., output="sos")`` of scipy.signal design (same order, poles and zeros; the
    pairing is this function's own: the pole pair nearest the unit circle takes the nearest zero pair and comes last, the gain sits in the first section)."""
    n, z, p, k = ellip_bandpass_zpk(fc, fs, Q, stop, rp, rs)
    pu = sorted([x for x in p if x.imag > 0], key=lambda x: 1.0 - abs(x))
    if 2 * len(pu) != len(p):
        raise ValueError("ellip_bandpass_sos: a real pole (the band is too wide for this pairing)")
    zu = [("c", x) for x in z if x.imag > 1e-12]
    real = sorted(x.real for x in z if abs(x.imag) <= 1e-12)
    if len(real) % 2:
        raise ValueError("ellip_bandpass_sos: an odd number of real zeros")
    zu += [("r", (real[i], real[len(real) - 1 - i])) for i in range(len(real) // 2)]
    if len(zu) != len(pu):
        raise ValueError("ellip_bandpass_sos: zero and pole pairs differ in number")
    sections = []
    for pole in pu:
        def dist(e):
            return abs(e[1] - pole) if e[0] == "c" else min(abs(e[1][0] - pole), abs(e[1][1] - pole))
        e = min(zu, key=dist)
        zu.remove(e)
        b = [1.0, -2.0 * e[1].real, abs(e[1]) ** 2] if e[0] == "c" else [1.0, -(e[1][0] + e[1][1]), e[1][0] * e[1][1]]
        sections.append(b + [1.0, -2.0 * pole.real, abs(pole) ** 2])
    sos = np.array(sections[::-1], np.float64)
    sos[0, :3] *= k
    return sos


# ---------------------------------------------------------------------------------------------- the bank and the chunk tables
def step_matrix(sos: np.ndarray) -> np.ndarray:
    """A [12][12]: the state of the cascade (z0, z1 of section 0, of section 1, ...; transposed direct form II, the recurrence of ``sosfilt``) after one step with input
    0, as a linear map of the state before it.  Unused sections leave zero rows and columns."""
    ns = sos.shape[0]
    A = np.zeros((2 * MAX_SECTIONS, 2 * MAX_SECTIONS), np.float64)
    for j in range(2 * ns):
        z = np.zeros(2 * ns)
        z[j] = 1.0
        x = 0.0
        for k in range(ns):
            b0, b1, b2, _, a1, a2 = sos[k]
            y = b0 * x + z[2 * k]
            z[2 * k] = b1 * x - a1 * y + z[2 * k + 1]
            z[2 * k + 1] = b2 * x - a2 * y
            x = y
        A[: 2 * ns, j] = z
    return A


def chunk_power(sos: np.ndarray, L: int) -> np.ndarray:
    """A^L by repeated squaring in fp64: the map from a chunk's true start state to its contribution to the next chunk's"""
    return np.linalg.matrix_power(step_matrix(sos), int(L))


def pitch_filterbank(tuning_offset: float = 0.0, chunk: int = 256) -> Dict[str, np.ndarray]:
    """All 88 bands for a tuning offset in cents: {"sos": [88][6][6] fp64 (unused sections zero), "n_sections": [88] int32, "apow": [88][12][12] fp64 (A^chunk),
    "fc": [88]}"""
    t = float(tuning_offset)
    if not abs(t) <= 50.0:
        raise ValueError(f"pitch_filterbank: tuning_offset must be within +-50 cents, got {tuning_offset}")
    sos = np.zeros((N_BANDS, MAX_SECTIONS, 6), np.float64)
    nsec = np.zeros(N_BANDS, np.int32)
    apow = np.zeros((N_BANDS, 2 * MAX_SECTIONS, 2 * MAX_SECTIONS), np.float64)
    fcs = np.zeros(N_BANDS, np.float64)
    for b, p in enumerate(PITCHES):
        fc = 440.0 * 2.0 ** ((p - 69 + t / 100.0) / 12.0)
        s = ellip_bandpass_sos(fc, TIER_FS[tier_of_pitch(p)])
        if s.shape[0] > MAX_SECTIONS:
            raise ValueError(f"pitch_filterbank: pitch {p} needs {s.shape[0]} sections, the engine takes {MAX_SECTIONS}")
        sos[b, : s.shape[0]] = s
        nsec[b] = s.shape[0]
        apow[b] = chunk_power(s, chunk)
        fcs[b] = fc
    return {"sos": sos, "n_sections": nsec, "apow": apow, "fc": fcs}


_bank_cache: Dict[Tuple[float, int], Dict[str, np.ndarray]] = {}


def _bank(t: float, chunk: int) -> Dict[str, np.ndarray]:
    key = (float(t), int(chunk))
    if key not in _bank_cache:
        if len(_bank_cache) >= 64:
            _bank_cache.clear()
        _bank_cache[key] = pitch_filterbank(t, chunk)
    return _bank_cache[key]


def limits() -> dict:
    """Host only: the constants of the built library"""
    L, ms, mb, mg = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    mn = C.c_longlong()
    _lib.check(_lib.lib().etd_alignfeat_limits(C.byref(L), C.byref(ms), C.byref(mn), C.byref(mg), C.byref(mb)), "etd_alignfeat_limits")
    return dict(chunk=L.value, max_sections=ms.value, max_samples=mn.value, max_songs=mg.value, max_banks=mb.value)


class _Handle(Engine):
    """one etd_alignfeat handle: the filterbanks of a fixed tuple of tuning offsets"""
    _destroy = "etd_alignfeat_destroy"

    def __init__(self, lib, tunings: Tuple[float, ...], chunk: int):
        banks = [_bank(t, chunk) for t in tunings]
        sos = np.ascontiguousarray(np.stack([b["sos"] for b in banks]))
        nsec = np.ascontiguousarray(np.stack([b["n_sections"] for b in banks]))
        apow = np.ascontiguousarray(np.stack([b["apow"] for b in banks]))
        fir = decimation_fir()
        cfg = _lib.AlignFeatCfg(sample_rate=FS, hop=HOP, fir_taps=2 * FIR_HALF + 1, decimation=DECIM, chunk=chunk, n_banks=len(banks))
        h = C.c_void_p()
        _lib.check(lib.etd_alignfeat_create(C.byref(cfg), fir.ctypes.data, sos.ctypes.data, nsec.ctypes.data, apow.ctypes.data, C.byref(h)), "etd_alignfeat_create")
        self._adopt(h)
        self.index = {t: i for i, t in enumerate(tunings)}


class AlignFeatures(Engine):
    """Mono audio at 22 050 Hz -> (quantised chroma, DLNCO), both [12][ceil(N / 441)] float32 device tensors: what ``DTWEngine`` aligns.

    A song is a 1-d float32 array or tensor (host or device), finite, N >= 1, with a tuning offset in cents (|t| <= 50, default 0; ``"estimate"`` asks the
    device estimator of ``etude_amd.tuning``, which needs N >= 32 768).  ``workspace_budget`` bytes bound the device workspace of one launch sequence: ``features_many`` splits a call into sub-batches under it, which changes
    no song's bits.  Constructing needs no GPU; ``features_many`` does: there is no CPU path."""

    def __init__(self, device: Union[str, torch.device] = "cuda", workspace_budget: int = DEFAULT_WORKSPACE_BUDGET):
        self.device = torch.device("cuda" if device == "auto" else device)
        self.workspace_budget = int(workspace_budget)
        self._lib = _lib.lib()
        self.limits = limits()
        self.chunk = self.limits["chunk"]
        self._handles: Dict[Tuple[float, ...], _Handle] = {}
        self._handle((0.0,))

    def close(self) -> None:
        """this engine's handles are its ``_Handle`` objects, one per set of filterbanks: close them all (a later call makes the ones it needs again)"""
        for hd in getattr(self, "_handles", {}).values():
            hd.close()
        self._handles = {}

    def _handle(self, tunings: Tuple[float, ...]) -> _Handle:
        """the handle that holds these tunings' filterbanks: an existing one whose banks include them all, else a new one (at most 8 are kept; the one made
        longest ago goes first, never the default (0.0,))"""
        for hd in self._handles.values():
            if all(t in hd.index for t in tunings):
                return hd
        if len(self._handles) >= 8:
            del self._handles[next(k for k in self._handles if k != (0.0,))]
        self._handles[tunings] = _Handle(self._lib, tunings, self.chunk)
        return self._handles[tunings]

    def num_frames(self, N: int) -> int:
        T = int(self._lib.etd_alignfeat_num_frames(self._handle((0.0,)).h, int(N)))
        if T < 0:
            raise ValueError(f"num_frames: N must be >= 1, got {N}")
        return T

    def workspace_bytes(self, Ns: Sequence[int]) -> int:
        return nonneg(self._lib.etd_alignfeat_workspace_bytes(self._handle((0.0,)).h, len(Ns), i64(Ns)), "etd_alignfeat_workspace_bytes")

    def layout(self, Ns: Sequence[int], song: int) -> dict:
        """test hook (host arithmetic): where song `song` of a call with these lengths keeps its intermediate stages in the workspace (byte offsets) and their counts"""
        out = (C.c_int64 * len(_lib.ALIGNFEAT_LAYOUT))()
        _lib.check(self._lib.etd_alignfeat_debug_layout(self._handle((0.0,)).h, len(Ns), i64(Ns), int(song), out, len(_lib.ALIGNFEAT_LAYOUT)), "etd_alignfeat_debug_layout")
        return dict(zip(_lib.ALIGNFEAT_LAYOUT, [int(v) for v in out]))

    def _batches(self, Ns: Sequence[int], tunings: Optional[Sequence[float]] = None) -> List[List[int]]:
        """consecutive songs grouped so that every group's workspace fits the budget (a song that alone exceeds it is refused) and no group holds more songs or
        more distinct tuning offsets than one handle takes"""
        groups, cur, banks = [], [], set()
        for i, n in enumerate(Ns):
            t = 0.0 if tunings is None else float(tunings[i])
            if cur and (len(cur) >= self.limits["max_songs"] or len(banks | {t}) > self.limits["max_banks"]
                        or self.workspace_bytes([Ns[j] for j in cur] + [n]) > self.workspace_budget):
                groups.append(cur)
                cur, banks = [], set()
            cur.append(i)
            banks.add(t)
            if len(cur) == 1 and self.workspace_bytes([n]) > self.workspace_budget:
                raise ValueError(f"song {i}: N = {n} needs {self.workspace_bytes([n])} bytes of workspace, the budget is {self.workspace_budget}")
        groups.append(cur)
        return groups

    def run_raw(self, songs: Sequence[torch.Tensor], tunings: Sequence[float], chroma: torch.Tensor, dlnco: torch.Tensor, ws: torch.Tensor) -> None:
        """one launch sequence on checked device tensors with the caller's buffers (tests put canaries around them)"""
        n = len(songs)
        distinct = tuple(sorted(set(float(t) for t in tunings)))
        if len(distinct) > self.limits["max_banks"]:
            raise ValueError(f"run_raw: {len(distinct)} distinct tuning offsets in one launch sequence, a handle takes {self.limits['max_banks']} (features_many splits such a call)")
        hd = self._handle(distinct)
        dev = self._device()
        with torch.cuda.device(dev):
            _lib.check(self._lib.etd_alignfeat_run(hd.h, ptrs(songs), n, i64([t.numel() for t in songs]), i32([hd.index[float(t)] for t in tunings]),
                                                   C.c_void_p(chroma.data_ptr()), C.c_void_p(dlnco.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel() * ws.element_size(),
                                                   self._stream(dev)), "etd_alignfeat_run")

    def features_many(self, wavs: Sequence, tuning_offsets: Union[None, str, Sequence[float]] = None) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """songs [N_s] -> [(quantised chroma [12][T_s], DLNCO [12][T_s])] as device tensors.  A song's features depend on its samples and its tuning offset alone:
        bit-identical alone, in any batch, in any order and under any workspace budget.  ``tuning_offsets="estimate"``: every song's offset is estimated on the
        device first (``TuningEstimator``, N >= 32 768), from the same uploaded samples."""
        if len(wavs) == 0:
            return []
        estimate = isinstance(tuning_offsets, str)
        if estimate:
            if tuning_offsets != "estimate":
                raise ValueError(f"features_many: tuning_offsets is a sequence of cents, None or \"estimate\", got {tuning_offsets!r}")
            from .tuning import default_tuning_estimator
            songs = default_tuning_estimator(self._device()).check_songs(wavs)          # (its checks include those below; the samples are uploaded once)
            return self._features_checked(songs, [float(t) for t in default_tuning_estimator(self._device()).estimate_device(songs)[0]])
        if tuning_offsets is None:
            tuning_offsets = [0.0] * len(wavs)
        if len(tuning_offsets) != len(wavs):
            raise ValueError(f"features_many: {len(wavs)} songs but {len(tuning_offsets)} tuning offsets")
        for i, t in enumerate(tuning_offsets):
            if not abs(float(t)) <= 50.0:
                raise ValueError(f"song {i}: tuning_offset must be within +-50 cents, got {t}")
        return self._features_checked(mono_songs_to_device(wavs, self._device, 1, self.limits["max_samples"]), tuning_offsets)

    def _features_checked(self, songs: List[torch.Tensor], tuning_offsets: Sequence[float]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        dev = self._device()
        Ns = [int(t.numel()) for t in songs]
        out: List[Tuple[torch.Tensor, torch.Tensor]] = []
        with torch.cuda.device(dev):
            for group in self._batches(Ns, tuning_offsets):
                Ts = [self.num_frames(Ns[i]) for i in group]
                chroma = torch.empty(12 * sum(Ts), dtype=torch.float32, device=dev)
                dlnco = torch.empty(12 * sum(Ts), dtype=torch.float32, device=dev)
                ws = torch.empty(self.workspace_bytes([Ns[i] for i in group]), dtype=torch.uint8, device=dev)
                self.run_raw([songs[i] for i in group], [tuning_offsets[i] for i in group], chroma, dlnco, ws)
                off = 0
                for T in Ts:
                    out.append((chroma[off: off + 12 * T].view(12, T), dlnco[off: off + 12 * T].view(12, T)))
                    off += 12 * T
            hold(songs, dev)
        return out

    def features(self, wav, tuning_offset: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.features_many([wav], [tuning_offset])[0]

    def as_feature_fn(self, load_fn: Callable, tuning_fn: Union[None, str, Callable] = None) -> Callable:
        """-> the ``path -> (quantised chroma, DLNCO)`` callable ``AudioAligner(feature_fn=...)`` takes.  load_fn(path) -> mono samples at 22 050 Hz (``AudioLoader().as_load_fn()``
        for WAV files of any rate; other formats are the caller's); tuning_fn(path, samples) -> cents, default 0; ``tuning_fn="estimate"`` estimates it on the device."""
        if isinstance(tuning_fn, str) and tuning_fn != "estimate":
            raise ValueError(f"as_feature_fn: tuning_fn is a callable, None or \"estimate\", got {tuning_fn!r}")

        def fn(path):
            x = load_fn(path)
            if isinstance(tuning_fn, str):
                return self.features_many([x], "estimate")[0]
            return self.features(x, 0.0 if tuning_fn is None else float(tuning_fn(path, x)))
        return fn


_default: Dict[str, AlignFeatures] = {}


def default_align_features(device="cuda") -> AlignFeatures:
    """one ``AlignFeatures`` per device, made once"""
    key = str(torch.device(device))
    if key not in _default:
        _default[key] = AlignFeatures(device)
    return _default[key]
