"""fp64 restatement of the DBN beat / downbeat trackers (madmom 0.16's DBNBeatTrackingProcessor / DBNDownBeatTrackingProcessor from their published
description).  A helper, not a test.

The transition model is a DENSE [S][S] log matrix and the backpointers a full [T][S] array, so nothing here shares structure with the kernel's sparse form
(csrc/dbn.hip).  ``viterbi(..., dense=False)`` is the same recursion with the matrix product restricted to its non-(-inf) blocks: it exists because the dense step
costs S^2 per frame (7 M at the 4-beat bar, minutes for a 3-minute song) and is held bitwise equal to the dense one by tests/test_dbn_cpu.py.

Arithmetic that decides bits is written out: tables use ``math.exp`` / ``math.log`` one value at a time and left-to-right sums (what the library's host tables do), the
recursion is ``(prev + logtrans) + density``, ties go to the lowest predecessor index among the predecessors that have an edge, the final state is the lowest index of
the maximum.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

NINF = -math.inf


@dataclass
class HMM:
    num_beats: int
    bar: bool                       # False: the beat HMM (2 densities), True: a bar HMM (3)
    intervals: np.ndarray           # [n] int
    S: int = 0
    position: np.ndarray = None     # [S] float64
    pointer: np.ndarray = None      # [S] int
    first_states: np.ndarray = None  # [num_beats][n]
    last_states: np.ndarray = None
    lt: np.ndarray = None           # [n from][n to] log transition between beats, -inf = no edge
    _dense: Optional[np.ndarray] = field(default=None, repr=False)

    @property
    def K(self):
        return 3 if self.bar else 2

    def dense(self) -> np.ndarray:
        """[S from][S to] log transition matrix"""
        if self._dense is None:
            A = np.full((self.S, self.S), NINF)
            n = len(self.intervals)
            firsts = set(int(x) for x in self.first_states.reshape(-1))
            for s in range(1, self.S):
                if s not in firsts:
                    A[s - 1, s] = 0.0                      # log(1)
            for b in range(self.num_beats):
                pb = (b - 1) % self.num_beats
                for f in range(n):
                    for t in range(n):
                        A[self.last_states[pb, f], self.first_states[b, t]] = self.lt[f, t]
            self._dense = A
        return self._dense


def intervals_of(fps: float, min_bpm: float, max_bpm: float, num_tempi: Optional[int] = None) -> np.ndarray:
    min_interval, max_interval = 60.0 * fps / max_bpm, 60.0 * fps / min_bpm
    iv = np.arange(np.round(min_interval), np.round(max_interval) + 1)
    if num_tempi and num_tempi < len(iv):
        n = num_tempi
        while True:
            iv = np.unique(np.round(np.logspace(np.log2(min_interval), np.log2(max_interval), n, base=2)))
            if len(iv) >= num_tempi:
                break
            n += 1
    return iv.astype(np.int64)


def transitions(iv: Sequence[int], transition_lambda: float) -> np.ndarray:
    """[from][to] log probabilities of last state of `from` -> first state of `to`"""
    n = len(iv)
    out = np.full((n, n), NINF)
    eps = float(np.spacing(1.0))
    for f in range(n):
        row = []
        for t in range(n):
            p = math.exp(-transition_lambda * abs(float(iv[t]) / float(iv[f]) - 1.0))
            row.append(0.0 if p <= eps else p)
        total = 0.0
        for p in row:
            total += p
        for t in range(n):
            if row[t] != 0.0:
                out[f, t] = math.log(row[t] / total)
    return out


def make_hmm(fps, min_bpm, max_bpm, num_beats=None, transition_lambda=100.0, observation_lambda=16.0, num_tempi=None) -> HMM:
    iv = intervals_of(fps, min_bpm, max_bpm, num_tempi)
    bar = num_beats is not None
    B = num_beats if bar else 1
    per = int(iv.sum())
    h = HMM(B, bar, iv, S=per * B)
    first = np.cumsum(np.r_[0, iv[:-1]])
    last = np.cumsum(iv) - 1
    h.first_states = np.stack([first + b * per for b in range(B)])
    h.last_states = np.stack([last + b * per for b in range(B)])
    pos = np.empty(h.S)
    for b in range(B):
        for j, i in enumerate(iv):
            for k in range(int(i)):
                pos[b * per + first[j] + k] = k / float(i) + b
    h.position = pos
    border = 1.0 / observation_lambda
    ptr = np.zeros(h.S, np.int64)
    if bar:
        ptr[np.array([math.fmod(p, 1.0) < border for p in pos])] = 1
        ptr[pos < border] = 2
    else:
        ptr[pos < border] = 1
    h.pointer = ptr
    h.lt = transitions(iv, transition_lambda)
    return h


def viterbi(h: HMM, dens: np.ndarray, dense: bool = True):
    """dens [T][K] fp64 log densities -> (path [T] int, log probability)"""
    T, S = len(dens), h.S
    v = np.full(S, math.log(1.0 / S))
    bp = np.zeros((T, S), np.int16)
    n = len(h.intervals)
    with np.errstate(invalid="ignore"):
        if dense:
            A = h.dense()
            edge = A > NINF
            first_edge = np.argmax(edge, axis=0)
            for t in range(T):
                cand = v[:, None] + A
                m = cand.max(axis=0)
                a = cand.argmax(axis=0)
                a = np.where(m == NINF, first_edge, a)
                bp[t] = a
                v = m + dens[t][h.pointer]
        else:
            edge = h.lt > NINF
            first_edge = np.argmax(edge, axis=0)
            idx = np.arange(S)
            for t in range(T):
                m = np.empty(S)
                m[1:] = v[:-1] + 0.0
                a = idx - 1
                for b in range(h.num_beats):
                    lasts = h.last_states[(b - 1) % h.num_beats]
                    cand = v[lasts][:, None] + h.lt
                    mm = cand.max(axis=0)
                    aa = np.where(mm == NINF, first_edge, cand.argmax(axis=0))
                    m[h.first_states[b]] = mm
                    a[h.first_states[b]] = lasts[aa]
                bp[t] = a
                v = m + dens[t][h.pointer]
    state = int(np.argmax(v))
    logp = float(v[state])
    path = np.empty(T, np.int64)
    path[T - 1] = state
    for t in range(T - 1, 0, -1):
        state = int(bp[t, state])
        path[t - 1] = state
    return path, logp


@dataclass
class TrackerCfg:
    fps: float
    min_bpm: float = 55.0
    max_bpm: float = 215.0
    threshold: float = 0.0
    transition_lambda: float = 100.0
    observation_lambda: float = 16.0
    num_tempi: Optional[int] = None
    beats_per_bar: Sequence[int] = (3, 4)


def _trim(act: np.ndarray, threshold: float):
    """-> (trimmed, first).  `idx.any()` is False when the only index is 0 (kept quirk)."""
    first = 0
    if threshold:
        hit = act >= np.float32(threshold)
        idx = np.nonzero(hit.any(axis=1) if act.ndim == 2 else hit)[0]
        if idx.any():
            first = int(idx.min())
            last = min(len(act), int(idx.max()) + 1)
        else:
            last = first = 0
        act = act[first:last]
    return act, first


def _perturb(d: np.ndarray, eps: float, mode: int) -> np.ndarray:
    if not eps:
        return d
    if mode == 0:
        s = 1.0
    elif mode == 1:
        s = -1.0
    else:
        s = np.random.default_rng(12345).choice([-1.0, 1.0], size=d.shape)
    with np.errstate(invalid="ignore"):
        return d * (1.0 + eps * s)


def beat_densities(act: np.ndarray, observation_lambda: float) -> np.ndarray:
    a = act.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.log((1.0 - a) / (observation_lambda - 1.0)), np.log(a)], axis=1)


def bar_densities(act: np.ndarray, observation_lambda: float) -> np.ndarray:
    s = (act[:, 0] + act[:, 1]).astype(np.float64)               # the sum in fp32, everything after it in fp64
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.log((1.0 - s) / (observation_lambda - 1.0)), np.log(act[:, 0].astype(np.float64)), np.log(act[:, 1].astype(np.float64))], axis=1)


def _runs(r: np.ndarray):
    borders = np.nonzero(np.diff(r.astype(np.int64)))[0] + 1
    if r[0]:
        borders = np.r_[0, borders]
    if r[-1]:
        borders = np.r_[borders, len(r)]
    if not borders.any():
        return []
    return [(int(l), int(rr)) for l, rr in borders.reshape(-1, 2)]


def track_beats(act: np.ndarray, cfg: TrackerCfg, hmm: Optional[HMM] = None, eps: float = 0.0, mode: int = 0, dense: bool = False) -> np.ndarray:
    """act [T] float32 -> absolute beat frames (int64); times are frames / fps"""
    act = np.asarray(act, np.float32)
    act, first = _trim(act, cfg.threshold)
    if len(act) == 0 or not act.any():
        return np.zeros(0, np.int64)
    h = hmm or make_hmm(cfg.fps, cfg.min_bpm, cfg.max_bpm, None, cfg.transition_lambda, cfg.observation_lambda, cfg.num_tempi)
    path, logp = viterbi(h, _perturb(beat_densities(act, cfg.observation_lambda), eps, mode), dense)
    if logp == NINF:
        return np.zeros(0, np.int64)
    r = h.pointer[path]
    return np.array([int(np.argmax(act[l:rr])) + l + first for l, rr in _runs(r)], np.int64)


def track_downbeats(act: np.ndarray, cfg: TrackerCfg, hmms: Optional[List[HMM]] = None, eps: float = 0.0, mode: int = 0, dense: bool = False):
    """act [T][2] float32 = (max(beat - downbeat, 0), downbeat) -> (rows [n][2] int64 of (absolute frame, beat number), index of the chosen bar length or -1)"""
    act = np.asarray(act, np.float32)
    act, first = _trim(act, cfg.threshold)
    if len(act) == 0 or not act.any():
        return np.zeros((0, 2), np.int64), -1
    hs = hmms or [make_hmm(cfg.fps, cfg.min_bpm, cfg.max_bpm, b, cfg.transition_lambda, cfg.observation_lambda, cfg.num_tempi) for b in cfg.beats_per_bar]
    d = _perturb(bar_densities(act, cfg.observation_lambda), eps, mode)
    res = [viterbi(h, d, dense) for h in hs]
    best = int(np.argmax([lp for _, lp in res]))
    path, logp = res[best]
    if logp == NINF:
        return np.zeros((0, 2), np.int64), -1
    h = hs[best]
    r = h.pointer[path] >= 1
    rows = []
    for l, rr in _runs(r):
        peak = int(np.argmax(act[l:rr])) // 2 + l
        rows.append((peak + first, int(h.position[path[peak]]) + 1))
    return np.array(rows, np.int64).reshape(-1, 2), best


def combined(beat: np.ndarray, down: np.ndarray) -> np.ndarray:
    return np.stack([np.maximum(beat - down, 0), down], axis=-1).astype(np.float32)


def detect(beat: np.ndarray, down: np.ndarray, cfg: TrackerCfg, hmms=None) -> dict:
    """what BeatDetector.detect returns for these activations"""
    bh, dh = (hmms[0], hmms[1:]) if hmms else (None, None)
    b = track_beats(beat, cfg, bh)
    rows, _ = track_downbeats(combined(beat, down), cfg, dh)
    return {"beat_pred": (b.astype(np.float64) / cfg.fps).tolist(), "downbeat_pred": (rows[rows[:, 1] == 1][:, 0].astype(np.float64) / cfg.fps).tolist()}
