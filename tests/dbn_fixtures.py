"""Activation fixtures shared by tests/test_dbn_cpu.py (which proves each one robust: the restatement's output does not move when its densities are perturbed by
1e-12 relative, so an ulp of difference between the device's log and numpy's cannot change it) and tests/test_gpu_dbn.py (trackers against the restatement).
A helper, not a test."""
from __future__ import annotations

import functools

import numpy as np

import dbn_np
from etude_amd import synth

FPS = 44100 / 1024
CFG = dbn_np.TrackerCfg(fps=FPS, min_bpm=70.0, max_bpm=250.0, threshold=0.2, beats_per_bar=(3, 4))          # BeatDetectorConfig's defaults
CFG_NO_THRESHOLD = dbn_np.TrackerCfg(fps=FPS, min_bpm=70.0, max_bpm=250.0, threshold=0.0, beats_per_bar=(3, 4))
T = 1200


@functools.lru_cache(maxsize=None)
def hmms():
    """[beat HMM, 3-beat bar, 4-beat bar] of CFG (the model does not depend on the threshold)"""
    return [dbn_np.make_hmm(FPS, 70.0, 250.0, b) for b in (None, 3, 4)]


def _silence(act, lo, hi):
    act = act.copy()
    act[:lo] *= 0.5
    act[hi:] *= 0.5
    act[:lo] = np.minimum(act[:lo], 0.15)
    act[hi:] = np.minimum(act[hi:], 0.15)
    return act


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (act [T][2] float32 of (beat, downbeat), cfg, planted [n][2] or None, beats per bar of the material or None)"""
    f = {}
    a, p = synth.beat_activations(21, T, ((None, 120.0),), 4, jitter=0.004)
    f["steady_4_4"] = (a, CFG, p, 4)
    a, p = synth.beat_activations(22, T, ((12.0, 100.0), (None, 140.0)), 4, jitter=0.004)
    f["tempo_change"] = (a, CFG, p, 4)
    a, p = synth.beat_activations(23, T, ((None, 132.0),), 3, jitter=0.004)
    f["steady_3_4"] = (a, CFG, p, 3)
    a, p = synth.beat_activations(24, T, ((None, 110.0),), 4, jitter=0.0)
    f["silence_at_both_ends"] = (_silence(a, 170, 1010), CFG, None, 4)
    a, _ = synth.beat_activations(25, 400, ((None, 120.0),), 4)
    f["all_below_threshold"] = ((a * 0.2).astype(np.float32), CFG, None, None)
    a = np.full((300, 2), 0.05, np.float32)
    a[0] = (0.9, 0.3)
    f["only_frame_0_above_threshold"] = (a, CFG, None, None)
    f["one_frame"] = (np.array([[0.7, 0.2]], np.float32), CFG, None, None)
    f["one_frame_no_threshold"] = (np.array([[0.7, 0.2]], np.float32), CFG_NO_THRESHOLD, None, None)
    a, p = synth.beat_activations(26, 900, ((None, 125.0),), 4)
    a = a.copy()
    for k, (fr, num) in enumerate(p):
        if k % 3 == 0:
            a[fr] = (1.0, 1.0 if num == 1 else 0.0)             # exact 1.0: log(1 - a) = -inf
    a[5::37] = 0.0                                               # exact 0.0: log(a) = -inf
    a[np.array([fr for fr, _ in p])] = np.maximum(a[np.array([fr for fr, _ in p])], 0.3)
    f["exact_zeros_and_ones"] = (a.astype(np.float32), CFG, None, 4)
    return f


def restated(name, eps=0.0, mode=0):
    """-> (beat frames, downbeat rows, index of the chosen bar length)"""
    act, cfg, _, _ = fixtures()[name]
    h = hmms()
    beats = dbn_np.track_beats(act[:, 0], cfg, h[0], eps, mode)
    rows, choice = dbn_np.track_downbeats(dbn_np.combined(act[:, 0], act[:, 1]), cfg, h[1:], eps, mode)
    return beats, rows, choice
