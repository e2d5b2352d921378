#!/usr/bin/env python3
"""Time the stem mel-dB features (etude_amd.StemFeatures, csrc/stemfeat.hip) and the route from separated stems to beat times: 64 songs x 5 stems x 2 channels x
3 minutes at 44.1 kHz, generated on the device (about 20 GB; ``--songs`` cuts it down).

Four figures from one run, each the median of ``--repeats`` windows that end in a device synchronise, after 2 warm-up calls:
  features_ms            the feature call alone (three launches for the whole batch)
  forward_ms             the Beat-Transformer forward pass of the same batch
  detect_stems_many_ms   stems on the device -> beat / downbeat times
  detect_many_ms         the same features held on the host -> beat / downbeat times (the route without device features: range check, concatenation and upload first)
and the two conditions DESIGN.md 4d states: the feature call takes less time than the forward pass, and detect_stems_many is no slower than detect_many.
The feature call is also set against a floor: every input byte read once at 8 TB/s plus the fp32 butterflies at the device's vector fp32 peak.
Every GPU step runs under its own time limit (``--step-limit`` seconds): when one runs out, what was measured so far is written and the process ends with status 124
without starting anything more on the device.

Usage:  python tools/bench_stem_features.py [--songs 64] [--seconds 180] [--repeats 5] [--out profiles/stem_features.json]
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8.0e12
FP32_VECTOR_FLOPS = 157.3e12


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_features needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import BeatDetector, StemFeatures, synth
    res = dict(songs=a.songs, seconds=a.seconds, device=torch.cuda.get_device_name(0))

    def write():
        print(json.dumps(res), flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    def step(name, fn):
        def expired(*_):
            res["timed_out_in"] = name
            write()
            os._exit(124)
        signal.signal(signal.SIGALRM, expired)
        signal.alarm(a.step_limit)
        try:
            return fn()
        finally:
            signal.alarm(0)

    sr, instr, channels = 44100, 5, 2
    N = int(a.seconds * sr)
    sf = StemFeatures()
    det = BeatDetector(state_dict=synth.beat_state_dict(7), tracker="native")

    def make():
        g = torch.Generator(device="cuda").manual_seed(1)
        t = torch.arange(N, device="cuda", dtype=torch.float32) / sr
        songs = []
        for s in range(a.songs):
            x = torch.randn((instr, channels, N), generator=g, device="cuda") * 1e-3
            beat = 0.5 + 0.5 * torch.cos(2 * np.pi * (1.5 + 0.02 * s) * t) ** 8          # a pulse at 90 + 1.2 s bpm
            for i in range(instr):
                x[i] += 0.1 * beat * torch.sin(2 * np.pi * (60.0 * 2 ** i + s) * t)
            songs.append(x)
        torch.cuda.synchronize()
        return songs
    stems = step("generate", make)
    res["input_gb"] = a.songs * instr * channels * N * 4 / 1e9
    T = sf.num_frames(N)
    res["frames_per_song"] = T

    res["features_ms"] = step("features", lambda: timed(lambda: sf.features_many(stems), a.repeats))
    feat, Ts = sf.features_many(stems)
    res["forward_ms"] = step("forward", lambda: timed(lambda: det._run(feat, Ts, want_tempo=False), a.repeats))
    res["detect_stems_many_ms"] = step("detect_stems_many", lambda: timed(lambda: det.detect_stems_many(stems, stem_features=sf), a.repeats))
    per = instr * T * 128
    host = feat.cpu().numpy()
    feats_host = [host[s * per:(s + 1) * per].reshape(instr, T, 128) for s in range(a.songs)]
    res["detect_many_ms"] = step("detect_many", lambda: timed(lambda: det.detect_many(feats_host), a.repeats))
    same = step("compare", lambda: det.detect_stems_many(stems, stem_features=sf) == det.detect_many(feats_host))
    res["detect_stems_many_equals_detect_many"] = bool(same)

    frames = a.songs * instr * T
    M, lgM = sf.n_fft // 2, (sf.n_fft // 2).bit_length() - 1
    flops = frames * (5.0 * M * lgM + 12.0 * M + 2.0 * 2009)
    floor_ms = (res["input_gb"] * 1e9 / HBM_BYTES_PER_S + flops / FP32_VECTOR_FLOPS) * 1e3
    res["feature_floor_ms"] = floor_ms
    res["feature_flops"] = flops
    res["features_over_floor"] = res["features_ms"]["median"] / floor_ms
    res["features_faster_than_forward"] = bool(res["features_ms"]["median"] < res["forward_ms"]["median"])
    res["detect_stems_many_not_slower_than_detect_many"] = bool(res["detect_stems_many_ms"]["median"] <= res["detect_many_ms"]["median"])
    write()


if __name__ == "__main__":
    main()
