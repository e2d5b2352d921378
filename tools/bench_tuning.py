#!/usr/bin/env python3
"""Time the tuning estimator (etude_amd.TuningEstimator, csrc/tuning.hip) against the alignment features it feeds: 128 sides of 3-minute mono audio at 22 050 Hz,
generated on the device (``--sides`` / ``--seconds`` cut it down).

From one run, each figure the median of ``--repeats`` windows that end in a device synchronise, after 2 warm-up calls:
  estimate_ms       ``estimate_many`` of all sides (checks, three launches, the integers back on the host)
  frames_ms         the frame kernel alone, by the library's own event profiler around one profiled call (with the other two launches beside it)
  features_ms       ``AlignFeatures.features_many`` of the same sides at 0 cents, for context
and the one condition DESIGN.md 4g states, read inside this run and asserted nowhere in advance: estimating takes less time than the features it feeds.
The only derived figure is the floor: about 5 x 8 192 x 13 flops per frame, under 0.1 TFLOP for 128 sides -- the call is bound by launches and LDS traffic, not
arithmetic.
Every GPU step runs under its own time limit (``--step-limit`` seconds): when one runs out, what was measured so far is written and the process ends with status 124
without starting anything more on the device; any other failure ends the process there too.  The limit is an alarm signal whose handler is Python code: it cannot run
while the main thread is blocked inside a HIP call, so a step that HANGS on the device is ended only by a limit from outside (run the tool under ``timeout -k``), as
with tools/bench_align_features.py.

Usage:  python tools/bench_tuning.py [--sides 128] [--seconds 180] [--repeats 5] [--out profiles/r10_tuning.json]
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
    ap.add_argument("--sides", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--budget-gb", type=float, default=8.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tuning needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import _lib
    from etude_amd.alignfeat import AlignFeatures
    from etude_amd.tuning import TuningEstimator
    N = int(a.seconds * 22050)
    res = dict(sides=a.sides, seconds=a.seconds, samples=N, device=torch.cuda.get_device_name(0))

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

    est = TuningEstimator()
    af = AlignFeatures(workspace_budget=int(a.budget_gb * (1 << 30)))
    frames = est.num_frames(N)
    res.update(frames_per_side=frames, workspace_mb_per_side=est.workspace_bytes([N]) / 1e6)

    def make():
        g = torch.Generator(device="cuda").manual_seed(1)
        gh = torch.Generator().manual_seed(1)
        t = torch.arange(N, device="cuda", dtype=torch.float64) / 22050.0
        wavs = []
        for s in range(a.sides):
            x = 1e-3 * torch.randn(N, generator=g, device="cuda", dtype=torch.float32)
            cents = float(torch.empty(1).uniform_(-50.0, 50.0, generator=gh))          # every side its own detuning
            for _ in range(6):          # a few notes that change every 0.4 .. 1 s: a chord sequence of the side's own
                seg = (t / float(torch.empty(1).uniform_(0.4, 1.0, generator=gh))).long()
                pitch = torch.randint(40, 90, (int(seg.max()) + 1,), generator=g, device="cuda")[seg]
                f = 440.0 * torch.pow(2.0, (pitch.double() - 69.0 + cents / 100.0) / 12.0)
                x += (0.05 * torch.sin(2 * np.pi * f * t)).float()
            wavs.append(x)
        torch.cuda.synchronize()
        return wavs
    wavs = step("generate", make)

    tun = []

    def run_estimate():
        tun[:] = est.estimate_many(wavs).tolist()
    res["estimate_ms"] = step("estimate", lambda: timed(run_estimate, a.repeats))
    res["distinct_estimates"] = len(set(tun))

    def profiled():
        _lib.prof_enable(True)
        _lib.prof_reset()
        est.estimate_many(wavs)
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        return {k: v["ms"] for k, v in rep.items() if k.startswith("k_tn")}
    res["launches_ms"] = step("profiled", profiled)
    res["frames_ms"] = res["launches_ms"].get("k_tn_frames")

    res["features_ms"] = step("features", lambda: timed(lambda: af.features_many(wavs), a.repeats))

    flops = 5.0 * 8192 * 13 * frames * a.sides
    res["fft_flops"] = flops
    res["floor_ms"] = flops / 157.3e12 * 1e3          # (derived: the chip's fp32 vector peak; the call is nowhere near it by construction)
    res["estimate_under_features"] = bool(res["estimate_ms"]["median"] < res["features_ms"]["median"])
    write()
    assert res["estimate_under_features"], "estimating the tuning took longer than the features it feeds"


if __name__ == "__main__":
    main()
