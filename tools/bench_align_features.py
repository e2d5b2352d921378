#!/usr/bin/env python3
"""Time the alignment features (etude_amd.AlignFeatures, csrc/alignfeat.hip) against the alignment they feed: 64 pairs (128 sides) of 3-minute mono audio at
22 050 Hz, generated on the device (``--pairs`` / ``--seconds`` cut it down).

From one run, each figure the median of ``--repeats`` windows that end in a device synchronise, after 2 warm-up calls:
  features_ms       ``features_many`` of all sides (sub-batched under the workspace budget)
  align_ms          ``align_many`` of the same pairs on those features
  launches_ms       the library's own event profiler around the launch groups of one profiled features call
  numpy_10s_s       for context: the fp64 numpy restatement (tests/alignfeat_np.py) of ONE 10-second side on the host
and the one condition DESIGN.md 4f states, read inside this run and asserted nowhere in advance: the features call takes less time than the alignment call.
The only derived figure is the floor: 1.5 G fp64 biquad updates per 3-minute side for the two filter passes (9 operations each, uncontracted) at the chip's fp64
vector rate without fused operations (39.3 T operations/s: half of the 78.6 TFLOP/s that counts a fused multiply-add as two).
Every GPU step runs under its own time limit (``--step-limit`` seconds): when one runs out, what was measured so far is written and the process ends with status 124
without starting anything more on the device; any other failure ends the process there too.  The limit is an alarm signal whose handler is Python code: it
ends a step that is slow, but it cannot run while the main thread is blocked inside a device synchronise or another HIP call, so a step that HANGS on the device is ended
only by a limit from outside (run the tool under ``timeout -k``); tools/bench_align.py is guarded the same way.
The input is reproducible: one seeded device generator for the samples and pitches, one seeded host generator for the note lengths.

Usage:  python tools/bench_align_features.py [--pairs 64] [--seconds 180] [--repeats 5] [--out profiles/r09_align_features.json]
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
sys.path.insert(0, str(ROOT / "tests"))


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
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--budget-gb", type=float, default=8.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align_features needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import _lib
    from etude_amd.aligner import DTWEngine
    from etude_amd.alignfeat import AlignFeatures, pitch_filterbank
    N = int(a.seconds * 22050)
    res = dict(pairs=a.pairs, seconds=a.seconds, samples=N, device=torch.cuda.get_device_name(0))

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

    af = AlignFeatures(workspace_budget=int(a.budget_gb * (1 << 30)))
    eng = DTWEngine()
    res.update(chunk=af.chunk, workspace_gb_per_side=af.workspace_bytes([N]) / 1e9, sub_batches=len(af._batches([N] * (2 * a.pairs))))

    def make():
        g = torch.Generator(device="cuda").manual_seed(1)
        gh = torch.Generator().manual_seed(1)
        t = torch.arange(N, device="cuda", dtype=torch.float64) / 22050.0
        wavs = []
        for s in range(2 * a.pairs):
            x = 1e-3 * torch.randn(N, generator=g, device="cuda", dtype=torch.float32)
            for _ in range(6):          # a few notes that change every 0.4 .. 1 s: a chord sequence of the side's own
                seg = (t / float(torch.empty(1).uniform_(0.4, 1.0, generator=gh))).long()
                pitch = torch.randint(40, 90, (int(seg.max()) + 1,), generator=g, device="cuda")[seg]
                f = 440.0 * torch.pow(2.0, (pitch.double() - 69.0) / 12.0)
                x += (0.05 * torch.sin(2 * np.pi * f * t)).float()
            wavs.append(x)
        torch.cuda.synchronize()
        return wavs
    wavs = step("generate", make)

    feats = []

    def run_features():
        feats[:] = af.features_many(wavs)
    res["features_ms"] = step("features", lambda: timed(run_features, a.repeats))
    pairs = [(feats[2 * i], feats[2 * i + 1]) for i in range(a.pairs)]
    res["align_ms"] = step("align", lambda: timed(lambda: eng.align_many(pairs), a.repeats))

    def profiled():
        _lib.prof_enable(True)
        _lib.prof_reset()
        af.features_many(wavs)
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        return {k: v["ms"] for k, v in rep.items() if k.startswith("k_af")}
    res["launches_ms"] = step("profiled", profiled)

    import alignfeat_np as R
    x = wavs[0][: 10 * 22050].cpu().numpy()
    bank = pitch_filterbank(0.0, af.chunk)
    t0 = time.perf_counter()
    R.features(x, bank)
    res["numpy_10s_s"] = time.perf_counter() - t0

    updates = 2.0 * sum(int(bank["n_sections"][b]) * (N // (1, 5, 25)[R.tier_of_pitch(21 + b)]) for b in range(88)) * 2 * a.pairs
    res["biquad_updates_two_passes"] = updates
    res["floor_ms"] = updates * 9.0 / 39.3e12 * 1e3
    res["features_under_align"] = bool(res["features_ms"]["median"] < res["align_ms"]["median"])
    write()


if __name__ == "__main__":
    main()
