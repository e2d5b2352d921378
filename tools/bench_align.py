#!/usr/bin/env python3
"""Time the exact DTW alignment (etude_amd.aligner, csrc/dtw.hip): 64 pairs of 9 000 x 9 000 frames (two 3-minute songs at 50 features/s), generated on the device
(``--pairs`` / ``--frames`` cut it down).

From one run, each figure the median of ``--repeats`` windows that end in a device synchronise, after 2 warm-up calls:
  single_ms         one pair alone (all five launches, the result copied to the host)
  batch_ms          the whole batch in one ragged call
  shift_launch_ms   the transposition launch alone (12 CENS DTWs per pair; the library's own event profiler around that launch, from one profiled batch call)
  final_launch_ms   the final DTW launch alone, from the same call
  numpy_2000_s      for context: the fp64 numpy restatement (tests/dtw_np.py) of ONE 2 000 x 2 000 pair on the host
and the two conditions DESIGN.md 4e states, read inside this run and asserted nowhere in advance: the batch takes less than twice the single pair (64 independent
workgroups on 256 CUs; the factor 2 is for clocks and backpointer traffic), and the transposition launch takes less than the final one.
Every GPU step runs under its own time limit (``--step-limit`` seconds): when one runs out, what was measured so far is written and the process ends with status 124
without starting anything more on the device; any other failure ends the process there too.

Usage:  python tools/bench_align.py [--pairs 64] [--frames 9000] [--repeats 5] [--out profiles/r08_align.json]
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
    ap.add_argument("--frames", type=int, default=9000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import _lib
    from etude_amd.aligner import DTWEngine, limits
    res = dict(pairs=a.pairs, frames=a.frames, device=torch.cuda.get_device_name(0), **limits())

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

    eng = DTWEngine()
    N = a.frames

    def make():
        g = torch.Generator(device="cuda").manual_seed(1)
        seg = torch.arange(N, device="cuda") // 40
        pairs = []
        for p in range(a.pairs):
            sides = []
            for side in range(2):
                root = torch.randint(0, 12, (N // 40 + 1,), generator=g, device="cuda")[seg] if side == 0 else (sides[0][2] + 3) % 12
                chroma = torch.zeros((12, N), device="cuda")
                cols = torch.arange(N, device="cuda")
                for iv, v in ((0, 4.0), (4, 3.0), (7, 3.0)):
                    chroma[(root + iv) % 12, cols] = v
                chroma += (torch.rand((12, N), generator=g, device="cuda") < 0.05).float()
                dl = torch.rand((12, N), generator=g, device="cuda") * (torch.rand((12, N), generator=g, device="cuda") < 0.1)
                sides.append((chroma, dl, root))
            pairs.append(((sides[1][0], sides[1][1]), (sides[0][0], sides[0][1])))      # the cover is the origin transposed by 3, with noise of its own
        torch.cuda.synchronize()
        return pairs
    pairs = step("generate", make)
    tensors = [eng._pair(i, c, o) for i, (c, o) in enumerate(pairs)]
    ws_bytes, res_ints, _ = eng.workspace_bytes([N] * a.pairs, [N] * a.pairs)
    res["workspace_gb"] = ws_bytes / 1e9
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(res_ints, dtype=torch.int32, device="cuda")

    res["single_ms"] = step("single", lambda: timed(lambda: eng.align_raw(tensors[:1], ws, out), a.repeats))
    res["batch_ms"] = step("batch", lambda: timed(lambda: eng.align_raw(tensors, ws, out), a.repeats))

    def profiled():
        _lib.prof_enable(True)
        _lib.prof_reset()
        eng.align_raw(tensors, ws, out)
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        return {k: v["ms"] for k, v in rep.items() if k.startswith("k_dtw")}
    launches = step("profiled", profiled)
    res["launches_ms"] = launches
    res["shift_launch_ms"], res["final_launch_ms"] = launches.get("k_dtw_shift"), launches.get("k_dtw_final")
    host, off = eng.align_raw(tensors, ws, out)
    res["opt_shifts"] = sorted({int(host[o + 1]) for o in off})
    res["path_lengths"] = [int(min(host[o] for o in off)), int(max(host[o] for o in off))]

    import dtw_np as R
    rng = np.random.default_rng(0)
    c, o = R.random_pair(rng, 2000, 2000)
    t0 = time.perf_counter()
    R.align(c, o)
    res["numpy_2000_s"] = time.perf_counter() - t0

    cells = float(a.pairs) * N * N
    res["batch_gcells_per_s"] = cells / (res["batch_ms"]["median"] * 1e-3) / 1e9
    res["batch_under_twice_single"] = bool(res["batch_ms"]["median"] < 2 * res["single_ms"]["median"])
    res["shift_launch_under_final_launch"] = bool(res["shift_launch_ms"] < res["final_launch_ms"])
    write()


if __name__ == "__main__":
    main()
