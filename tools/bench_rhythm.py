#!/usr/bin/env python3
"""Time the rhythm metrics (etude_amd.RhythmMetrics, csrc/rhythm.hip) on what one bench step generates: 1 728 covers of about 1 000 onsets each, seeded, on a 16th-note
grid with 10 ms of jitter (``--covers`` / ``--onsets`` cut it down), and the reference's two calculators on the same lists on the host.

Two modes, two processes, one set of covers (the same seed):
  --mode device   ``metrics_many`` from the host lists to the host dicts (np.unique and packing, one copy in, one launch, two copies out, the dicts): the median of
                  ``--repeats`` windows that end with the results on the host, after 2 warm-up calls; the kernel alone by the library's event profiler around one
                  further call.  Needs a ROCm GPU.
  --mode host     ``RGCCalculator.calculate`` + ``IPECalculator.calculate`` of the reference checkout given by ``--reference`` on the covers written as .json note
                  files (their own reading included: it is what a host run pays), one pass, in a process that never imports torch: no GPU is opened.  Needs
                  scikit-learn; pretty_midi is replaced by an empty stub as in tests/golden/make_golden_rhythm.py.
Each mode writes its JSON (``--out``); ``--mode device --host-json FILE`` reads the host figure beside its own and states the one condition DESIGN.md 4h sets, asserted
nowhere in advance: the device batch is not slower than the host reference.
The device step runs under its own time limit (``--step-limit`` seconds, an alarm; run the tool under ``timeout -k`` as well: the handler cannot run inside a HIP call).

Usage:  python tools/bench_rhythm.py --mode host --reference DIR --out profiles/rhythm_host.json
        python tools/bench_rhythm.py --mode device --host-json profiles/rhythm_host.json --out profiles/rhythm_device.json
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
STEPS = np.array([1, 2, 3, 4, 6, 8, 16, 40, 80])
STEP_P = np.array([0.30, 0.25, 0.10, 0.15, 0.05, 0.08, 0.04, 0.02, 0.01])


def make_covers(n_covers: int, n_onsets: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    covers = []
    for _ in range(n_covers):
        n = int(rng.integers(int(0.8 * n_onsets), int(1.2 * n_onsets) + 1))
        unit = 60.0 / rng.uniform(60.0, 180.0) / 4.0
        covers.append(np.cumsum(rng.choice(STEPS, size=n, p=STEP_P)) * unit + rng.normal(0.0, 0.010, n))
    return covers


def run_host(a, covers, res):
    ref = Path(a.reference)
    for pkg in ("etude", "etude.evaluation", "etude.evaluation.metrics"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(ref.joinpath(*pkg.split(".")))]
        sys.modules[pkg] = m
    sys.modules["pretty_midi"] = types.ModuleType("pretty_midi")
    import etude.evaluation.metrics.ipe as ipe
    import etude.evaluation.metrics.rgc as rgc
    rc, ic = rgc.RGCCalculator(), ipe.IPECalculator()
    with tempfile.TemporaryDirectory() as td:
        files = []
        for i, t in enumerate(covers):
            f = Path(td) / f"{i}.json"
            f.write_text(json.dumps([{"pitch": 60, "onset": float(x), "offset": float(x) + 0.1, "velocity": 64} for x in t]))
            files.append(f)
        rc.calculate(files[0]); ic.calculate(files[0])      # warm-up: imports, thread pools
        t0 = time.perf_counter()
        r = [rc.calculate(f) for f in files]
        t1 = time.perf_counter()
        p = [ic.calculate(f) for f in files]
        t2 = time.perf_counter()
    res.update(rgc_ms=(t1 - t0) * 1e3, ipe_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3, per_cover_ms=(t2 - t0) * 1e3 / len(files),
               scores=sum("rgc_score" in x for x in r) + sum("ipe_score" in x for x in p), cpus=os.cpu_count())
    assert "torch" not in sys.modules


def run_device(a, covers, res):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rhythm --mode device needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import _lib
    from etude_amd.rhythm import RhythmMetrics
    res["device"] = torch.cuda.get_device_name(0)
    eng = RhythmMetrics()
    rows = []

    def call():
        rows[:] = eng.metrics_many(covers, details=True)

    def measure():
        for _ in range(2):
            call()
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()      # (ends with the results on the host: the copies back synchronise)
            ms.append((time.perf_counter() - t0) * 1e3)
        res["metrics_many_ms"] = dict(median=statistics.median(ms), min=min(ms), max=max(ms))
        t0 = time.perf_counter()
        packed, offsets = eng.pack(covers)
        res["pack_ms"] = (time.perf_counter() - t0) * 1e3
        _lib.prof_enable(True)
        _lib.prof_reset()
        eng.run_packed(packed, offsets)
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        res["kernel_ms"] = rep.get("k_rhythm", {}).get("ms")

    def expired(*_):
        res["timed_out"] = True
        print(json.dumps(res), flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.step_limit)
    try:
        measure()
    finally:
        signal.alarm(0)
    res.update(scores=sum("rgc_score" in x for x in rows) + sum("ipe_score" in x for x in rows), relocated=sum(x["relocated"] for x in rows),
               iterations_max=max(x["iterations"] for x in rows))
    if a.host_json:
        host = json.loads(Path(a.host_json).read_text())
        same = host["covers"] == res["covers"] and host["onsets"] == res["onsets"] and host["seed"] == res["seed"]
        res.update(host_total_ms=host["total_ms"], host_same_covers=same, not_slower_than_host=bool(res["metrics_many_ms"]["median"] <= host["total_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("device", "host"), required=True)
    ap.add_argument("--covers", type=int, default=1728)
    ap.add_argument("--onsets", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--reference", default="", help="--mode host: a checkout of the reference repository (Xiugapurin/Etude)")
    ap.add_argument("--host-json", default="", help="--mode device: the file a --mode host run wrote")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    covers = make_covers(a.covers, a.onsets, a.seed)
    res = dict(mode=a.mode, covers=a.covers, onsets=a.onsets, seed=a.seed, total_onsets=int(sum(len(c) for c in covers)))
    if a.mode == "host":
        if not a.reference:
            raise SystemExit("--mode host needs --reference DIR")
        run_host(a, covers, res)
    else:
        run_device(a, covers, res)
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if a.mode == "device" and a.host_json:
        assert res["host_same_covers"], "the host figure was measured on other covers"
        assert res["not_slower_than_host"], "the device batch took longer than the reference's calculators on the host"


if __name__ == "__main__":
    main()
