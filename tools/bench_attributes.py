#!/usr/bin/env python3
"""Time the bar attributes (etude_amd.BarAttributes, csrc/attributes.hip) on what one bench step generates: 1 728 covers x 92 bar pairs of about 48 tokens per bar
(``--covers`` / ``--bars`` / ``--tokens`` cut it down), seeded, over the synthetic vocabulary of etude_amd.synth, and the restatement on the same pairs on the host.

  device   ``pairs_many`` end to end from the packed host arrays (ids + bar lengths, as ``generate_many(as_arrays=True)`` returns them) to the structured array on the
           host, bins included: the median of ``--repeats`` windows after 2 warm-up calls; the kernel alone by the library's event profiler around one further call.
  host     tests/attributes_np.py (plain Python) on the same pairs, one pass, in this process on this machine's CPU.
The results must be identical, and the one condition DESIGN.md 4i sets is stated inside the run: the device call is not slower than the host restatement.
The device step runs under its own time limit (``--step-limit`` seconds, an alarm; run the tool under ``timeout -k`` as well: the handler cannot run inside a HIP call).

Usage:  python tools/bench_attributes.py --out profiles/attributes_device.json
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def make_vocab():
    from etude_amd import synth
    from etude_amd.vocab import Vocab
    toks, special = synth.vocab_tokens(48)
    v = Vocab(special_tokens=special)
    for t in toks:
        v._add_token(t)
    return v


def make_bars(rng, v, n_bars: int, tokens: int):
    """(flat ids int32, bar lengths int64): [Bar_BOS, (Pos, (Note, Duration) x 1 .. 3) ..., Bar_EOS] of 0.6 .. 1.4 x `tokens` tokens, positions ascending"""
    bos, eos = v.get_bar_bos_id(), v.get_bar_eos_id()
    pos = [v.token_to_id[f"Pos_{i}"] for i in range(48)]
    note = [v.token_to_id[f"Note_{p}"] for p in range(21, 109)]
    dur = [v.token_to_id[f"Duration_{d}"] for d in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)]
    pool = []
    for _ in range(4096):                                    # distinct bars; a corpus draws from them
        want = int(rng.integers(int(0.6 * tokens), int(1.4 * tokens) + 1))
        bar, p = [bos], int(rng.integers(0, 4))
        while len(bar) < want - 1 and p < 48:
            bar.append(pos[p])
            for _ in range(int(rng.integers(1, 4))):
                bar += [note[int(rng.integers(0, len(note)))], dur[int(rng.integers(0, len(dur)))]]
            p += int(rng.integers(1, 5))
        pool.append(np.asarray(bar + [eos], np.int32))
    pick = rng.integers(0, len(pool), n_bars)
    return np.concatenate([pool[i] for i in pick]), np.asarray([len(pool[i]) for i in pick], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--covers", type=int, default=1728)
    ap.add_argument("--bars", type=int, default=92)
    ap.add_argument("--tokens", type=int, default=48)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attributes needs a ROCm GPU: there is no CPU path and no CPU timing stands in for the device")
    import attributes_np as an
    from etude_amd import _lib
    from etude_amd.attributes import BarAttributes, calculate_bin_edges
    v = make_vocab()
    rng = np.random.default_rng(a.seed)
    P = a.covers * a.bars
    src, tgt = make_bars(rng, v, P, a.tokens), make_bars(rng, v, P, a.tokens)
    res = dict(covers=a.covers, bars_per_cover=a.bars, pairs=P, tokens=int(src[0].size + tgt[0].size), seed=a.seed, device=torch.cuda.get_device_name(0), cpus=os.cpu_count())
    eng = BarAttributes(v)
    edges = calculate_bin_edges(eng.pairs_many(src, tgt))
    out = []

    def measure():
        for _ in range(2):
            eng.pairs_many(src, tgt, edges=edges)
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[:] = [eng.pairs_many(src, tgt, edges=edges)]      # (ends with the arrays on the host: the copy back synchronises)
            ms.append((time.perf_counter() - t0) * 1e3)
        res["pairs_many_ms"] = dict(median=statistics.median(ms), min=min(ms), max=max(ms))
        _lib.prof_enable(True)
        _lib.prof_reset()
        eng.pairs_many(src, tgt, edges=edges)
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        res["kernel_ms"] = rep.get("k_attr", {}).get("ms")

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
    host = an.Engine(eng.table)
    t0 = time.perf_counter()
    want = host.pairs_many(src, tgt, edges=edges)
    res["host_restatement_ms"] = (time.perf_counter() - t0) * 1e3
    res["identical"] = all(out[0][f].tobytes() == want[f].tobytes() for f in ("features", "attributes", "bins", "status"))
    res["not_slower_than_host"] = bool(res["pairs_many_ms"]["median"] <= res["host_restatement_ms"])
    res["bins"] = np.bincount(want["bins"].reshape(-1), minlength=3).tolist()
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    assert res["identical"], "the device and the restatement disagree"
    assert res["not_slower_than_host"], "the device call took longer than the restatement on the host"


if __name__ == "__main__":
    main()
