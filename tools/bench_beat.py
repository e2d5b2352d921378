#!/usr/bin/env python3
"""Beat-Transformer engine throughput on a prepare.py-like batch: full-architecture seeded weights, 16 ragged songs of 150-210 s, 5 stems, one ragged call.
Prints ms per song, audio-s/s, algorithmic TFLOP/s (and its share of the fp32-grade rate, 3 f16 MFMAs per product = 833 TFLOP/s, and of the 2.5 PFLOP/s f16 peak),
the per-kernel etd_prof table, and whether a song's logits are bit-identical alone and inside the batch.

usage: python tools/bench_beat.py [--songs 16] [--iters 3] [--warmup 1] [--seed 0]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from etude_amd import BeatDetector, _lib, synth  # noqa: E402

FPS = 44100 / 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    secs = rng.uniform(150, 210, a.songs)
    Ts = [int(s * FPS) for s in secs]
    det = BeatDetector(state_dict=synth.beat_state_dict(7))
    songs = [synth.beat_features(100 + i, T) for i, T in enumerate(Ts)]
    feat = torch.cat([torch.from_numpy(s).reshape(-1) for s in songs]).cuda()
    for _ in range(a.warmup):
        det._run(feat, Ts)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        lg, tp = det._run(feat, Ts)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    flops = sum(det.flops(T) for T in Ts)
    _lib.prof_enable(True)
    _lib.prof_reset()
    det._run(feat, Ts)
    prof = _lib.prof_report()
    _lib.prof_enable(False)
    solo, _ = det._run(torch.from_numpy(songs[3]).reshape(-1).cuda(), [Ts[3]])
    o = sum(Ts[:3])
    bitwise = bool(torch.equal(solo, lg[o:o + Ts[3]]))
    tfs = flops / t / 1e12
    print(f"{a.songs} songs, {sum(secs):.0f} s of audio, {sum(Ts)} frames: {t * 1e3:.1f} ms per batch (median of {a.iters}; {', '.join(f'{x * 1e3:.1f}' for x in times)})")
    print(f"  {t * 1e3 / a.songs:.2f} ms per song   {sum(secs) / t:.0f} audio-s/s   {flops / 1e12:.2f} TFLOP algorithmic -> {tfs:.1f} TFLOP/s "
          f"= {100 * tfs / 833:.1f} % of the fp32-grade rate (833), {100 * tfs / 2500:.1f} % of the f16 peak (2500)")
    print(f"  song 3 alone vs inside the batch: {'bit-identical' if bitwise else 'DIFFERENT'}")
    tot = sum(v["ms"] for v in prof.values())
    print(f"  {'kernel':<18}{'ms':>9}{'share':>8}{'launches':>10}{'TFLOP/s':>9}{'GB/s':>8}")
    for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        ms = v["ms"]
        print(f"  {k:<18}{ms:9.2f}{100 * ms / tot:7.1f}%{v['launches']:10d}{v['flops'] / ms / 1e9 if ms else 0:9.1f}{v['bytes'] / ms / 1e6 if ms else 0:8.0f}")
    print(json.dumps({"songs": a.songs, "ms_per_song": round(t * 1e3 / a.songs, 3), "audio_s_per_s": round(sum(secs) / t, 1), "tflops": round(tfs, 2),
                      "bitwise_solo_vs_batch": bitwise}))


if __name__ == "__main__":
    main()
