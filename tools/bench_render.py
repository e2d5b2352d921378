"""Measure the note renderer (csrc/render.hip) on the GPU: 64 covers of random notes shaped like BASELINE's configs[0] -- about 92 bars at 120 bpm, about 8 notes
per bar, three minutes each -- and a dense variant with 4 times the notes; then ``align_notes_many`` end to end on the first set with its split into render,
features and DTW.  Median of 5 runs after 2 warm-ups, every run bracketed by a device synchronisation.

Usage:  python tools/bench_render.py --out profiles/render_bench.json [--covers 64] [--align-covers 16]

partial_samples counts (note, partial, sample) triples inside the notes' supports: the sine + exponential evaluations the kernel cannot avoid (it also evaluates, and
masks, the samples of a touched block that lie outside a note's support).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from etude_amd.aligner import align_features_many  # noqa: E402
from etude_amd.alignfeat import default_align_features  # noqa: E402
from etude_amd.render import NOTE_DTYPE, NoteRenderer  # noqa: E402

SR = 22050
BARS, BAR_SECONDS = 92, 2.0


def random_cover(rng, notes_per_bar):
    n = int(BARS * notes_per_bar)
    on = np.sort(rng.random(n) * BARS * BAR_SECONDS)
    a = np.zeros(n, NOTE_DTYPE)
    a["onset"], a["offset"] = on, on + 0.1 + rng.random(n) * 0.9
    a["pitch"], a["velocity"] = rng.integers(36, 97, n), rng.integers(40, 120, n)
    return a


def median_ms(fn, runs=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def partial_samples(r, covers):
    p = r.pack(covers)
    fe, _ = r.plan(p)
    K = np.zeros(len(p.notes), np.int64)
    v = r.voice
    f0 = 440.0 * 2.0 ** ((p.notes["pitch"] - 69) / 12.0)
    B = v.inharmonicity * 2.0 ** ((p.notes["pitch"] - 60) / v.inharmonicity_step)
    for k in range(1, v.partials + 1):
        K += (k * f0 * np.sqrt(1.0 + B * k * k) < v.nyquist_fraction * SR)
    return int(p.num_samples.sum()), int(((fe[:, 1] - fe[:, 0]) * K).sum()), int(len(p.notes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--covers", type=int, default=64)
    ap.add_argument("--align-covers", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render needs a ROCm GPU"
    r = NoteRenderer()
    res = {"device": torch.cuda.get_device_name(0), "covers": a.covers, "sample_rate": SR, "runs": 5, "warmups": 2}
    for name, npb in (("baseline_8_per_bar", 8), ("dense_32_per_bar", 32)):
        rng = np.random.default_rng(7)
        covers = [random_cover(rng, npb) for _ in range(a.covers)]
        samples, psamples, notes = partial_samples(r, covers)
        packed = r.pack(covers)
        ms_pack, _ = median_ms(lambda: r.pack(covers), 3, 1)
        ms, all_ms = median_ms(lambda: [t for _, ts in r.iter_rendered(packed) for t in ts])
        res[name] = dict(notes=notes, samples=samples, partial_samples=psamples, render_ms=ms, render_ms_runs=all_ms, pack_ms=ms_pack,
                         samples_per_s=samples / ms * 1e3, partial_samples_per_s=psamples / ms * 1e3, ms_per_cover=ms / a.covers)
        print(name, json.dumps(res[name]))
        if npb == 8:
            base = covers
    # end to end: the covers against origins that are the same notes under a linear map (rendered once, outside the clock)
    n = a.align_covers
    feats = default_align_features("cuda")
    origins = []
    for c in base[:n]:
        o = c.copy()
        o["onset"], o["offset"] = 1.05 * c["onset"] + 0.3, 1.05 * c["offset"] + 0.3
        origins.append(o)
    f_org = feats.features_many(r.render_many(origins))
    from etude_amd.aligner import align_notes_many
    ms_all, runs_all = median_ms(lambda: align_notes_many(list(zip(base[:n], f_org)), renderer=r, features=feats), 5, 2)
    xs = r.render_many(base[:n])
    ms_r, _ = median_ms(lambda: r.render_many(base[:n]))
    ms_f, _ = median_ms(lambda: feats.features_many(xs))
    f_cov = feats.features_many(xs)
    ms_d, _ = median_ms(lambda: align_features_many(list(zip(f_cov, f_org))))
    res["align_notes_many"] = dict(pairs=n, total_ms=ms_all, total_ms_runs=runs_all, render_ms=ms_r, features_ms=ms_f, dtw_ms=ms_d)
    print("align_notes_many", json.dumps(res["align_notes_many"]))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
