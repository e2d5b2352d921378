#!/usr/bin/env python3
"""Generate tests/golden/tempo_cases.json by RUNNING THE REFERENCE's BeatAnalyzer (etude/data/beat_analyzer.py) on seeded beat_pred inputs.

Runs only where the reference checkout is available.  Each case stores its input ({"beat_pred", "downbeat_pred"}: what BeatDetector.detect writes) and the reference's
output (tempo.json content) -- data only.  The inputs are built here from a seed: bars of a given tempo and beat count with a few milliseconds of jitter, optional
holes (missing downbeats) between sections.  The generator asserts that each case shows the behaviour it is named for.

Usage:  python tests/golden/make_golden_tempo.py --reference DIR
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def song(seed, sections, jitter=0.003, start=0.4):
    """sections: (n_bars, bpm, beats per bar as detected, hole in measures AFTER the section); -> beat_pred.json content.  A section's bars carry `beats` beats
    each; the downbeat is also a beat (as the two trackers report it), displaced independently by the jitter."""
    rng = np.random.default_rng(seed)
    beats, downs, t = [], [], start
    for n_bars, bpm, per_bar, hole in sections:
        bar = 60.0 / bpm * 4 if per_bar != 3 else 60.0 / bpm * 3
        for _ in range(n_bars):
            for k in range(per_bar):
                bt = t + bar * k / per_bar + rng.normal(0, jitter)
                beats.append(bt)
                if k == 0:
                    downs.append(bt + rng.normal(0, jitter / 3))
            t += bar
        t += hole * bar
    return {"beat_pred": [float(x) for x in sorted(beats)], "downbeat_pred": [float(x) for x in sorted(downs)]}


def cases():
    c = []
    c.append(("steady_4_4", song(1, [(40, 120, 4, 0)])))
    c.append(("steady_3_4", song(2, [(40, 150, 3, 0)])))
    c.append(("two_beats_per_bar_reads_as_4", song(3, [(30, 100, 2, 0)])))
    c.append(("fewer_than_10_uniform_measures", song(4, [(8, 150, 3, 0)])))
    c.append(("tempo_change", song(5, [(20, 120, 4, 0), (20, 90, 4, 0)])))
    # (a region's last measure is the one that holds the hole, so the region's mean duration -- the unit the gap is measured in -- grows with the hole)
    c.append(("hole_of_1_measure_filled_with_whole_measures", song(6, [(16, 120, 4, 1), (16, 126, 4, 0)])))
    c.append(("hole_of_2_measures_filled_with_a_half_measure", song(7, [(16, 120, 4, 2), (16, 120, 4, 0)])))
    c.append(("gap_outside_tolerance", song(8, [(16, 120, 4, 0.15), (16, 120, 4, 0)])))
    c.append(("gap_of_3_5_measures_then_faster", song(9, [(12, 100, 4, 3.5), (14, 132, 4, 0)])))
    c.append(("regions_that_merge", song(10, [(14, 120, 4, 1), (14, 120.4, 4, 1), (14, 119.7, 4, 0)])))
    c.append(("no_downbeats", {"beat_pred": song(11, [(10, 120, 4, 0)])["beat_pred"], "downbeat_pred": []}))
    c.append(("fewer_than_4_measures", song(12, [(4, 120, 4, 0)])))
    c.append(("heavy_jitter_nothing_stable", song(13, [(24, 120, 4, 0)], jitter=0.25)))
    c.append(("three_sections_3_4", song(14, [(15, 140, 3, 2), (15, 140, 3, 0.5), (15, 170, 3, 0)])))
    d = song(15, [(30, 110, 4, 0)])
    d["beat_pred"] = [b for i, b in enumerate(d["beat_pred"]) if i % 7 != 3]          # missing beats: some measures are not uniform
    c.append(("missing_beats", d))
    d = song(16, [(30, 128, 4, 0)])
    d["beat_pred"] = sorted(d["beat_pred"] + [x + 0.06 for x in d["downbeat_pred"][::3]])   # spurious beats within 0.1 s of a downbeat are dropped
    c.append(("beats_close_to_downbeats", d))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from etude.data.beat_analyzer import BeatAnalyzer
    out = []
    with tempfile.TemporaryDirectory() as td:
        for name, data in cases():
            p = Path(td) / "beat_pred.json"
            p.write_text(json.dumps(data))
            res = BeatAnalyzer().analyze(p)
            res = json.loads(json.dumps(res))                    # plain Python numbers (numpy scalars would not serialise)
            out.append({"name": name, "input": data, "output": res})
            print(f"{name:34s} regions {len(res)}  " + "  ".join(f"{r['time_sig']}/4 {r['bpm']:.2f} x{len(r['downbeats'])}" for r in res))
    by = {c["name"]: c["output"] for c in out}
    assert by["steady_4_4"][0]["time_sig"] == 4 and len(by["steady_4_4"]) == 1
    assert by["steady_3_4"][0]["time_sig"] == 3
    assert by["two_beats_per_bar_reads_as_4"][0]["time_sig"] == 4
    assert by["fewer_than_10_uniform_measures"][0]["time_sig"] == 4
    assert len({round(r["bpm"]) for r in by["tempo_change"]}) >= 2
    g = by["hole_of_1_measure_filled_with_whole_measures"]
    assert all(r["time_sig"] == 4 for r in g) and sum(len(r["downbeats"]) for r in g) == 32 - 1          # 16 + 1 inserted, then 14 (a region needs its 4-measure window)
    assert any(r["time_sig"] == 2 for r in by["hole_of_2_measures_filled_with_a_half_measure"]) and any(r["time_sig"] == 2 for r in by["gap_of_3_5_measures_then_faster"])
    g = by["gap_outside_tolerance"]
    assert len(g) == 2 and all(r["time_sig"] == 4 for r in g) and sum(len(r["downbeats"]) for r in g) == 30          # nothing inserted
    assert len(by["regions_that_merge"]) < 3
    assert by["no_downbeats"] == [] and by["fewer_than_4_measures"] == []
    assert len(out) >= 12
    (HERE / "tempo_cases.json").write_text(json.dumps(out, indent=1))
    print("wrote tempo_cases.json", (HERE / "tempo_cases.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
