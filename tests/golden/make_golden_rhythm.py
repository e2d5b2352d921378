#!/usr/bin/env python3
"""Generate tests/golden/rhythm_cases.npz by RUNNING THE REFERENCE's RGCCalculator and IPECalculator (etude/evaluation/metrics/rgc.py, ipe.py) on .json note files.

Runs only where the reference checkout, numpy and scikit-learn are available.  pretty_midi, which base_metric.py imports at its top and uses for .mid files only, is
replaced by an empty stub; the packages' own __init__ files are not run.  Every case stores its onsets and the reference's outputs (scores, error strings and the
KMeans labels of IPECalculator._quantize_ioi_to_symbols): data only.

The covers lie on a 16th-note grid at a random tempo, steps drawn from {1, 2, 3, 4, 6, 8, 16, 40, 80}, in three variants (exact, rounded to 1 ms, jittered by 10 ms)
at the lengths that can break the kernel, plus a single repeated IOI, IOIs all below 0.0625 s, one cover at the engine's limit and one past it.  Seeds of the lengths
above 40 are advanced until the restatement (tests/rhythm_np.py) never relocates an empty cluster on them: there scikit-learn's argpartition leaves a choice open.

Usage:  python tests/golden/make_golden_rhythm.py --reference DIR
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import rhythm_np as rn      # noqa: E402

LIMIT = 8192      # onsets per cover of the engine (etd_rhythm_limits)
LENGTHS = (0, 1, 2, 8, 9, 10, 12, 40, 255, 256, 257, 600, 1500)
STEPS = np.array([1, 2, 3, 4, 6, 8, 16, 40, 80])
STEP_P = np.array([0.30, 0.25, 0.10, 0.15, 0.05, 0.08, 0.04, 0.02, 0.01])


def load_reference(ref: str):
    ref = Path(ref)
    for pkg in ("etude", "etude.evaluation", "etude.evaluation.metrics"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(ref.joinpath(*pkg.split(".")))]
        sys.modules[pkg] = m
    sys.modules["pretty_midi"] = types.ModuleType("pretty_midi")
    import etude.evaluation.metrics.ipe as ipe
    import etude.evaluation.metrics.rgc as rgc
    return rgc, ipe


def grid(rng, n: int, variant: str) -> np.ndarray:
    if n == 0:
        return np.zeros(0)
    unit = 60.0 / rng.uniform(60.0, 180.0) / 4.0
    steps = rng.choice(STEPS, size=n, p=STEP_P)
    t = np.cumsum(steps) * unit
    if variant == "ms":
        t = np.round(t, 3)
    elif variant == "jitter":
        t = t + rng.normal(0.0, 0.010, n)
    return t


def write_notes(path: Path, onsets) -> None:
    path.write_text(json.dumps([{"pitch": 60, "onset": float(t), "offset": float(t) + 0.1, "velocity": 64} for t in onsets]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    rgc_mod, ipe_mod = load_reference(args.reference)
    base = sys.modules["etude.evaluation.metrics.base_metric"]
    rgc_calc, ipe_calc = rgc_mod.RGCCalculator(), ipe_mod.IPECalculator()

    cases = []      # (name, raw onsets)
    for n in LENGTHS:
        for v, variant in enumerate(("exact", "ms", "jitter")):
            seed = 1000 * n + v
            while True:
                t = grid(np.random.default_rng(seed), n, variant)
                u = np.unique(t)
                if n <= 40 or not rn.ipe(u)["relocated"]:
                    break
                seed += 100
            cases.append((f"n{n}_{variant}", t))
    cases.append(("single_ioi", np.arange(64) * 0.25))
    rng = np.random.default_rng(7)
    cases.append(("all_below_min", np.cumsum(rng.choice([0.01, 0.02, 0.03, 0.05], size=64))))
    for name, n in (("at_limit", LIMIT), ("past_limit", LIMIT + 1)):
        seed = 5
        while True:
            t = grid(np.random.default_rng(seed + n), n, "exact")
            if len(np.unique(t)) == n and not rn.ipe(np.unique(t))["relocated"]:
                break
            seed += 1
        cases.append((name, t))

    names, onsets, offsets, labels, label_offsets = [], [], [0], [], [0]
    rgc_score, rgc_tau, rgc_error, ipe_score, ipe_error, flagged = [], [], [], [], [], []
    with tempfile.TemporaryDirectory() as td:
        for name, t in cases:
            f = Path(td) / f"{name}.json"
            write_notes(f, t)
            u = base.get_onsets_from_file(f)      # what both calculators see: sorted, unique (empty below two notes)
            r, p = rgc_calc.calculate(f), ipe_calc.calculate(f)
            lab = np.zeros(0, np.int64)
            if "ipe_score" in p:
                lab = np.asarray(ipe_calc._quantize_ioi_to_symbols(ipe_calc._process_raw_ioi(np.diff(u))))
            names.append(name)
            onsets.append(np.asarray(u, np.float64)); offsets.append(offsets[-1] + len(u))
            labels.append(lab.astype(np.int8)); label_offsets.append(label_offsets[-1] + len(lab))
            rgc_score.append(float(r.get("rgc_score", np.nan))); rgc_tau.append(float(r.get("inferred_tau", np.nan))); rgc_error.append(r.get("error", ""))
            ipe_score.append(float(p.get("ipe_score", np.nan))); ipe_error.append(p.get("error", ""))
            flagged.append(bool(rn.ipe(u)["relocated"]))
    n_ok = sum(1 for e in ipe_error if not e)
    assert all(not fl for nm, fl, o0, o1 in zip(names, flagged, offsets, offsets[1:]) if o1 - o0 > 40), "a case above 40 onsets relocates"
    assert 4 * sum(flagged) <= len(names), (sum(flagged), len(names))
    assert {e for e in rgc_error if e} <= set(rn.RGC_ERRORS.values()) and {e for e in ipe_error if e} <= set(rn.IPE_ERRORS.values())
    path = HERE / "rhythm_cases.npz"
    np.savez_compressed(path, names=np.asarray(names), onsets=np.concatenate(onsets), offsets=np.asarray(offsets, np.int64), labels=np.concatenate(labels),
                        label_offsets=np.asarray(label_offsets, np.int64), rgc_score=np.asarray(rgc_score), rgc_tau=np.asarray(rgc_tau), rgc_error=np.asarray(rgc_error),
                        ipe_score=np.asarray(ipe_score), ipe_error=np.asarray(ipe_error), flagged=np.asarray(flagged), limit=np.int64(LIMIT))
    print("wrote", path, path.stat().st_size, "bytes;", len(names), "cases,", n_ok, "with an IPE score,", sum(flagged), "flagged")
    print("rgc errors:", sorted({e for e in rgc_error if e}))
    print("ipe errors:", sorted({e for e in ipe_error if e}))


if __name__ == "__main__":
    main()
