#!/usr/bin/env python3
"""Generate tests/golden/align_cases.json by RUNNING THE REFERENCE's host functions of stage 3 on seeded inputs: WPDCalculator (etude/evaluation/metrics/wpd.py),
compute_wp_std / create_time_map_from_downbeats / weakly_align (etude/utils/preprocess.py) and AudioAligner's wp.json cache (etude/data/aligner.py).

Runs only where the reference checkout is available.  The modules those files import at their top and never use in the functions called here -- librosa,
synctoolbox.*, pretty_midi -- are replaced by empty stubs, and so is the reference's logger; the packages' own __init__ files are not run.  Every case stores its
input and the reference's output: data only.

Usage:  python tests/golden/make_golden_align.py --reference DIR
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


class _Quiet:
    def __getattr__(self, name):
        return lambda *a, **k: None


def load_reference(ref: str):
    ref = Path(ref)
    for pkg in ("etude", "etude.utils", "etude.data", "etude.evaluation", "etude.evaluation.metrics"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(ref.joinpath(*pkg.split(".")))]
        sys.modules[pkg] = m
    for name in ("librosa", "pretty_midi", "synctoolbox", "synctoolbox.dtw", "synctoolbox.dtw.mrmsdtw", "synctoolbox.dtw.utils", "synctoolbox.feature",
                 "synctoolbox.feature.chroma", "synctoolbox.feature.dlnco", "synctoolbox.feature.pitch", "synctoolbox.feature.pitch_onset", "synctoolbox.feature.utils"):
        sys.modules[name] = _Anything(name)
    lg = types.ModuleType("etude.utils.logger")
    lg.logger = _Quiet()
    sys.modules["etude.utils.logger"] = lg
    import etude.data.aligner as al
    import etude.evaluation.metrics.wpd as wpd
    import etude.utils.preprocess as pp
    return wpd, pp, al


def plain(x):
    """numpy scalars / arrays -> plain Python (inf stays a float: Python's json writes and reads Infinity)"""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


def random_path(rng, n_cover, n_origin, wobble):
    """a strictly monotonic path from (0, 0) to (n_cover - 1, n_origin - 1) around a line with slow wobble"""
    L = int(min(n_cover, n_origin) * rng.uniform(0.6, 0.9))
    u = np.linspace(0, 1, L)
    dev = wobble * np.sin(2 * np.pi * (u * rng.uniform(1, 4) + rng.random())) * u * (1 - u)
    a = np.unique(np.clip(np.round(u * (n_cover - 1)).astype(int), 0, n_cover - 1))
    L = len(a)
    u = a / (n_cover - 1)
    b = np.clip(np.round((u + np.interp(u, np.linspace(0, 1, len(dev)), dev)) * (n_origin - 1)).astype(int), 0, n_origin - 1)
    b = np.maximum.accumulate(b)
    keep = np.concatenate([[True], np.diff(b) > 0])
    a, b = a[keep], b[keep]
    a[-1], b[-1] = n_cover - 1, n_origin - 1
    return np.stack([a, b]).astype(int)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    wpd, pp, al = load_reference(args.reference)
    rng = np.random.default_rng(20240612)
    out = {}

    # ---- WPD: sixteen paths x (subsample_step, trim_seconds)
    paths = []
    for k in range(13):
        n_c, n_o = int(rng.integers(250, 600)), int(rng.integers(250, 600))
        paths.append({"wp": random_path(rng, n_c, n_o, rng.uniform(0.0, 0.6)), "num_frames_cover": n_c, "num_frames_origin": n_o})
    paths.append({"wp": random_path(rng, 40, 45, 0.2)[:, :24], "num_frames_cover": 40, "num_frames_origin": 45})      # < 10 points once subsampled by 3
    paths.append({"wp": np.stack([np.arange(8), np.arange(8)]), "num_frames_cover": 8, "num_frames_origin": 8})         # < 10 points always
    paths.append({"wp": random_path(rng, 300, 300, 0.1), "num_frames_cover": 300})                                      # a key is missing
    wcases = []
    for p in paths:
        outs = []
        for step in (1, 3):
            for trim in (0, 2):
                res = wpd.WPDCalculator(subsample_step=step, trim_seconds=trim).calculate(dict(p))
                outs.append({"subsample_step": step, "trim_seconds": trim, "result": plain(res)})
        wcases.append({"align_result": plain(p), "outputs": outs})
    errs = {o["result"].get("error") for c in wcases for o in c["outputs"] if "error" in o["result"]}
    assert len(wcases) == 16 and len(errs) == 2, errs
    assert sum("wpd_score" in o["result"] for c in wcases for o in c["outputs"]) >= 50
    out["wpd"] = wcases

    # ---- time map + WP-Std
    tcases = []
    for k in range(6):
        n_c, n_o = int(rng.integers(300, 700)), int(rng.integers(300, 700))
        wp = random_path(rng, n_c, n_o, rng.uniform(0.05, 0.5))
        end = (n_o - 1) / 50
        downs = sorted(float(x) for x in rng.uniform(0, end * (1.3 if k % 2 else 1.0), 12))
        if k == 2:
            downs = [0.0, float(wp[1, 5] / 50), end, end + 1e-9, end + 3.0]      # on path points, at the end, just past it, far past it
        if k == 3:
            downs = [end + 1.0, end + 2.0]                                      # every downbeat past the path's end: an empty map
        tm = pp.create_time_map_from_downbeats(list(downs), {"wp": wp})
        tcases.append({"wp": wp.tolist(), "downbeats": downs, "feature_rate": 50, "time_map": plain(tm), "wp_std": float(pp.compute_wp_std(tm))})
    wp = random_path(rng, 400, 380, 0.3)
    tm = pp.create_time_map_from_downbeats([0.5, 1.5, 2.5], {"wp": wp}, feature_rate=25)
    tcases.append({"wp": wp.tolist(), "downbeats": [0.5, 1.5, 2.5], "feature_rate": 25, "time_map": plain(tm), "wp_std": float(pp.compute_wp_std(tm))})
    assert tcases[3]["time_map"] == [] and tcases[3]["wp_std"] == float("inf")
    assert any(len(c["time_map"]) < len(c["downbeats"]) and c["time_map"] for c in tcases)
    out["time_map"] = tcases

    # ---- weak alignment
    def notes(n, t_max):
        on = rng.uniform(-0.5, t_max, n)
        return [{"pitch": int(rng.integers(21, 109)), "onset": float(t), "offset": float(t + rng.uniform(0.05, 1.5)), "velocity": int(rng.integers(1, 128))} for t in on]
    acases = []
    for k in range(4):
        n = int(rng.integers(5, 12))
        s = np.cumsum(rng.uniform(1.5, 2.5, n))
        p = np.cumsum(rng.uniform(1.5, 2.5, n)) + rng.uniform(-1, 1)
        tm = [[float(a), float(b)] for a, b in zip(s, p)]
        if k == 1:
            tm[3][1] = tm[2][1] + 1e-7                      # a segment shorter than 1e-6 s: its notes are skipped
        if k == 2:
            order = rng.permutation(n)
            tm = [tm[i] for i in order]                     # unsorted on entry
        nt = notes(40, float(p[-1]) + 14.0)                 # some past the last anchor: the + 10 tail, and beyond it
        if k == 1:
            nt.append({"pitch": 60, "onset": tm[2][1] + 5e-8, "offset": tm[2][1] + 0.5, "velocity": 64})
        res = pp.weakly_align(copy.deepcopy(nt), copy.deepcopy(tm))
        acases.append({"notes": nt, "time_map": tm, "aligned": plain(res)})
    acases.append({"notes": [], "time_map": [[0.0, 0.0], [1.0, 1.0]], "aligned": plain(pp.weakly_align([], [[0.0, 0.0], [1.0, 1.0]]))})
    acases.append({"notes": notes(3, 2.0), "time_map": [], "aligned": []})
    last = max(p[1] for p in acases[0]["time_map"])
    assert any(n["onset"] >= last and n["onset"] < last + 10 for n in acases[0]["notes"]) and any(n["onset"] >= last + 10 for n in acases[0]["notes"])
    assert 0 < len(acases[1]["aligned"]) < len(acases[1]["notes"])
    out["weakly_align"] = acases

    # ---- the wp.json cache
    a = al.AudioAligner()
    with tempfile.TemporaryDirectory() as td:
        r1 = {"wp": random_path(rng, 120, 110, 0.2), "pitch_shift": -3, "num_frames_cover": 120, "num_frames_origin": 110}
        r2 = {"wp": random_path(rng, 90, 100, 0.1), "pitch_shift": 2, "num_frames_cover": 90, "num_frames_origin": 100}
        a._save_to_cache(td, "cover", r1)
        a._save_to_cache(td, "v2", r2)
        text = (Path(td) / "wp.json").read_text()
        everything = json.loads(text)
        everything["simple"] = r1["wp"].tolist()                                         # the simple format: a bare path
        everything["no_pitch_shift"] = {k: v for k, v in everything["v2"].items() if k != "pitch_shift"}
        everything["missing_key"] = {"wp": r2["wp"].tolist(), "num_frames_cover": 90}
        everything["not_a_dict"] = 7
        (Path(td) / "wp.json").write_text(json.dumps(everything, indent=4))
        loads = {k: plain(a._load_from_cache(td, k)) for k in ("cover", "v2", "simple", "no_pitch_shift", "missing_key", "not_a_dict", "absent")}
        (Path(td) / "wp.json").write_text(text[: len(text) // 2])                       # a truncated file
        broken = plain(a._load_from_cache(td, "cover"))
    assert loads["cover"]["pitch_shift"] == -3 and loads["no_pitch_shift"]["pitch_shift"] == 0
    assert loads["simple"] is None and loads["missing_key"] is None and loads["not_a_dict"] is None and loads["absent"] is None and broken is None
    out["cache"] = {"saved": [{"key": "cover", "result": plain(r1)}, {"key": "v2", "result": plain(r2)}], "file_text": text, "edited_file": everything,
                    "loads": loads, "truncated_file_load": broken}

    path = HERE / "align_cases.json"
    path.write_text(json.dumps(out, indent=None, separators=(",", ":")))
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
