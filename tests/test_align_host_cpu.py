"""The host functions of stage 3 against tests/golden/align_cases.json -- the reference's own outputs (tests/golden/make_golden_align.py): WPDCalculator, the time map
from downbeats, WP-Std, the weak alignment and AudioAligner's wp.json cache.  Floats to 1e-12 relative, everything else exactly."""
import copy
import json
import math

import numpy as np
import pytest

from etude_amd.aligner import AudioAligner, filter_and_weakly_align
from etude_amd.evaluation import WPDCalculator, wpd_many
from etude_amd.preprocess import compute_wp_std, create_time_map_from_downbeats, weakly_align

RTOL = 1e-12


@pytest.fixture(scope="module")
def cases(golden_dir):
    return json.loads((golden_dir / "align_cases.json").read_text())


def close(a, b):
    """the same structure; floats to 1e-12 relative (inf equal to inf), the rest exactly"""
    if isinstance(b, dict):
        return isinstance(a, dict) and a.keys() == b.keys() and all(close(a[k], b[k]) for k in b)
    if isinstance(b, list):
        return isinstance(a, (list, tuple)) and len(a) == len(b) and all(close(x, y) for x, y in zip(a, b))
    if isinstance(b, float):
        a = float(a)
        return a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= RTOL * max(abs(a), abs(b)))
    return a == b and not isinstance(a, float)


def _result(d):
    d = dict(d)
    d["wp"] = np.array(d["wp"], dtype=int)
    return d


def test_wpd_calculator_matches_the_reference_on_sixteen_paths(cases):
    seen_err, n_scores = set(), 0
    assert len(cases["wpd"]) == 16
    for c in cases["wpd"]:
        for o in c["outputs"]:
            got = WPDCalculator(subsample_step=o["subsample_step"], trim_seconds=o["trim_seconds"]).calculate(_result(c["align_result"]))
            want = o["result"]
            assert got.keys() == want.keys(), (got, want)
            if "error" in want:
                assert got["error"] == want["error"]
                seen_err.add(want["error"])
            else:
                assert close(float(got["wpd_score"]), want["wpd_score"]), (got, want)
                n_scores += 1
    assert len(seen_err) == 2 and n_scores >= 50


def test_wpd_constructor_checks_and_batch_form(cases):
    for bad in (dict(subsample_step=0), dict(subsample_step=1.0), dict(trim_seconds=-1), dict(trim_seconds="2")):
        with pytest.raises(ValueError):
            WPDCalculator(**bad)
    rs = [_result(c["align_result"]) for c in cases["wpd"][:3]] + [None]
    many = wpd_many(rs, subsample_step=3, trim_seconds=2)
    for c, got in zip(cases["wpd"][:3], many):
        want = [o for o in c["outputs"] if o["subsample_step"] == 3 and o["trim_seconds"] == 2][0]["result"]
        assert close({k: float(v) if k == "wpd_score" else v for k, v in got.items()}, want)
    assert "error" in many[3]


def test_time_map_and_wp_std_match_the_reference(cases):
    empties = 0
    for c in cases["time_map"]:
        tm = create_time_map_from_downbeats(c["downbeats"], {"wp": np.array(c["wp"], dtype=int)}, c["feature_rate"])
        assert close(tm, c["time_map"]), (tm[:3], c["time_map"][:3])
        assert all(type(x) is float for p in tm for x in p)
        assert close(float(compute_wp_std(tm)), c["wp_std"])
        empties += not tm
    assert empties == 1 and compute_wp_std([]) == float("inf")


def test_weakly_align_matches_the_reference(cases):
    for c in cases["weakly_align"]:
        tm = copy.deepcopy(c["time_map"])
        got = weakly_align(copy.deepcopy(c["notes"]), tm)
        assert close(got, c["aligned"])
        assert tm == sorted(c["time_map"], key=lambda p: p[1])      # sorted in place, as the reference leaves it


def test_wp_json_cache_round_trip_matches_the_reference(cases, tmp_path):
    g = cases["cache"]
    a = AudioAligner()
    assert (a.fs, a.feature_rate, a.threshold_rec) == (22050, 50, 10 ** 6)
    assert a.step_weights.tolist() == [1.5, 1.5, 2.0] and a.win_len_smooth.tolist() == [101, 51, 21, 1]
    for s in g["saved"]:
        a._save_to_cache(tmp_path, s["key"], _result(s["result"]))
    assert (tmp_path / "wp.json").read_text() == g["file_text"]          # the file itself, byte for byte
    (tmp_path / "wp.json").write_text(json.dumps(g["edited_file"], indent=4))
    for key, want in g["loads"].items():
        got = a._load_from_cache(tmp_path, key)
        if want is None:
            assert got is None, key
        else:
            assert isinstance(got["wp"], np.ndarray) and got["wp"].dtype == np.array([0], dtype=int).dtype
            got = dict(got); got["wp"] = got["wp"].tolist()
            assert got == want, key
    (tmp_path / "wp.json").write_text(g["file_text"][: len(g["file_text"]) // 2])
    assert a._load_from_cache(tmp_path, "cover") is None
    # align(): a cache hit needs neither audio nor features; a miss without feature_fn is None
    (tmp_path / "wp.json").write_text(g["file_text"])
    hit = a.align(tmp_path / "origin.wav", tmp_path / "cover.wav", tmp_path)
    assert hit["pitch_shift"] == -3 and hit["wp"].tolist() == g["saved"][0]["result"]["wp"]
    assert a.align(tmp_path / "origin.wav", tmp_path / "other.wav", tmp_path) is None


def test_filter_and_weakly_align_chains_the_three_functions(cases):
    c = cases["time_map"][0]
    res = {"wp": np.array(c["wp"], dtype=int), "pitch_shift": 0, "num_frames_cover": 1, "num_frames_origin": 1}
    notes = cases["weakly_align"][0]["notes"]
    outs, meta = filter_and_weakly_align([res, None, res], [c["downbeats"]] * 3, [notes] * 3, c["wp_std"] + 1e-9, names=["a", "b", "c"])
    assert outs[1] is None and close(outs[0], weakly_align(copy.deepcopy(notes), copy.deepcopy(c["time_map"])))
    assert [m["dir_name"] for m in meta] == ["a", "c"] and all(m["status"] == "kept" and close(float(m["wp_std"]), c["wp_std"]) for m in meta)
    outs, meta = filter_and_weakly_align([res], [c["downbeats"]], [notes], c["wp_std"] * 0.5)
    assert outs == [None] and meta == []
