"""Rhythm metrics on the MI355X (csrc/rhythm.hip, etude_amd.RhythmMetrics) against the fp64 restatement of DESIGN.md 4h (tests/rhythm_np.py) and against the
reference's own outputs (tests/golden/rhythm_cases.npz); error exits, batch invariance, run-to-run identity, the refusal past the limit and the note-list surface.

RGC: bitwise.  IPE: the restatement is fed the centred log-IOIs the device clustered (the tap of etd_rhythm_debug_logioi: the device's logarithm may differ from
numpy's by an ulp); the labels must be identical and the centres within 1e-12 relative.

The entropy's tolerance.  H = -sum of n_terms <= n_ngrams products p log2 p, each in [-0.5308, 0] with sum |p log2 p| = H.  The device adds the terms in another order
than the restatement: two orders of a sum of n terms differ by at most (n - 1) u sum|terms| each from the exact sum, u = 2^-53, so by 2 (n - 1) u H from one another;
an ulp of log2 in each term (both sides) adds 2 u sum|terms| = 2 u H, the rounding of each product and quotient less than that again.  4 n_ngrams u max(1, H) covers
the sum of these for every n_ngrams >= 1."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rhythm_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
_cache = {}


def cases(golden_dir):
    if "cases" not in _cache:
        _cache["cases"] = rn.load_cases(golden_dir / "rhythm_cases.npz")[0]
    return _cache["cases"]


def _eng():
    from etude_amd.rhythm import RhythmMetrics
    if "eng" not in _cache:
        _cache["eng"] = RhythmMetrics()
    return _cache["eng"]


def _golden_run(golden_dir):
    """every golden cover the engine accepts, in ONE tapped call: (cases, out, status, offsets, tap), computed once"""
    if "run" not in _cache:
        cs = [c for c in cases(golden_dir) if len(c["onsets"]) <= _eng().limits["max_onsets"]]
        for c in cs:
            c["onsets"].setflags(write=False)
        eng = _eng()
        eng.tap(True)
        out, status, offsets = eng.raw_many([c["onsets"] for c in cs])
        tap = eng.last_tap
        eng.tap(False)
        _cache["run"] = (cs, out, status, offsets, tap)
    return _cache["run"]


def _tol(n_onsets, H, n_gram=8):
    return 4 * max(1, n_onsets - 1 - n_gram + 1) * U * max(1.0, H)


def _check_against_restatement(onsets, out, st, xc, lab, centres, name):
    rgc_st, score, tau = rn.rgc(onsets)
    assert (st & 15) == rgc_st, name
    if rgc_st == rn.RGC_OK:
        assert out[0] == score and out[1] == tau, (name, out[:2], score, tau)
    else:
        assert np.isnan(out[0]) and np.isnan(out[1])
    if len(onsets) < 2:
        assert ((st >> 4) & 15) == rn.IPE_FEW_ONSETS and np.isnan(out[2])
        return None
    m = len(onsets) - 1
    x_np, _ = rn.log_ioi(onsets)
    n_unique = len(np.unique(np.log(np.clip(np.diff(onsets), 0.0625, 4.0))))
    if min(8, n_unique) < 2:
        assert ((st >> 4) & 15) == rn.IPE_NO_SYMBOLS and np.isnan(out[2]), name
        return None
    assert ((st >> 4) & 15) == rn.IPE_OK, name
    assert np.abs(xc - x_np).max() <= 8 * U * max(1.0, np.abs(x_np).max()), name      # the device's log and mean against numpy's: a few ulps
    var = rn.np_sum([float(v) * float(v) for v in xc]) / float(m)
    p = rn.ipe_from_logioi(xc, var, n_unique)
    assert np.array_equal(lab, p["labels"]), name
    assert ((st >> 12) & 15) == p["k"] and bool((st >> 8) & 1) == p["relocated"] and ((st >> 16) & 511) == p["iterations"], (name, hex(st), p["k"], p["relocated"], p["iterations"])
    assert np.abs(centres[:p["k"]] - p["centres"]).max() <= 1e-12 * np.abs(p["centres"]).max(), name
    assert np.isnan(centres[p["k"]:]).all()
    assert abs(out[2] - p["score"]) <= _tol(len(onsets), p["score"]), (name, out[2], p["score"])
    return p


def test_device_against_the_restatement_on_every_golden(golden_dir):
    cs, out, status, offsets, tap = _golden_run(golden_dir)
    n_ipe = 0
    for b, c in enumerate(cs):
        m = max(len(c["onsets"]) - 1, 0)
        o = int(offsets[b])
        p = _check_against_restatement(c["onsets"], out[b], int(status[b]), tap["logioi"][o:o + m], tap["labels"][o:o + m], tap["centres"][b], c["name"])
        n_ipe += p is not None
    assert n_ipe >= 28


def test_device_against_the_reference_goldens(golden_dir):
    from etude_amd import rhythm
    cs, out, status, offsets, tap = _golden_run(golden_dir)
    n_ok = n_flag = n_flag_same = 0
    for b, c in enumerate(cs):
        st = int(status[b])
        assert rhythm.RGC_ERRORS.get(st & 15, "") == c["rgc_error"], c["name"]
        if not c["rgc_error"]:
            assert out[b, 0] == c["rgc_score"] and out[b, 1] == c["rgc_tau"], c["name"]
        assert rhythm.IPE_ERRORS.get((st >> 4) & 15, "") == c["ipe_error"], c["name"]
        if c["ipe_error"]:
            continue
        m, o = len(c["onsets"]) - 1, int(offsets[b])
        same = rn.same_partition(tap["labels"][o:o + m], c["labels"]) and abs(out[b, 2] - c["ipe_score"]) <= _tol(len(c["onsets"]), c["ipe_score"])
        if (st >> 8) & 1:
            n_flag += 1
            n_flag_same += bool(same)
            assert len(c["onsets"]) <= 40, c["name"]
            continue
        n_ok += 1
        assert same, (c["name"], out[b, 2], c["ipe_score"])
    print(f"device vs scikit-learn: {n_ok} unflagged covers identical; flagged (relocated): {n_flag_same} of {n_flag} match")
    assert 4 * n_ok >= 3 * (n_ok + n_flag) and n_ok >= 24


def _exits():
    rng = np.random.default_rng(11)
    grid = np.cumsum(rng.choice([1, 2, 3, 4, 6, 8], size=120)) * 0.125
    return [("valid", grid), ("empty", np.zeros(0)), ("one", np.array([1.0])), ("few_iois", np.array([0.0, 0.5, 1.0, 1.75, 2.0])), ("single_ioi", np.arange(20) * 0.25),
            ("no_tau", np.cumsum(np.tile([0.002, 0.003, 0.004], 6))), ("below_min", np.cumsum(rng.choice([0.02, 0.03, 0.05], size=30))),
            ("valid2", np.cumsum(rng.choice([1, 2, 3, 4, 6, 8, 16], size=257)) * 0.11 + rng.normal(0, 0.01, 257)), ("two", np.array([0.0, 0.5]))]


def test_ragged_batch_mixing_every_error_exit():
    from etude_amd import rhythm
    eng = _eng()
    covers = _exits()
    rows = eng.metrics_many([c for _, c in covers], details=True)
    want_rgc = {"empty": 1, "one": 1, "few_iois": 2, "single_ioi": 3, "no_tau": 4, "below_min": 0, "two": 2}
    want_ipe = {"empty": 1, "one": 1, "single_ioi": 3, "no_tau": 3, "below_min": 3, "two": 3}
    seen = set()
    for (name, c), row in zip(covers, rows):
        u = np.unique(c)
        st, score, tau = rn.rgc(u)
        assert st == want_rgc.get(name, 0), name
        seen.add(st)
        if st:
            assert row["rgc_error"] == rhythm.RGC_ERRORS[st] and "rgc_score" not in row and "inferred_tau" not in row, name
        else:
            assert row["rgc_score"] == score and row["inferred_tau"] == tau and "rgc_error" not in row, name
        p = rn.ipe(u)
        assert p["status"] == want_ipe.get(name, 0), name
        if p["status"]:
            assert row["ipe_error"] == rhythm.IPE_ERRORS[p["status"]] and "ipe_score" not in row, name
        else:
            assert "ipe_error" not in row and np.isfinite(row["ipe_score"]) and row["n_clusters"] == p["k"], name
    assert seen == {0, 1, 2, 3, 4}


def test_alone_and_in_batches_of_2_27_300_and_twice(golden_dir):
    cs = [c for c in cases(golden_dir) if 2 <= len(c["onsets"]) <= 600]
    pool = [c["onsets"] for c in cs] + [c for _, c in _exits()]
    eng = _eng()
    alone = [eng.raw_many([x])[:2] for x in pool]
    for size in (2, 27, 300):
        order = [(7 * i + 3) % len(pool) for i in range(size)]
        out, status, _ = eng.raw_many([pool[j] for j in order])
        out2, status2, _ = eng.raw_many([pool[j] for j in order])
        assert out.tobytes() == out2.tobytes() and status.tobytes() == status2.tobytes(), size      # two consecutive runs
        for i, j in enumerate(order):
            assert out[i].tobytes() == alone[j][0][0].tobytes() and status[i] == alone[j][1][0], (size, i, j)


def test_at_the_limit_and_refusal_beyond_it(golden_dir):
    from etude_amd import _lib
    eng = _eng()
    by = {c["name"]: c for c in cases(golden_dir)}
    lim = eng.limits["max_onsets"]
    assert len(by["at_limit"]["onsets"]) == lim and len(by["past_limit"]["onsets"]) == lim + 1
    small = by["n12_exact"]["onsets"]
    rows = eng.metrics_many([small, by["at_limit"]["onsets"]])
    assert rows[1]["rgc_score"] == by["at_limit"]["rgc_score"] and rows[0]["rgc_score"] == by["n12_exact"]["rgc_score"]
    with pytest.raises(_lib.EtudeHipError, match=r"cover 1 has 8193 onsets \(> 8192"):
        eng.metrics_many([small, by["past_limit"]["onsets"]])
    assert eng.metrics_many([small]) == [rows[0]]      # the engine goes on after a refusal


def test_metrics_for_decoded_notes_equal_the_calculators_on_json(golden_dir, tmp_path):
    from etude_amd import rhythm, synth
    from etude_amd.tokenizer import TinyREMITokenizer
    from etude_amd.vocab import Vocab
    v = Vocab()
    v.token_to_id = synth.vocab_json()["token_to_id"]
    v.id_to_token = [""] * len(v.token_to_id)
    for t, i in v.token_to_id.items():
        v.id_to_token[i] = t
    tempo = [{"start": 0.5, "bpm": 120, "time_sig": 4, "downbeats": [round(0.5 + 2.0 * i, 6) for i in range(90)]}]
    (tmp_path / "tempo.json").write_text(json.dumps(tempo))
    tk = TinyREMITokenizer(str(tmp_path / "tempo.json"))
    notes = tk.decode_to_notes(v.decode_sequence_to_events(np.load(golden_dir / "clip_ctx.npz")["gen_ids"].tolist()))
    assert len(notes) > 100
    lists = [notes, notes[:len(notes) // 2], notes[len(notes) // 3:], notes[:5], []]
    rows = rhythm.rhythm_metrics_for_notes(lists)
    rgc, ipe = rhythm.RGCCalculator(), rhythm.IPECalculator()
    n_scores = 0
    for i, (lst, row) in enumerate(zip(lists, rows)):
        f = tmp_path / f"cover{i}.json"
        f.write_text(json.dumps(lst))
        r, p = rgc.calculate(f), ipe.calculate(f)
        assert r == ({"error": row["rgc_error"]} if "rgc_error" in row else {"rgc_score": row["rgc_score"], "inferred_tau": row["inferred_tau"]}), i
        assert p == ({"error": row["ipe_error"]} if "ipe_error" in row else {"ipe_score": row["ipe_score"]}), i
        n_scores += "rgc_score" in row and "ipe_score" in row
    assert n_scores >= 3 and "rgc_error" in rows[-1] and "ipe_error" in rows[-1]
