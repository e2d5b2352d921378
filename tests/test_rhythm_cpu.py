"""The rhythm metrics without a GPU: the fp64 restatement of DESIGN.md 4h (tests/rhythm_np.py) against the reference's RGCCalculator / IPECalculator on the golden
covers (tests/golden/rhythm_cases.npz, written by make_golden_rhythm.py from the reference and scikit-learn 1.7.2), numpy's summation order read off numpy itself,
the MIDI reader against the project's own writer, the error strings and what the C ABI refuses before it touches a device.

RGC: score, tau and the error exit bitwise.  IPE: the same error exit; on every cover the restatement does NOT flag `relocated`, scikit-learn's partition and an equal
score.  On flagged covers (an empty cluster was relocated: scikit-learn's argpartition leaves the order of equally far samples open, 4h takes distance descending, then
lowest index) parity is reported, not asserted."""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rhythm_np as rn  # noqa: E402

_cache = {}


def cases(golden_dir):
    if "g" not in _cache:
        _cache["g"], _cache["limit"] = rn.load_cases(golden_dir / "rhythm_cases.npz")
    return _cache["g"]


def restated(golden_dir):
    """the restatement on every golden cover, computed once"""
    if "r" not in _cache:
        _cache["r"] = [(rn.rgc(c["onsets"]), rn.ipe(c["onsets"])) for c in cases(golden_dir)]
    return _cache["r"]


def test_np_sum_is_numpys_order():
    rng = np.random.default_rng(0)
    for n in list(range(1, 40)) + [127, 128, 129, 130, 255, 256, 257, 600, 1499, 8191]:
        x = rng.standard_normal(n) * rng.uniform(0.1, 10.0)
        assert rn.np_sum(x) == np.sum(x) == x.reshape(-1, 1).sum(axis=0)[0], n
        assert rn.np_sum(x) / float(n) == np.mean(x), n
    x = rng.uniform(0.0, 0.5, 8)
    assert np.mean(x) == (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) / 8.0      # exactly 8: the eight-accumulator form


def test_random_table_is_what_kmeans_draws():
    rs = np.random.RandomState(42)
    t = rn.random_table()
    assert t.shape == (29,) and t[0] == rs.random_sample() and np.array_equal(t[1:5], rs.uniform(size=4))
    assert abs(t[0] - 0.3745401188473625) < 1e-16


def test_rgc_bitwise_against_the_reference(golden_dir):
    seen = set()
    for c, (r, _) in zip(cases(golden_dir), restated(golden_dir)):
        st, score, tau = r
        assert rn.RGC_ERRORS.get(st, "") == c["rgc_error"], c["name"]
        seen.add(st)
        if st == rn.RGC_OK:
            assert score == c["rgc_score"] and tau == c["rgc_tau"], (c["name"], score, c["rgc_score"], tau, c["rgc_tau"])
    assert {rn.RGC_OK, rn.RGC_FEW_ONSETS, rn.RGC_FEW_IOIS, rn.RGC_FEW_UNIQUE} <= seen


def test_rgc_no_valid_tau_and_ties():
    t = np.cumsum(np.tile([0.002, 0.003, 0.004], 6))
    assert rn.rgc(t)[0] == rn.RGC_NO_TAU
    # ties by first occurrence: 0.5 and 0.25 both twice, 0.5 first -> the candidates start with 0.5
    t = np.cumsum([0.5, 0.25, 0.5, 0.25, 0.125, 1.0, 2.0, 0.75, 1.5])
    st, score, tau = rn.rgc(t, top_k=8)
    assert st == rn.RGC_OK and tau == 0.125 and score == 0.0


def test_ipe_partition_against_scikit_learn(golden_dir):
    n_flag = n_ok = n_flag_same = 0
    for c, (_, p) in zip(cases(golden_dir), restated(golden_dir)):
        assert rn.IPE_ERRORS.get(p["status"], "") == c["ipe_error"], c["name"]
        if p["status"] != rn.IPE_OK:
            continue
        same = rn.same_partition(p["labels"], c["labels"]) and p["score"] == c["ipe_score"]
        if p["relocated"]:
            n_flag += 1
            n_flag_same += same
            assert len(c["onsets"]) <= 40, c["name"]
            continue
        n_ok += 1
        assert rn.same_partition(p["labels"], c["labels"]), c["name"]
        assert p["score"] == c["ipe_score"], (c["name"], p["score"], c["ipe_score"])
    print(f"IPE: {n_ok} unflagged covers with scikit-learn's partition and score; flagged (relocated): {n_flag_same} of {n_flag} match")
    assert 4 * n_ok >= 3 * (n_ok + n_flag) and n_ok >= 24


def test_goldens_cover_the_lengths(golden_dir):
    cs = cases(golden_dir)
    limit = _cache["limit"]
    lens = {len(c["onsets"]) for c in cs}
    assert {0, 2, 8, 9, 10, 12, 40, 255, 256, 257, 600, 1500, limit, limit + 1} <= lens
    by = {c["name"]: c for c in cs}
    assert by["single_ioi"]["rgc_error"] == rn.RGC_ERRORS[rn.RGC_FEW_UNIQUE] and by["single_ioi"]["ipe_error"] == rn.IPE_ERRORS[rn.IPE_NO_SYMBOLS]
    assert float(np.diff(by["all_below_min"]["onsets"]).max()) < 0.0625 and by["all_below_min"]["ipe_error"] == rn.IPE_ERRORS[rn.IPE_NO_SYMBOLS]


def test_error_strings_match_the_restatement():
    from etude_amd import rhythm
    assert rhythm.RGC_ERRORS == rn.RGC_ERRORS and rhythm.IPE_ERRORS == rn.IPE_ERRORS


def test_midi_reader_round_trips_the_writer(tmp_path):
    from etude_amd import rhythm
    from etude_amd.tokenizer import TinyREMITokenizer
    rng = np.random.default_rng(5)
    on = np.sort(rng.uniform(0.0, 90.0, 200))
    notes = [{"pitch": int(rng.integers(21, 109)), "onset": float(t), "offset": float(t + rng.uniform(0.05, 1.0)), "velocity": int(rng.integers(1, 128))} for t in on]
    TinyREMITokenizer.note_to_midi(notes, tmp_path / "a.mid")
    got = rhythm.read_midi_onsets(tmp_path / "a.mid")
    tick = 60.0 / (120.0 * 220)
    assert got.shape == on.shape and np.abs(np.sort(got) - on).max() <= tick
    u = rhythm.get_onsets_from_file(tmp_path / "a.mid")
    assert np.array_equal(u, np.unique(got))
    (tmp_path / "a.json").write_text(json.dumps(notes))
    assert np.array_equal(rhythm.get_onsets_from_file(tmp_path / "a.json"), np.unique(on))
    assert rhythm.get_onsets_from_file(tmp_path / "missing.mid").size == 0
    (tmp_path / "bad.mid").write_bytes(b"not a midi file")
    assert rhythm.get_onsets_from_file(tmp_path / "bad.mid").size == 0
    (tmp_path / "one.json").write_text(json.dumps(notes[:1]))
    assert rhythm.get_onsets_from_file(tmp_path / "one.json").size == 0


def test_midi_reader_tempo_map_drums_and_running_status(tmp_path):
    from etude_amd import rhythm
    # format 1, 480 ticks per beat: tempo 500 000 at tick 0, 250 000 at tick 960; note-ons at ticks 0, 480 (running status), 960, 1440; a drum note (channel 10) and a
    # note-on with velocity 0 are not onsets
    trk0 = bytes([0x00, 0xFF, 0x51, 0x03, 0x07, 0xA1, 0x20, 0x87, 0x40, 0xFF, 0x51, 0x03, 0x03, 0xD0, 0x90, 0x00, 0xFF, 0x2F, 0x00])
    trk1 = bytes([0x00, 0x90, 60, 64, 0x83, 0x60, 62, 64, 0x00, 0x99, 36, 100, 0x00, 0x90, 60, 0, 0x83, 0x60, 0x90, 64, 64, 0x83, 0x60, 65, 64, 0x00, 0xFF, 0x2F, 0x00])
    data = b"MThd" + (6).to_bytes(4, "big") + (1).to_bytes(2, "big") + (2).to_bytes(2, "big") + (480).to_bytes(2, "big")
    for t in (trk0, trk1):
        data += b"MTrk" + len(t).to_bytes(4, "big") + t
    (tmp_path / "t.mid").write_bytes(data)
    got = rhythm.read_midi_onsets(tmp_path / "t.mid")
    assert np.allclose(got, [0.0, 0.5, 1.0, 1.25], rtol=0, atol=1e-12)


def test_c_abi_refuses_on_the_host():
    from etude_amd import _lib, rhythm
    lib = _lib.lib()
    lim = rhythm.limits()
    assert lim["max_onsets"] >= 8192
    rnd = np.ascontiguousarray(rn.random_table())

    def cfg(**kw):
        p = dict(top_k=8, precision_digits=4, n_gram=8, n_clusters=8, min_ioi=0.0625, max_ioi=4.0)
        p.update(kw)
        return _lib.RhythmCfg(n_random=29, random_host=rnd.ctypes.data_as(C.POINTER(C.c_double)), **p)

    h = C.c_void_p()
    for bad in (dict(top_k=0), dict(top_k=lim["max_top_k"] + 1), dict(precision_digits=10), dict(n_gram=0), dict(n_gram=lim["max_n_gram"] + 1), dict(n_clusters=9),
                dict(min_ioi=0.0), dict(max_ioi=0.01)):
        c = cfg(**bad)
        assert lib.etd_rhythm_create(C.byref(c), C.byref(h)) == -22, bad
    c = cfg()
    c.struct_bytes += 8
    assert lib.etd_rhythm_create(C.byref(c), C.byref(h)) == -22
    c = cfg()
    c.n_random = 28
    assert lib.etd_rhythm_create(C.byref(c), C.byref(h)) == -22
    eng = rhythm.RhythmMetrics()
    eng.check_offsets(np.array([0, lim["max_onsets"], lim["max_onsets"] + 5]))
    with pytest.raises(_lib.EtudeHipError, match=r"cover 1 has 8193 onsets \(> 8192"):
        eng.check_offsets(np.array([0, 3, 3 + lim["max_onsets"] + 1]))
    with pytest.raises(_lib.EtudeHipError, match="decreases at cover 0"):
        eng.check_offsets(np.array([0, -1]))
    with pytest.raises(_lib.EtudeHipError, match=r"offsets_host\[0\]"):
        eng.check_offsets(np.array([1, 2]))
    # the run itself refuses the same before it touches a device (no GPU is opened by these calls), and null outputs
    off = np.array([0, lim["max_onsets"] + 1], np.int64)
    fake = C.c_void_p(256)
    assert lib.etd_rhythm_run(eng.h, fake, fake, off.ctypes.data_as(_lib.c_i64_p), 1, fake, fake, None) == -22
    assert b"8193 onsets" in lib.etd_last_error()
    off = np.array([0, 4], np.int64)
    assert lib.etd_rhythm_run(eng.h, fake, fake, off.ctypes.data_as(_lib.c_i64_p), 1, None, fake, None) == -22
    assert lib.etd_rhythm_debug_logioi(eng.h, fake, None, None) == -22
    with pytest.raises(ValueError, match="non-finite"):
        eng.pack([[0.0, float("nan")]])
    with pytest.raises(ValueError, match="too long"):
        eng.pack([[0.0, 1e12]])
    packed, offsets = eng.pack([[0.5, 0.1, 0.1, 0.3], [], [2.0]])
    assert offsets.tolist() == [0, 3, 3, 4] and packed[:4].tolist() == [0, 3, 3, 4] and packed[4:].view(np.float64).tolist() == [0.1, 0.3, 0.5, 2.0]
