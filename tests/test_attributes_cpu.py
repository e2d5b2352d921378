"""Bar attributes without a GPU: the restatement (tests/attributes_np.py) and the host layer of etude_amd.attributes against the reference's own outputs
(tests/golden/attributes_cases.npz, made by make_golden_attributes.py), and the library's refusals.

The pitch-overlap tolerance.  The reference and the restatement both take the mean of the same n_pos ratios in [0, 1], the reference in the order of a Python set, the
restatement ascending.  A sum of n terms in [0, 1] in any order lies within (n - 1) u n of the exact sum, u = 2^-53, so two orders differ by at most 2 (n - 1) n u, and
after the division by n (one more rounding each, of a quotient <= 1) by less than 2 n u.  Below three terms every order gives the same bits."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attributes_np as an  # noqa: E402

from etude_amd import _lib  # noqa: E402
from etude_amd import attributes as at  # noqa: E402

U = 2.0 ** -53
_cache = {}


def gold(golden_dir):
    if "g" not in _cache:
        _cache["g"] = an.load_golden(golden_dir / "attributes_cases.npz")
    return _cache["g"]


def restated(golden_dir):
    if "out" not in _cache:
        gd = gold(golden_dir)
        _cache["out"] = an.Engine(gd["table"]).pairs_many(gd["src_bars"], gd["tgt_bars"], edges=gd["edges"])
        _cache["out"].setflags(write=False)
    return _cache["out"]


def check_against_reference(out, g):
    """the comparisons of the issue, for the restatement and (tests/test_gpu_attributes.py) the device; no case is left out"""
    assert len(out) == len(g["attributes"]) >= 150
    assert np.array_equal(out["features"], g["features"])
    assert out["attributes"][:, :3].tobytes() == g["attributes"][:, :3].tobytes()
    d = np.abs(out["attributes"][:, 3] - g["attributes"][:, 3])
    assert (d <= 2 * g["n_pos"] * U).all(), d.max()
    assert (d[g["n_pos"] < 3] == 0).all()
    assert np.array_equal(out["status"] >> an.NPOS_SHIFT, g["n_pos"]) and not (out["status"] & 255).any()
    assert np.array_equal(out["bins"], g["bins"])


def test_symbols_exported():
    lib = _lib.lib()
    for name in ("etd_attr_limits", "etd_attr_create", "etd_attr_destroy", "etd_attr_check", "etd_attr_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert at.limits() == dict(max_bar_tokens=4096, max_pairs=1 << 20, max_pos_range=4096, max_edges=2)


def test_restatement_against_the_reference(golden_dir):
    g = gold(golden_dir)["g"]
    check_against_reference(restated(golden_dir), g)
    n = g["n_pos"]
    assert (n == 0).any() and (n >= 129).any() and ((n >= 8) & (n <= 128)).any() and set(np.unique(g["bins"])) == {0, 1, 2}


def test_the_special_bars_are_in_the_corpus(golden_dir):
    g = gold(golden_dir)["g"]
    f, a = g["features"], g["attributes"]
    no_pos = (f[:, 1] == 0)
    assert no_pos.any() and (a[no_pos, 0] == 1.0).all() and (a[no_pos, 1] == 1.0).all() and (f[no_pos, 0] == 0).all() and (f[no_pos, 2] > 0).any()
    assert ((f[:, 0] == 0) & (f[:, 1] > 0)).any() and ((f[:, 3] == 0) & (f[:, 4] > 0)).any()


def test_split_into_bars_is_the_datasets(golden_dir):
    gd = gold(golden_dir)
    v = gd["vocab"]
    bos, eos = v.get_bar_bos_id(), v.get_bar_eos_id()
    for s in gd["songs"]:
        assert at.split_into_bars(s["src"], bos, eos) == s["src_bars"] and at.split_into_bars(s["tgt"], bos, eos) == s["tgt_bars"]
    s0 = gd["songs"][0]
    assert s0["tgt"][-1] != eos and s0["tgt_bars"][-1][-1] == eos                       # the unterminated last bar is closed
    assert len(s0["src_bars"]) == len(s0["tgt_bars"]) + 1                               # one bar more on the source side, the empty bar dropped
    assert at.split_into_bars([5, bos, eos, bos, 7, bos, 8, 9], bos, eos) == [[bos, 7, eos], [bos, 8, 9, eos]]
    assert at.split_into_bars([eos, 4], bos, eos) == []


def test_bin_edges_are_the_references(golden_dir, tmp_path):
    gd = gold(golden_dir)
    g = gd["g"]
    e = at.calculate_bin_edges(g["attributes"])
    for n in an.ATTRIBUTES:
        assert e[n].tobytes() == gd["edges"][n].tobytes(), n
    assert all(at.calculate_bin_edges(restated(golden_dir))[n].tobytes() == gd["edges"][n].tobytes() for n in an.ATTRIBUTES)
    for branch in ("one_value", "constant", "spread"):
        e = at.calculate_bin_edges(g[f"branch_{branch}_in"])
        for n in an.ATTRIBUTES:
            assert e[n].tobytes() == g[f"branch_{branch}_{n}"].tobytes(), (branch, n)
    assert g["branch_one_value_relative_polyphony"].tolist() == [-0.5, 0.5]             # fewer than two values
    assert g["branch_constant_relative_polyphony"].tolist() == [1.0 - 1e-3, 1.0 + 1e-3]       # std < 1e-6
    assert g["branch_constant_relative_rhythmic_intensity"].tolist() == [-1e-3, 1e-3]   # ... around a mean below 1e-6
    assert all(len(x) == 0 for x in at.calculate_bin_edges(np.zeros((0, 4))).values())
    at.save_bin_edges(gd["edges"], tmp_path / "bin_edges.json")
    back = at.load_bin_edges(tmp_path / "bin_edges.json")
    assert all(back[n].tobytes() == gd["edges"][n].tobytes() for n in an.ATTRIBUTES)
    assert at.digitize(0.3, []) == 1 and at.digitize(0.3, np.array([0.3, 0.5])) == 1 and at.digitize(0.29, np.array([0.3, 0.5])) == 0


def check_dataset_against_reference(ds, gd):
    """edges, the sample map, the stored chunks and their batch: identical to the reference's"""
    g = gd["g"]
    for n in an.ATTRIBUTES:
        assert ds.attribute_bin_edges[n].tobytes() == gd["edges"][n].tobytes(), n
    assert len(ds) == len(g["sample_map"])
    assert [[e["song_idx"], e["bar_idx"], e["slice"].start, e["slice"].stop] for e in ds.sample_map] == g["sample_map"].tolist()
    keys = ["input_ids", "class_ids", "labels", "polyphony_bin_ids", "rhythm_intensity_bin_ids", "sustain_bin_ids", "pitch_overlap_bin_ids"]
    items = [ds[int(i)] for i in g["chunk_index"]]
    for k, item in enumerate(items):
        assert sorted(item) == sorted(keys)
        for key in keys:
            assert item[key] == g[f"chunk{k}_{key}"].tolist(), (k, key)
    batch = ds.collate_fn(items)
    assert sorted(batch) == sorted(keys + ["attention_mask"])
    for key, val in batch.items():
        assert val.dtype.is_floating_point is False and np.array_equal(val.numpy(), g[f"collate_{key}"]), key


def test_dataset_with_the_restatement_as_engine(golden_dir, tmp_path):
    gd = gold(golden_dir)
    an.write_corpus(gd, tmp_path)
    (tmp_path / "notes").mkdir()
    eng = an.Engine(gd["table"])
    ds = at.EtudeDataset(tmp_path, gd["vocab"], max_seq_len=int(gd["g"]["max_seq_len"]), context_num_past_xy_pairs=int(gd["g"]["n_ctx"]), engine=eng)
    assert eng.calls == 1                                                               # phase 1: the whole corpus in ONE call
    check_dataset_against_reference(ds, gd)
    assert ds.get_attributes_for_model() == list(an.ATTRIBUTES)
    with pytest.raises(IndexError):
        ds[len(ds)]
    first = next(iter(ds.get_dataloader(batch_size=3, shuffle=False)))
    assert first["input_ids"].shape[0] == 3 and first["attention_mask"].sum() == sum(len(ds[i]["input_ids"]) for i in range(3))
    empty = tmp_path / "empty"
    empty.mkdir()
    assert len(at.EtudeDataset(empty, gd["vocab"], max_seq_len=64, engine=eng)) == 0


def _create(table, **cfg):
    lib = _lib.lib()
    c = _lib.AttrCfg(**dict(dict(type_pos=1, type_note=2, type_duration=3), **cfg))
    t = np.ascontiguousarray(table, np.int32)
    h = C.c_void_p()
    rc = lib.etd_attr_create(C.byref(c), C.c_void_p(t.ctypes.data), len(t), C.byref(h))
    return rc, h, (lib.etd_last_error() or b"").decode()


def test_create_refusals():
    lib = _lib.lib()
    ok = [[0, 1], [0, 0], [1, 0], [1, 4095], [2, 60], [3, 4]]
    rc, h, _ = _create(ok)
    assert rc == 0
    lib.etd_attr_destroy(h)
    rc, _, msg = _create(ok + [[1, 4096]])
    assert rc == -22 and "Pos values span 0 .. 4096, 4097 values (> 4096" in msg
    rc, _, msg = _create([[1, -5], [1, 4091]])
    assert rc == -22 and "span -5 .. 4091" in msg
    rc, _, msg = _create(ok + [[3, 1 << 20]])
    assert rc == -22 and "Duration value of 1048576" in msg
    rc, _, msg = _create(ok, type_note=1)
    assert rc == -22 and "three different codes" in msg
    c = _lib.AttrCfg(type_pos=1, type_note=2, type_duration=3)
    c.struct_bytes = 8
    t = np.asarray(ok, np.int32)
    h = C.c_void_p()
    assert lib.etd_attr_create(C.byref(c), C.c_void_p(t.ctypes.data), len(t), C.byref(h)) == -22 and b"bytes here" in lib.etd_last_error()
    assert lib.etd_attr_create(C.byref(_lib.AttrCfg(type_pos=1, type_note=2, type_duration=3)), None, 4, C.byref(h)) == -22
    rc, _, msg = _create(np.zeros((0, 2)))
    assert rc == -22 and "vocab_size = 0" in msg


def test_check_refusals_and_the_token_limit(golden_dir):
    eng = at.BarAttributes(gold(golden_dir)["vocab"])                                   # constructing needs no GPU
    lim = eng.limits["max_bar_tokens"]
    eng.check_offsets(np.array([0, 3, 3, 3 + lim]))                                     # an empty bar and one at the limit pass
    with pytest.raises(_lib.EtudeHipError, match=rf"bar 1 has {lim + 1} tokens \(> {lim}"):
        eng.check_offsets(np.array([0, 3, 4 + lim]))
    with pytest.raises(_lib.EtudeHipError, match=r"offsets_host\[0\] = 2 \(need 0\)"):
        eng.check_offsets(np.array([2, 3]))
    with pytest.raises(_lib.EtudeHipError, match="offsets_host decreases at bar 1"):
        eng.check_offsets(np.array([0, 5, 4]))
    with pytest.raises(_lib.EtudeHipError, match=r"0 bars in one call \(need 1 .. 1048576\)"):
        eng.check_offsets(np.array([0]))
    lib = _lib.lib()
    assert lib.etd_attr_check(eng.h, None, 1) == -22 and lib.etd_attr_check(None, None, 1) == -22
    assert lib.etd_attr_run(*([None] * 3), None, 0, None, None, None, None, 0, None, 0, *([None] * 7)) == -22 and b"attr_run: null argument" in lib.etd_last_error()


def test_inputs_of_the_host_layer():
    ids, off = at.pack_bars([[1, 2, 3], [], [4]])
    assert ids.tolist() == [1, 2, 3, 4] and off.tolist() == [0, 3, 3, 4] and ids.dtype == np.int32 and off.dtype == np.int64
    ids2, off2 = at.pack_bars((np.array([1, 2, 3, 4], np.int32), np.array([3, 0, 1])))
    assert ids2.tolist() == ids.tolist() and off2.tolist() == off.tolist()
    with pytest.raises(ValueError):
        at.pack_bars((np.array([1, 2], np.int32), np.array([3])))
    from etude_amd.decoder import PackedBars
    ids3, off3 = at.pack_bars(PackedBars.from_lists([[1, 2, 3], [], [4]]))
    assert ids3.tolist() == ids.tolist() and off3.tolist() == off.tolist() and off3.dtype == np.int64
    e, n = at.edges_arrays({"relative_polyphony": [0.5, 1.5], "pitch_overlap_ratio": [0.25]})
    assert e.tolist() == [[0.5, 1.5], [0, 0], [0, 0], [0.25, 0]] and n.tolist() == [2, 0, 0, 1]
    with pytest.raises(ValueError):
        at.edges_arrays([[1, 2, 3], [], [], []])
    rq = at.requested_bins([dict(polyphony_bin=0, rhythm_intensity_bin=1, sustain_bin=2, pitch_overlap_bin=1)])
    assert rq.tolist() == [[0, 1, 2, 1]] and at.requested_bins(np.array([[1, 0, 2, 1]], np.int32)).tolist() == [[0, 1, 2, 1]]      # the ABI order: overlap, polyphony, sustain, rhythm
    import etude_amd
    assert etude_amd.BarAttributes is at.BarAttributes and etude_amd.attribute_adherence is at.attribute_adherence


def test_adherence_through_the_restatement(golden_dir):
    gd = gold(golden_dir)
    src, tgt = gd["src_bars"][20:25], gd["tgt_bars"][20:25]
    grid = [dict(polyphony_bin=p, rhythm_intensity_bin=1, sustain_bin=2 - p, pitch_overlap_bin=2) for p in range(3)]
    jobs = [(src, [a] * 5) for a in grid]
    results = [tgt, tgt[:3], gd["tgt_bars"][30:35]]
    r = at.attribute_adherence(jobs, results, gd["vocab"], gd["edges"], engine=an.Engine(gd["table"]))
    assert [len(j["realised"]) for j in r["per_job"]] == [5, 3, 5] and r["n_bars"] == 13 and r["counts"].sum() == 4 * 13
    assert np.array_equal(r["per_job"][0]["realised"], gd["g"]["bins"][20:25]) and np.array_equal(r["per_job"][1]["realised"], gd["g"]["bins"][20:23])
    rq, rl = np.concatenate([j["requested"] for j in r["per_job"]]), np.concatenate([j["realised"] for j in r["per_job"]])
    assert np.array_equal(r["counts"], an.adherence_counts(rq, rl))
    assert np.allclose(r["hit_rate"], (rq == rl).mean(axis=0), rtol=0, atol=1e-15)
