"""Bar attributes on the MI355X (csrc/attributes.hip, etude_amd.BarAttributes) against the restatement of DESIGN.md 4i (tests/attributes_np.py), bit for bit on the six
counts, the four attributes, the bins and the status word, and against the reference's own outputs (tests/golden/attributes_cases.npz); the chunk edges of the scan,
the edges of the sum order, the carry, batch invariance, run-to-run identity, ids outside the vocabulary, adherence and the dataset through the device."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import attributes_np as an  # noqa: E402
from test_attributes_cpu import check_against_reference, check_dataset_against_reference, gold  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}
BAR_LENGTHS = (3, 63, 64, 65, 127, 128, 129, 4096)
POSITION_COUNTS = (1, 7, 8, 9, 128, 129, 192)


def _eng(golden_dir):
    from etude_amd.attributes import BarAttributes
    if "eng" not in _cache:
        _cache["eng"] = BarAttributes(gold(golden_dir)["vocab"])
    return _cache["eng"]


def _same(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("features", "attributes", "bins", "status"))


def _ids(gd):
    v = gd["vocab"]
    t = gd["table"]
    return dict(bos=v.get_bar_bos_id(), eos=v.get_bar_eos_id(), pos={int(val): i for i, (ty, val) in enumerate(t.tolist()) if ty == an.TYPE_POS},
                note=[i for i, (ty, _) in enumerate(t.tolist()) if ty == an.TYPE_NOTE], dur=[i for i, (ty, _) in enumerate(t.tolist()) if ty == an.TYPE_DURATION],
                other=[i for i, (ty, _) in enumerate(t.tolist()) if ty not in (0, an.TYPE_POS, an.TYPE_NOTE, an.TYPE_DURATION)])


def _random_bar(rng, k, n_tokens):
    """n_tokens tokens in all: any order of Pos, Note, Duration and ignored tokens (notes before the first Pos, repeated Pos values, positions without notes)"""
    kinds = rng.choice(4, size=n_tokens - 2, p=[0.2, 0.4, 0.35, 0.05])
    pos = list(k["pos"].values())
    body = [int(rng.choice(pos)) if q == 0 else int(rng.choice(k["note"])) if q == 1 else int(rng.choice(k["dur"])) if q == 2 else int(rng.choice(k["other"])) for q in kinds]
    return [k["bos"]] + body + [k["eos"]]


def _bar_with_positions(rng, k, positions):
    body = []
    for p in positions:
        body.append(k["pos"][int(p)])
        for _ in range(int(rng.integers(1, 4))):
            body += [int(rng.choice(k["note"])), int(rng.choice(k["dur"]))]
    return [k["bos"]] + body + [k["eos"]]


def _pool(golden_dir):
    """(source bars, target bars, what each pair is there for): 257 pairs of mixed lengths, made once with their restatement"""
    if "pool" not in _cache:
        gd = gold(golden_dir)
        k, rng = _ids(gd), np.random.default_rng(4)
        src, tgt, why = [], [], []
        for n in BAR_LENGTHS:                                                          # the chunk edges of the scan, on either side
            src.append(_random_bar(rng, k, n)); tgt.append(_random_bar(rng, k, int(rng.integers(3, 200)))); why.append(f"src{n}")
            src.append(_random_bar(rng, k, int(rng.integers(3, 200)))); tgt.append(_random_bar(rng, k, n)); why.append(f"tgt{n}")
        for n in POSITION_COUNTS:                                                      # the edges of the sum order: n positions in the union
            ps = np.sort(rng.choice(192, size=n, replace=False))
            src.append(_bar_with_positions(rng, k, ps)); tgt.append(_bar_with_positions(rng, k, np.sort(rng.choice(ps, size=max(1, n - 2), replace=False)))); why.append(f"npos{n}")
        for at_token in (63, 127):                                                     # a Pos as the last token of a chunk, its notes in the next: the carry
            bar = [k["bos"]] + [int(rng.choice(k["dur"])) for _ in range(at_token - 1)] + [k["pos"][5]] + [int(rng.choice(k["note"])) for _ in range(70)] + [k["eos"]]
            assert an.TYPE_POS == gd["table"][bar[at_token]][0] and len(bar) > at_token + 65
            src.append(bar); tgt.append(bar[:at_token] + [k["pos"][7]] + bar[at_token + 1:]); why.append(f"carry{at_token}")
            src.append(_random_bar(rng, k, 40)); tgt.append(bar); why.append(f"carry{at_token}_tgt")
        src.append([k["bos"], k["eos"]]); tgt.append([]); why.append("empty")
        while len(src) < 257:
            src.append(_random_bar(rng, k, int(rng.integers(3, 300)))); tgt.append(_random_bar(rng, k, int(rng.integers(3, 300)))); why.append("random")
        want = an.Engine(gd["table"]).pairs_many(src, tgt, edges=gd["edges"])
        want.setflags(write=False)
        _cache["pool"] = (src, tgt, why, want)
    return _cache["pool"]


def _pool_run(golden_dir):
    if "pool_run" not in _cache:
        src, tgt, _, _ = _pool(golden_dir)
        _cache["pool_run"] = _eng(golden_dir).pairs_many(src, tgt, edges=gold(golden_dir)["edges"])
        _cache["pool_run"].setflags(write=False)
    return _cache["pool_run"]


def _golden_run(golden_dir):
    if "golden_run" not in _cache:
        gd = gold(golden_dir)
        _cache["golden_run"] = _eng(golden_dir).pairs_many(gd["src_bars"], gd["tgt_bars"], edges=gd["edges"])
    return _cache["golden_run"]


def test_golden_corpus_against_the_restatement_and_the_reference(golden_dir):
    gd = gold(golden_dir)
    out = _golden_run(golden_dir)
    want = an.Engine(gd["table"]).pairs_many(gd["src_bars"], gd["tgt_bars"], edges=gd["edges"])
    for f in ("features", "attributes", "bins", "status"):
        assert out[f].tobytes() == want[f].tobytes(), f
    check_against_reference(out, gd["g"])
    raw = _eng(golden_dir).pairs_many(gd["src_bars"], gd["tgt_bars"])                   # without edges: raw values only
    assert raw["attributes"].tobytes() == out["attributes"].tobytes() and (raw["bins"] == -1).all()


def test_chunk_edges_sum_order_edges_and_the_carry(golden_dir):
    src, tgt, why, want = _pool(golden_dir)
    out = _pool_run(golden_dir)
    assert len(out) == 257
    for i, name in enumerate(why):
        for f in ("features", "attributes", "bins", "status"):
            assert out[f][i].tobytes() == want[f][i].tobytes(), (name, f, out[f][i], want[f][i])
    n_pos = dict(zip(why, (want["status"] >> an.NPOS_SHIFT).tolist()))
    assert [n_pos[f"npos{n}"] for n in POSITION_COUNTS] == list(POSITION_COUNTS)
    assert {len(b) for b in src} >= set(BAR_LENGTHS) and {len(b) for b in tgt} >= set(BAR_LENGTHS)
    for at_token in (63, 127):
        i = why.index(f"carry{at_token}")
        assert want["features"][i].tolist()[0] == 70 and want["features"][i].tolist()[3] == 70 and want["attributes"][i][3] == 0.0      # 70 notes at Pos 5 / at Pos 7: none shared
    assert want["features"][why.index("empty")].tolist() == [0] * 6 and want["attributes"][why.index("empty")].tolist() == [1.0, 1.0, 1.0, 0.0]


def test_alone_in_the_batch_and_twice(golden_dir):
    src, tgt, why, _ = _pool(golden_dir)
    eng, edges = _eng(golden_dir), gold(golden_dir)["edges"]
    out = _pool_run(golden_dir)
    again = eng.pairs_many(src, tgt, edges=edges)
    assert _same(out, again)                                                            # a second run
    for i in range(len(src)):                                                           # every pair of the P = 257 call against its own P = 1 call
        one = eng.pairs_many([src[i]], [tgt[i]], edges=edges)
        assert len(one) == 1 and _same(one, out[i:i + 1]), (i, why[i])
    order = [(7 * i + 3) % len(src) for i in range(31)]
    mixed = eng.pairs_many([src[j] for j in order], [tgt[j] for j in order], edges=edges)
    assert _same(mixed, out[order])                                                     # other neighbours in the workgroup


def test_input_forms_indices_and_features(golden_dir):
    from etude_amd.decoder import PackedBars
    src, tgt, _, _ = _pool(golden_dir)
    eng, edges = _eng(golden_dir), gold(golden_dir)["edges"]
    out = _pool_run(golden_dir)[:40]
    s, t = src[:40], tgt[:40]
    flat = lambda bars: (np.asarray([x for b in bars for x in b], np.int32), np.asarray([len(b) for b in bars], np.int64))      # noqa: E731
    assert _same(eng.pairs_many(PackedBars.from_lists(s), flat(t), edges=edges), out)
    # pair i = (source bar i % 5, target bar 39 - i) through the indices: five source bars uploaded once
    si, ti = np.arange(40, dtype=np.int32) % 5, 39 - np.arange(40, dtype=np.int32)
    got = eng.pairs_many(s[:5], t, edges=edges, src_index=si, tgt_index=ti)
    want = an.Engine(gold(golden_dir)["table"]).pairs_many(s[:5], t, edges=edges, src_index=si, tgt_index=ti)
    assert _same(got, want)
    feats = eng.features_many(s)
    assert feats.shape == (40, 3) and np.array_equal(feats, out["features"][:, :3])
    assert len(eng.pairs_many([], [])) == 0


def test_an_id_outside_the_vocabulary_is_a_status_bit(golden_dir):
    src, tgt, _, want = _pool(golden_dir)
    eng, gd = _eng(golden_dir), gold(golden_dir)
    V = len(gd["table"])
    lo = 16                                                                             # pairs 16 .. 23: two workgroups
    s, t = [list(b) for b in src[lo:lo + 8]], [list(b) for b in tgt[lo:lo + 8]]
    s[2][len(s[2]) // 2] = V
    t[2][1] = -1
    t[5][len(t[5]) // 2] = 1 << 30
    out = eng.pairs_many(s, t, edges=gd["edges"])
    ref = an.Engine(gd["table"]).pairs_many(s, t, edges=gd["edges"])
    assert _same(out, ref)
    assert [int(x) & 1 for x in out["status"]] == [0, 0, 1, 0, 0, 1, 0, 0]
    keep = [0, 1, 3, 4, 6, 7]
    assert _same(out[keep], want[[lo + i for i in keep]])                               # the neighbours' results are intact


def test_refusal_past_the_token_limit_and_going_on(golden_dir):
    from etude_amd import _lib
    src, tgt, _, _ = _pool(golden_dir)
    eng = _eng(golden_dir)
    long_bar = src[14] + [src[14][1]]
    assert len(src[14]) == 4096
    with pytest.raises(_lib.EtudeHipError, match=r"bar 1 has 4097 tokens \(> 4096"):
        eng.pairs_many([src[0], long_bar], [tgt[0], tgt[1]])
    assert _same(eng.pairs_many(src[:2], tgt[:2], edges=gold(golden_dir)["edges"]), _pool_run(golden_dir)[:2])


def test_attribute_adherence_of_a_hand_built_result(golden_dir):
    from etude_amd.attributes import attribute_adherence
    from etude_amd.decoder import PackedBars
    gd = gold(golden_dir)
    cond = PackedBars.from_lists(gd["src_bars"][40:45])                                 # one song: its five condition bars shared by three tuples
    a4 = [np.tile(np.asarray([[2, p, 2 - p, 1]], np.int32), (5, 1)) for p in range(3)]  # the ABI order: overlap, polyphony, sustain, rhythm
    jobs = [(cond, a) for a in a4]
    covers = [gd["tgt_bars"][40:45], gd["tgt_bars"][60:63], gd["tgt_bars"][80:85]]      # the second is cut short
    results = [covers[0], (np.asarray([x for b in covers[1] for x in b], np.int32), np.asarray([len(b) for b in covers[1]], np.int64)), covers[2]]
    got = attribute_adherence(jobs, results, gd["vocab"], gd["edges"], engine=_eng(golden_dir))
    want = attribute_adherence(jobs, results, gd["vocab"], gd["edges"], engine=an.Engine(gd["table"]))
    assert [len(j["realised"]) for j in got["per_job"]] == [5, 3, 5] and got["n_bars"] == 13
    for a, b in zip(got["per_job"], want["per_job"]):
        assert np.array_equal(a["realised"], b["realised"]) and np.array_equal(a["requested"], b["requested"]) and a["attributes"].tobytes() == b["attributes"].tobytes()
    assert np.array_equal(got["per_job"][0]["realised"], gd["g"]["bins"][40:45])
    assert np.array_equal(got["per_job"][1]["requested"], [[1, 1, 1, 2]] * 3)
    rq, rl = np.concatenate([j["requested"] for j in got["per_job"]]), np.concatenate([j["realised"] for j in got["per_job"]])
    assert np.array_equal(got["counts"], an.adherence_counts(rq, rl)) and np.array_equal(got["counts"], want["counts"])
    assert got["hit_rate"].tobytes() == want["hit_rate"].tobytes()


def test_dataset_on_the_golden_corpus_through_the_device(golden_dir, tmp_path):
    from etude_amd.attributes import EtudeDataset
    gd = gold(golden_dir)
    an.write_corpus(gd, tmp_path)
    ds = EtudeDataset(tmp_path, gd["vocab"], max_seq_len=int(gd["g"]["max_seq_len"]), context_num_past_xy_pairs=int(gd["g"]["n_ctx"]), engine=_eng(golden_dir))
    check_dataset_against_reference(ds, gd)
    assert ds.raw["attributes"].tobytes() == _golden_run(golden_dir)["attributes"].tobytes()
