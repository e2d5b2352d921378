#!/usr/bin/env python3
"""Generate tests/golden/attributes_cases.npz by RUNNING THE REFERENCE's EtudeDataset (etude/data/dataset.py) on a small seeded corpus.

Runs only where the reference checkout, numpy, torch and tqdm are available; the packages' own __init__ files are not run (package stubs, as make_golden_rhythm.py).
Stored: data only -- the corpus' id sequences, the synthetic vocabulary's token list, and the reference's outputs: ``_split_into_bars``, ``_extract_bar_features``,
``_compute_musical_attributes``, ``_calculate_bin_edges`` (the corpus' and three hand-made inputs for its branches), ``_get_attribute_bin_id``, the sample map, four
``__getitem__`` chunks and their ``collate_fn`` batch.

The vocabulary holds Pos_0 .. Pos_191.  Song 0001 is hand-built: a source bar with no Pos, bars with no notes, a Note and a Duration before the first Pos, a repeated
Pos value, positions held by one side only, an empty [BOS, EOS] bar (dropped), a bar opened inside a bar, tokens outside bars, an unterminated last bar, and pairs with
1, 7, 8, 9, 128, 129 and 192 distinct positions.  Songs 0002 .. 0004 are random.  The corpus seed is advanced until no attribute value of the REFERENCE lies within
1e-9 (relative) of one of its own bin edges, so that the last bit of a mean cannot decide a bin; that is asserted below on the reference's numbers alone.

Usage:  python tests/golden/make_golden_attributes.py --reference DIR
"""
from __future__ import annotations

import argparse
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
MAX_SEQ_LEN, N_CTX = 300, 4
NAMES = ("relative_polyphony", "relative_rhythmic_intensity", "relative_note_sustain", "pitch_overlap_ratio")
SHORT = ("polyphony", "rhythm_intensity", "sustain", "pitch_overlap")


def load_reference(ref: str):
    ref = Path(ref)
    for pkg in ("etude", "etude.data", "etude.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(ref.joinpath(*pkg.split(".")))]
        sys.modules[pkg] = m
    import etude.data.dataset as dataset
    import etude.data.vocab as vocab
    return dataset, vocab


def make_vocab(vocab_mod):
    v = vocab_mod.Vocab()
    toks = ["Bar_BOS", "Bar_EOS"] + [f"Pos_{i}" for i in range(192)] + [f"Note_{p}" for p in range(21, 109)] + [f"Duration_{d}" for d in range(1, 33)]
    toks += ["Grace_0", "Grace_1", "TimeSig_4"]
    for t in toks:
        v._add_token(t)
    return v


def bar(v, body, close=True):
    return [v.encode("Bar_BOS")] + [v.encode(t) for t in body] + ([v.encode("Bar_EOS")] if close else [])


def notes_at(rng, positions, lo=1, hi=4):
    body = []
    for p in positions:
        body.append(f"Pos_{int(p)}")
        for _ in range(int(rng.integers(lo, hi + 1))):
            body += [f"Note_{int(rng.integers(21, 109))}", f"Duration_{int(rng.integers(1, 33))}"]
            if rng.random() < 0.05:
                body.append("Grace_1")
    return body


def random_bar(rng, v, n_pos):
    return bar(v, notes_at(rng, np.sort(rng.choice(192, size=n_pos, replace=False))))


def special_song(rng, v):
    src, tgt = [v.encode("<BOS>")], [v.encode("<BOS>"), v.encode("Note_60")]      # tokens outside a bar are dropped
    def both(s, t):
        src.extend(s); tgt.extend(t)
    both(bar(v, ["Note_60", "Duration_4", "Note_64", "Duration_2"]), random_bar(rng, v, 5))                      # source with no Pos: the defaults 1.0
    both(bar(v, ["Pos_0", "Pos_8"]), random_bar(rng, v, 3))                                                      # source with no notes
    both(random_bar(rng, v, 4), bar(v, ["Pos_0", "Pos_8", "Pos_16"]))                                            # target with no notes
    both(bar(v, ["Pos_0"]), bar(v, ["Pos_4", "Pos_4"]))                                                          # no notes at all: no positions
    both(bar(v, ["Note_60", "Duration_8", "Pos_0", "Note_62", "Duration_4"]), bar(v, ["Duration_3", "Note_50", "Pos_0", "Note_74", "Duration_4", "Note_63", "Duration_2"]))
    both(bar(v, ["Pos_4", "Note_60", "Duration_2", "Pos_8", "Note_64", "Duration_2", "Pos_4", "Note_67", "Duration_2"]),
         bar(v, ["Pos_4", "Note_72", "Duration_2", "Pos_4", "Note_79", "Duration_1", "Note_61", "Duration_1", "Pos_8", "Note_65", "Duration_2"]))      # a repeated Pos value
    both(bar(v, ["Pos_0", "Note_60", "Duration_4", "Pos_16", "Note_64", "Duration_4"]), bar(v, ["Pos_0", "Note_48", "Duration_4", "Pos_32", "Note_64", "Duration_4"]))
    src.extend(bar(v, []))                                                                                       # an empty bar: dropped, on the source side only
    src.append(v.encode("Note_70"))                                                                              # between two bars: dropped
    both(random_bar(rng, v, 6)[:-1], random_bar(rng, v, 6))                                                      # a bar opened inside a bar: the first is closed
    for n_s, n_t in ((1, 1), (7, 3), (8, 8), (9, 5), (128, 100), (129, 129), (192, 192)):                      # the target's positions among the source's: n_s in all
        ps = np.sort(rng.choice(192, size=n_s, replace=False))
        both(bar(v, notes_at(rng, ps)), bar(v, notes_at(rng, np.sort(rng.choice(ps, size=n_t, replace=False)))))
    for n_s, n_t in ((60, 192), (130, 2)):
        both(random_bar(rng, v, n_s), random_bar(rng, v, n_t))
    both(random_bar(rng, v, 9), random_bar(rng, v, 7))
    src.extend(random_bar(rng, v, 3)); src.extend(random_bar(rng, v, 3))                                         # the source is one bar longer: min() of the two
    tgt.extend(random_bar(rng, v, 4)[:-1])                                                                       # the target ends unterminated
    return src, tgt


def random_song(rng, v, n_bars):
    src, tgt = [], []
    for _ in range(n_bars):
        n_s = int(rng.choice([1, 2, 4, 6, 8, 12, 16, 24]))
        n_t = int(np.clip(n_s + rng.integers(-3, 8), 1, 40))
        src.extend(random_bar(rng, v, n_s)); tgt.extend(random_bar(rng, v, n_t))
    return src, tgt


def corpus(seed, v):
    rng = np.random.default_rng(seed)
    return [special_song(rng, v)] + [random_song(rng, v, n) for n in (45, 60, 52)]


def clear_of_edges(attrs, edges) -> bool:
    for j, n in enumerate(NAMES):
        for e in edges[n]:
            if (np.abs(attrs[:, j] - e) <= 1e-9 * max(abs(e), 1e-300)).any():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    dataset_mod, vocab_mod = load_reference(args.reference)
    v = make_vocab(vocab_mod)
    seed = 0
    while True:
        songs = corpus(seed, v)
        with tempfile.TemporaryDirectory() as td:
            for i, (s, t) in enumerate(songs):
                d = Path(td) / f"{i + 1:04d}"
                d.mkdir()
                np.save(d / f"{d.name}_src.npy", np.asarray(s, np.int64))
                np.save(d / f"{d.name}_tgt.npy", np.asarray(t, np.int64))
            (Path(td) / "notes").mkdir()      # not a song directory
            ds = dataset_mod.EtudeDataset(td, v, max_seq_len=MAX_SEQ_LEN, context_num_past_xy_pairs=N_CTX)
        bars = [b for song in ds._songs for b in song["bars"]]
        attrs = np.asarray([[b["attributes"][n] for n in NAMES] for b in bars], np.float64)
        if clear_of_edges(attrs, ds.attribute_bin_edges):
            break
        seed += 1
    assert clear_of_edges(attrs, ds.attribute_bin_edges), "a reference attribute value lies within 1e-9 of one of its bin edges"

    save = dict(seed=np.int64(seed), max_seq_len=np.int64(MAX_SEQ_LEN), n_ctx=np.int64(N_CTX), tokens=np.asarray(v.id_to_token), special_tokens=np.asarray(v.special_tokens))
    for i, (s, t) in enumerate(songs):
        save[f"song{i}_src"], save[f"song{i}_tgt"] = np.asarray(s, np.int32), np.asarray(t, np.int32)
        for side, seq in (("src", s), ("tgt", t)):
            split = ds._split_into_bars(list(seq))
            save[f"song{i}_{side}_bars"] = np.asarray([x for b in split for x in b], np.int32)
            save[f"song{i}_{side}_bar_lens"] = np.asarray([len(b) for b in split], np.int64)
    feats, n_pos, bins = [], [], []
    for b in bars:
        c, t = ds._extract_bar_features(b["src_bar_ids"]), ds._extract_bar_features(b["tgt_bar_ids"])
        again = ds._compute_musical_attributes(c, t)
        assert all(again[n] == b["attributes"][n] for n in NAMES)
        feats.append([c["note_count"], c["pos_event_count"], c["total_duration_in_16ths"], t["note_count"], t["pos_event_count"], t["total_duration_in_16ths"]])
        n_pos.append(len(set(c["notes_by_position"]) | set(t["notes_by_position"])))
        bins.append([ds._get_attribute_bin_id(b["attributes"][n], n) for n in NAMES])
    n_pos = np.asarray(n_pos, np.int64)
    for want in (0, 1, 7, 8, 9, 128, 129, 192):
        assert (n_pos == want).any(), want
    assert (n_pos >= 129).any() and ((n_pos >= 8) & (n_pos <= 128)).any() and (n_pos == 0).any()
    save.update(song_of_pair=np.asarray([i for i, song in enumerate(ds._songs) for _ in song["bars"]], np.int64), features=np.asarray(feats, np.int32), attributes=attrs,
                n_pos=n_pos, bins=np.asarray(bins, np.int32))
    for n in NAMES:
        save[f"edges_{n}"] = np.asarray(ds.attribute_bin_edges[n], np.float64)
    save["sample_map"] = np.asarray([[e["song_idx"], e["bar_idx"], e["slice"].start, e["slice"].stop] for e in ds.sample_map], np.int64)
    keys = ["input_ids", "class_ids", "labels"] + [f"{s}_bin_ids" for s in SHORT]
    multi = [i for i, e in enumerate(ds.sample_map) if e["slice"].start > 0]
    picks = [0, multi[0], multi[len(multi) // 2], len(ds) - 1]
    save["chunk_index"] = np.asarray(picks, np.int64)
    items = [ds[i] for i in picks]
    for k, item in enumerate(items):
        for key in keys:
            save[f"chunk{k}_{key}"] = np.asarray(item[key], np.int64)
    for key, val in ds.collate_fn(items).items():
        save[f"collate_{key}"] = val.numpy()
    # the branches of _calculate_bin_edges on hand-made values (nan / inf: filtered)
    branch = {"one_value": np.array([[1.5, 0.5, 2.0, 0.25]]),
              "constant": np.array([[1.0, 0.0, 3.0, 1e-9]] * 5 + [[np.nan, np.inf, -np.inf, np.nan]]),
              "spread": np.array([[0.5, 1.0, 2.0, 0.1], [1.5, 1.0, 2.5, 0.9], [np.nan, 3.0, 0.5, 0.5], [1.0, 2.0, 1.0, 0.3]])}
    for name, a in branch.items():
        e = ds._calculate_bin_edges([{"attributes": {n: float(row[j]) for j, n in enumerate(NAMES)}} for row in a])
        save[f"branch_{name}_in"] = a
        for n in NAMES:
            save[f"branch_{name}_{n}"] = np.asarray(e[n], np.float64)
    assert all(len(x) == 0 for x in ds._calculate_bin_edges([]).values())
    path = HERE / "attributes_cases.npz"
    np.savez_compressed(path, **save)
    print("wrote", path, path.stat().st_size, "bytes; seed", seed, ";", len(bars), "bar pairs,", len(ds), "chunks; n_pos", sorted(set(n_pos.tolist()))[-5:],
          "bins", np.bincount(np.asarray(bins).reshape(-1), minlength=3).tolist())


if __name__ == "__main__":
    main()
