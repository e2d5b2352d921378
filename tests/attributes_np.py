"""Plain-Python / fp64 numpy restatement of the bar-attribute engine's contract: the six counts of a (condition bar, target bar) pair, its four relative
attributes, their bins and the status word, from the token ids and the vocabulary's event table.

Written from the contract and from the reference's ``_extract_bar_features`` / ``_compute_musical_attributes`` (etude/data/dataset.py:204-270), not from the device
code: one token at a time, dicts keyed by position, the pitch-overlap ratios in ASCENDING position value (the engine's own rule: the reference walks a Python set) and
their mean as numpy's add.reduce spelled out (``rhythm_np.np_sum``) over one correctly rounded division.  The device is held to it bit for bit.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from rhythm_np import np_sum  # noqa: E402

TYPE_POS, TYPE_NOTE, TYPE_DURATION = 1, 2, 3      # TinyREMITokenizer.event_table's codes
ATTRIBUTES = ("relative_polyphony", "relative_rhythmic_intensity", "relative_note_sustain", "pitch_overlap_ratio")
BAD_ID, BAD_INDEX, NPOS_SHIFT = 1, 2, 8
MAX_BAR_TOKENS = 4096
PAIR_DTYPE = np.dtype([("features", "<i4", (6,)), ("attributes", "<f8", (4,)), ("bins", "<i4", (4,)), ("status", "<i4")])


def bar_features(ids, table):
    """-> (note_count, pos_event_count, total_duration_in_16ths, {position: [pitches]}, an id was outside the table)"""
    notes = poss = dur = 0
    by_pos, cur, bad = {}, -1, False
    for i in ids:
        i = int(i)
        if not 0 <= i < len(table):
            bad = True
            continue
        ty, val = int(table[i][0]), int(table[i][1])
        if ty == TYPE_POS:
            poss += 1
            cur = val
        elif ty == TYPE_NOTE and cur != -1:
            notes += 1
            by_pos.setdefault(cur, []).append(val)
        elif ty == TYPE_DURATION:
            dur += val
    return notes, poss, dur, by_pos, bad


def _safe_div(n, d, default=0.0):
    return n / d if d else default


def pair(src_ids, tgt_ids, table, edges=None) -> dict:
    """edges: None, four ascending sequences of 0 .. 2 edges in ATTRIBUTES order, or a dict of them by attribute name"""
    if isinstance(edges, dict):
        edges = [edges.get(n, ()) for n in ATTRIBUTES]
    sn, sp, sd, s_by, s_bad = bar_features(src_ids, table)
    tn, tp, td, t_by, t_bad = bar_features(tgt_ids, table)
    a = [0.0] * 4
    a[0] = _safe_div(_safe_div(tn, tp), _safe_div(sn, sp), 1.0)
    a[1] = _safe_div(tp, sp, 1.0)
    a[2] = _safe_div(_safe_div(td, tn), _safe_div(sd, sn), 1.0)
    keys = sorted(set(s_by) | set(t_by))
    ratios = []
    for p in keys:
        if p in t_by:
            src_pc = {c % 12 for c in s_by.get(p, [])}
            ratios.append(sum(1 for t in t_by[p] if t % 12 in src_pc) / len(t_by[p]))
        else:
            ratios.append(0.0)
    a[3] = np_sum(ratios) / float(len(ratios)) if ratios else 0.0
    bins = [-1] * 4
    if edges is not None:
        for j in range(4):
            e = [float(x) for x in edges[j]]
            bins[j] = sum(1 for x in e if not a[j] < x) if e else 1
    status = (BAD_ID if s_bad or t_bad else 0) | (len(keys) << NPOS_SHIFT)
    return dict(features=[sn, sp, sd, tn, tp, td], attributes=[float(x) for x in a], bins=bins, status=status, n_pos=len(keys))


def as_bar_lists(bars):
    """lists of id lists, an object with ``ids`` / ``offsets`` (PackedBars) or ``(flat_ids, bar_lens)`` -> a list of id lists"""
    if hasattr(bars, "ids") and hasattr(bars, "offsets"):
        return [list(map(int, bars.ids[bars.offsets[i]: bars.offsets[i + 1]])) for i in range(len(bars.offsets) - 1)]
    if isinstance(bars, tuple) and len(bars) == 2 and isinstance(bars[0], np.ndarray):
        ends = np.cumsum(np.asarray(bars[1], np.int64))
        return [list(map(int, bars[0][e - l: e])) for l, e in zip(np.asarray(bars[1], np.int64).tolist(), ends.tolist())]
    return [list(map(int, b)) for b in bars]


class Engine:
    """the surface of ``etude_amd.BarAttributes`` on the host: what the CPU tests hand to ``EtudeDataset(engine=...)``"""

    def __init__(self, table):
        self.table = [(int(t), int(v)) for t, v in np.asarray(table).tolist()] if not isinstance(table, list) else table
        self.calls = 0

    def pairs_many(self, src_bars, tgt_bars, edges=None, src_index=None, tgt_index=None) -> np.ndarray:
        self.calls += 1
        src, tgt = as_bar_lists(src_bars), as_bar_lists(tgt_bars)
        si = list(range(len(src))) if src_index is None else [int(i) for i in src_index]
        ti = list(range(len(tgt))) if tgt_index is None else [int(i) for i in tgt_index]
        assert len(si) == len(ti)
        out = np.zeros(len(si), PAIR_DTYPE)
        for k, (i, j) in enumerate(zip(si, ti)):
            for b in (src[i], tgt[j]):
                if len(b) > MAX_BAR_TOKENS:
                    raise ValueError(f"a bar of {len(b)} tokens (> {MAX_BAR_TOKENS})")
            r = pair(src[i], tgt[j], self.table, edges)
            out[k] = (r["features"], r["attributes"], r["bins"], r["status"])
        return out

    def features_many(self, bars) -> np.ndarray:
        return self.pairs_many(bars, bars)["features"][:, :3].copy()


def adherence_counts(requested, realised) -> np.ndarray:
    """[n, 4] requested and realised bins -> the [4][3][3] requested x realised count matrix"""
    m = np.zeros((4, 3, 3), np.int64)
    for rq, rl in zip(np.asarray(requested).reshape(-1, 4).tolist(), np.asarray(realised).reshape(-1, 4).tolist()):
        for j in range(4):
            m[j, rq[j], rl[j]] += 1
    return m


# ---------------------------------------------------------------------------------------------------------------- the goldens
def load_golden(path) -> dict:
    """tests/golden/attributes_cases.npz (the reference's EtudeDataset on a seeded corpus, make_golden_attributes.py) -> a dict with the vocabulary rebuilt, the event
    table, the songs' id sequences, the reference's bars and, per bar pair, its outputs"""
    from etude_amd.tokenizer import TinyREMITokenizer
    from etude_amd.vocab import Vocab
    g = np.load(path)
    v = Vocab(special_tokens=[str(t) for t in g["special_tokens"]])
    for t in g["tokens"]:
        v._add_token(str(t))
    tab = TinyREMITokenizer.event_table(v)
    n_songs = len([k for k in g.files if k.startswith("song") and k.endswith("_src")])

    def bars(i, side):
        flat, lens = g[f"song{i}_{side}_bars"], g[f"song{i}_{side}_bar_lens"]
        ends = np.cumsum(lens)
        return [flat[e - l: e].tolist() for l, e in zip(lens.tolist(), ends.tolist())]
    songs = [dict(src=g[f"song{i}_src"].tolist(), tgt=g[f"song{i}_tgt"].tolist(), src_bars=bars(i, "src"), tgt_bars=bars(i, "tgt")) for i in range(n_songs)]
    src_bars, tgt_bars = [], []
    for s in songs:
        n = min(len(s["src_bars"]), len(s["tgt_bars"]))
        src_bars += s["src_bars"][:n]
        tgt_bars += s["tgt_bars"][:n]
    assert len(src_bars) == len(g["attributes"])
    return dict(g=g, vocab=v, table=np.stack([tab["type"], tab["value"]], axis=1).astype(np.int32), songs=songs, src_bars=src_bars, tgt_bars=tgt_bars,
                edges={n: g[f"edges_{n}"] for n in ATTRIBUTES})


def write_corpus(gold: dict, root) -> None:
    """the golden corpus as the dataset directory it was: NNNN/NNNN_src.npy, NNNN/NNNN_tgt.npy"""
    for i, s in enumerate(gold["songs"]):
        d = Path(root) / f"{i + 1:04d}"
        d.mkdir()
        np.save(d / f"{d.name}_src.npy", np.asarray(s["src"], np.int64))
        np.save(d / f"{d.name}_tgt.npy", np.asarray(s["tgt"], np.int64))
