"""Bar attributes on the MI355X: ``BarAttributes`` -- token ids of (condition bar, target bar) pairs -> the four relative attributes the decoder is conditioned on
(relative_polyphony, relative_rhythmic_intensity, relative_note_sustain, pitch_overlap_ratio), their corpus-wide bin edges and bins, and what is built on them:
``EtudeDataset`` (the reference's training samples) and ``attribute_adherence`` (does a generated cover realise the bins it was asked for).

Stands in for ``EtudeDataset`` of the reference (etude/data/dataset.py): one launch for a whole ragged batch of pairs, one wavefront per pair, integer counting plus one
fp64 mean in a fixed order (csrc/attributes.hip).  DESIGN.md 4i is the contract; tests/attributes_np.py restates it.  Splitting, bin edges and sample assembly are host
code, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import json
from collections import defaultdict
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._engine import Engine

SRC_CLASS_ID, TGT_CLASS_ID, PAD_CLASS_ID, ATTRIBUTE_PAD_ID = 1, 2, 0, 0
MODEL_ATTRIBUTES = ["relative_polyphony", "relative_rhythmic_intensity", "relative_note_sustain", "pitch_overlap_ratio"]
ATTRIBUTE_SHORT_NAME_MAP = {"relative_polyphony": "polyphony", "relative_rhythmic_intensity": "rhythm_intensity", "relative_note_sustain": "sustain",
                            "pitch_overlap_ratio": "pitch_overlap"}
STD_MULTIPLIERS = {"relative_rhythmic_intensity": [-0.2, 0.2], "relative_polyphony": [-0.5, 0.5], "relative_note_sustain": [-0.7, 0.7], "pitch_overlap_ratio": [-0.7, 0.7]}
# a generate_many job's attribute keys in MODEL_ATTRIBUTES order, and where each sits in the int32 [n_bars, 4] form (decoder.ABI_ATTR_KEYS: overlap, polyphony, sustain, rhythm)
JOB_ATTR_KEYS = ("polyphony_bin", "rhythm_intensity_bin", "sustain_bin", "pitch_overlap_bin")
_ABI_COLUMNS = (1, 3, 2, 0)
PAIR_DTYPE = np.dtype([("features", "<i4", (6,)), ("attributes", "<f8", (4,)), ("bins", "<i4", (4,)), ("status", "<i4")])
FEATURE_NAMES = ("note_count", "pos_event_count", "total_duration_in_16ths")
STATUS_BAD_ID, STATUS_BAD_INDEX, STATUS_NPOS_SHIFT = 1, 2, 8
TYPE_POS, TYPE_NOTE, TYPE_DURATION = 1, 2, 3      # TinyREMITokenizer.event_table's codes


def limits() -> dict:
    """Host only: the constants of the built library"""
    v = [C.c_int() for _ in range(4)]
    _lib.check(_lib.lib().etd_attr_limits(*[C.byref(x) for x in v]), "etd_attr_limits")
    return dict(zip(("max_bar_tokens", "max_pairs", "max_pos_range", "max_edges"), [x.value for x in v]))


def pack_bars(bars) -> Tuple[np.ndarray, np.ndarray]:
    """lists of id lists, a ``PackedBars`` (``ids`` / ``offsets``) or ``(flat_ids, bar_lens)`` as ``generate_many(as_arrays=True)`` returns them -> (ids int32, offsets
    int64 [n + 1])"""
    if hasattr(bars, "ids") and hasattr(bars, "offsets"):
        return np.ascontiguousarray(bars.ids, np.int32), np.ascontiguousarray(bars.offsets, np.int64)
    if isinstance(bars, tuple) and len(bars) == 2 and isinstance(bars[0], np.ndarray):
        lens = np.asarray(bars[1], np.int64).reshape(-1)
        ids = np.ascontiguousarray(bars[0], np.int32).reshape(-1)
        if (lens < 0).any() or int(lens.sum()) != ids.size:
            raise ValueError("(flat_ids, bar_lens): the lengths must be >= 0 and add up to len(flat_ids)")
    else:
        lens = np.asarray([len(b) for b in bars], np.int64)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32).reshape(-1) for b in bars])) if len(bars) else np.zeros(0, np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return ids, off


def edges_arrays(edges, max_edges: int = 2) -> Tuple[np.ndarray, np.ndarray]:
    """a dict by attribute name (``attribute_bin_edges``) or four sequences in MODEL_ATTRIBUTES order -> (fp64 [4][max_edges], int32 [4] edge counts)"""
    seqs = [edges.get(n, ()) for n in MODEL_ATTRIBUTES] if isinstance(edges, dict) else list(edges)
    if len(seqs) != 4:
        raise ValueError("edges: need one edge list per attribute (4)")
    e, n = np.zeros((4, max_edges), np.float64), np.zeros(4, np.int32)
    for j, s in enumerate(seqs):
        s = np.asarray(s, np.float64).reshape(-1)
        if s.size > max_edges:
            raise ValueError(f"edges: attribute {j} has {s.size} edges, the engine bins with at most {max_edges}")
        e[j, :s.size], n[j] = s, s.size
    return e, n


class BarAttributes(Engine):
    """Bar pairs -> structured arrays (``PAIR_DTYPE``: ``features`` int32 [6] = note_count, pos_event_count, total_duration_in_16ths of the source then of the target;
    ``attributes`` fp64 [4] in ``MODEL_ATTRIBUTES`` order; ``bins`` int32 [4], -1 without edges; ``status``).  Constructing needs no GPU; ``pairs_many`` does: there is
    no CPU path."""
    _destroy = "etd_attr_destroy"

    def __init__(self, vocab, device: Union[str, torch.device] = "cuda"):
        from .tokenizer import TinyREMITokenizer
        self.device = torch.device("cuda" if device == "auto" else device)
        self._lib = _lib.lib()
        self.limits = limits()
        tab = TinyREMITokenizer.event_table(vocab)
        self.table = np.ascontiguousarray(np.stack([tab["type"], tab["value"]], axis=1).astype(np.int32))
        cfg = _lib.AttrCfg(type_pos=TYPE_POS, type_note=TYPE_NOTE, type_duration=TYPE_DURATION)
        h = C.c_void_p()

        def create():
            _lib.check(self._lib.etd_attr_create(C.byref(cfg), C.c_void_p(self.table.ctypes.data), len(self.table), C.byref(h)), "etd_attr_create")
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self._device()):      # the event table is copied to this device
                create()
        else:
            create()
        self._adopt(h)

    def check_offsets(self, offsets: np.ndarray) -> None:
        """host only: the library's refusal of one side's bars (a bar above the token limit, too many bars), before anything touches the device"""
        off = np.ascontiguousarray(offsets, np.int64)
        _lib.check(self._lib.etd_attr_check(self.h, off.ctypes.data_as(_lib.c_i64_p), len(off) - 1), "etd_attr_check")

    def run_packed(self, src: Tuple[np.ndarray, np.ndarray], tgt: Tuple[np.ndarray, np.ndarray], src_index: Optional[np.ndarray] = None,
                   tgt_index: Optional[np.ndarray] = None, edges=None) -> np.ndarray:
        """one copy to the device, one launch, one copy back.  src / tgt: ``pack_bars`` output (the same object twice uploads it once)"""
        same = tgt is src
        (s_ids, s_off), (t_ids, t_off) = src, tgt
        P = len(src_index) if src_index is not None else len(s_off) - 1
        if (len(tgt_index) if tgt_index is not None else len(t_off) - 1) != P:
            raise ValueError("pairs_many: the two sides give different numbers of pairs")
        self.check_offsets(s_off)
        if not same:
            self.check_offsets(t_off)
        parts = [s_off] + ([] if same else [t_off])
        parts += [np.ascontiguousarray(i, np.int32) for i in (src_index, tgt_index) if i is not None]
        parts += [s_ids] + ([] if same else [t_ids])
        at, pos = [], 0
        for p in parts:
            at.append(pos)
            pos += p.nbytes
        packed = np.concatenate([p.view(np.uint8) for p in parts] + [np.zeros(8, np.uint8)])
        it = iter(at)
        o_soff = next(it)
        o_toff = o_soff if same else next(it)
        o_sidx = next(it) if src_index is not None else None
        o_tidx = next(it) if tgt_index is not None else None
        o_sids = next(it)
        o_tids = o_sids if same else next(it)
        e_arr = n_arr = None
        if edges is not None:
            e_arr, n_arr = edges_arrays(edges, self.limits["max_edges"])
        dev = self._device()
        with torch.cuda.device(dev):
            buf = torch.from_numpy(packed).to(dev)
            out = torch.empty(76 * P, dtype=torch.uint8, device=dev)      # fp64 [P][4] | int32 [P][6] | int32 [P][4] | int32 [P]
            base, ob = buf.data_ptr(), out.data_ptr()
            ptr = lambda o: C.c_void_p(base + o) if o is not None else None      # noqa: E731
            _lib.check(self._lib.etd_attr_run(
                self.h, ptr(o_sids), ptr(o_soff), s_off.ctypes.data_as(_lib.c_i64_p), len(s_off) - 1, ptr(o_sidx),
                ptr(o_tids), ptr(o_toff), t_off.ctypes.data_as(_lib.c_i64_p), len(t_off) - 1, ptr(o_tidx), P,
                C.c_void_p(e_arr.ctypes.data) if e_arr is not None else None, C.c_void_p(n_arr.ctypes.data) if n_arr is not None else None,
                C.c_void_p(ob + 32 * P), C.c_void_p(ob), C.c_void_p(ob + 56 * P) if e_arr is not None else None, C.c_void_p(ob + 72 * P), self._stream(dev)), "etd_attr_run")
            raw = out.cpu().numpy()
        res = np.empty(P, PAIR_DTYPE)
        res["attributes"] = raw[:32 * P].view(np.float64).reshape(P, 4)
        res["features"] = raw[32 * P:56 * P].view(np.int32).reshape(P, 6)
        res["bins"] = raw[56 * P:72 * P].view(np.int32).reshape(P, 4) if e_arr is not None else -1
        res["status"] = raw[72 * P:].view(np.int32)
        return res

    def pairs_many(self, src_bars, tgt_bars, edges=None, src_index=None, tgt_index=None) -> np.ndarray:
        """Pair i = (source bar i, target bar i) -- or (source bar ``src_index[i]``, target bar ``tgt_index[i]``), which lets many pairs share one uploaded bar.
        edges: ``attribute_bin_edges`` (a dict by attribute name) or four edge lists; without them ``bins`` is -1.  One copy in, one launch, one copy out; calls above
        the library's pairs-per-call limit are split.  A pair's numbers depend on its two bars alone: bit-identical alone, in any batch and from run to run."""
        src = pack_bars(src_bars)
        tgt = src if tgt_bars is src_bars else pack_bars(tgt_bars)
        P = len(src_index) if src_index is not None else len(src[1]) - 1
        cap = self.limits["max_pairs"]
        if P == 0:
            return np.zeros(0, PAIR_DTYPE)
        if P <= cap and len(src[1]) - 1 <= cap and len(tgt[1]) - 1 <= cap:
            return self.run_packed(src, tgt, src_index, tgt_index, edges)
        si = np.arange(len(src[1]) - 1, dtype=np.int64) if src_index is None else np.asarray(src_index, np.int64)
        ti = np.arange(len(tgt[1]) - 1, dtype=np.int64) if tgt_index is None else np.asarray(tgt_index, np.int64)
        outs = []
        for p0 in range(0, P, cap):      # each part brings the bars it names, renumbered
            part = []
            for (ids, off), idx in ((src, si[p0:p0 + cap]), (tgt, ti[p0:p0 + cap])):
                used, inv = np.unique(idx, return_inverse=True)
                lens = off[used + 1] - off[used]
                o = np.zeros(len(used) + 1, np.int64)
                np.cumsum(lens, out=o[1:])
                take = np.concatenate([np.arange(off[u], off[u + 1]) for u in used]) if len(used) else np.zeros(0, np.int64)
                part.append(((np.ascontiguousarray(ids[take]), o), inv.astype(np.int32)))
            outs.append(self.run_packed(part[0][0], part[1][0], part[0][1], part[1][1], edges))
        return np.concatenate(outs)

    def features_many(self, bars) -> np.ndarray:
        """bars -> int32 [n][3] = note_count, pos_event_count, total_duration_in_16ths"""
        return self.pairs_many(bars, bars)["features"][:, :3].copy()


# ---------------------------------------------------------------------------------------------------------------- host: bars, edges
def split_into_bars(ids: Sequence[int], bar_bos_id: int, bar_eos_id: int) -> List[List[int]]:
    """``EtudeDataset._split_into_bars`` (etude/data/dataset.py:177-202), the dataset's splitter (not the tokenizer's): an unterminated bar is closed with Bar_EOS,
    tokens outside a bar and bars of at most two tokens are dropped."""
    bars, current, in_bar = [], [], False
    for t in ids:
        if t == bar_bos_id:
            if in_bar and current:
                current.append(bar_eos_id)
                bars.append(current)
            current, in_bar = [t], True
        elif t == bar_eos_id:
            if in_bar:
                current.append(t)
                bars.append(current)
                current, in_bar = [], False
        elif in_bar:
            current.append(t)
    if in_bar and current:
        current.append(bar_eos_id)
        bars.append(current)
    return [b for b in bars if len(b) > 2]


def calculate_bin_edges(raw_attributes) -> Dict[str, np.ndarray]:
    """``EtudeDataset._calculate_bin_edges`` with numpy itself: mean + k std per attribute (k = -+0.2 rhythmic intensity, -+0.5 polyphony, -+0.7 sustain and overlap)
    over the finite values; fewer than two values give (-0.5, 0.5), std < 1e-6 gives mean -+ 1e-3 max(|mean|, 1 below 1e-6); then ``np.sort(np.unique(...))``.
    raw_attributes: a dict by attribute name, a ``PAIR_DTYPE`` array or an [n, 4] array in ``MODEL_ATTRIBUTES`` order; nothing at all gives empty edge lists."""
    if isinstance(raw_attributes, np.ndarray) and raw_attributes.dtype.names:
        raw_attributes = raw_attributes["attributes"]
    if not isinstance(raw_attributes, dict):
        a = np.asarray(raw_attributes, np.float64).reshape(-1, 4)
        raw_attributes = {n: a[:, j] for j, n in enumerate(MODEL_ATTRIBUTES)}
    if not len(next(iter(raw_attributes.values()), ())):
        return {n: np.array([]) for n in MODEL_ATTRIBUTES}
    out = {}
    for name in MODEL_ATTRIBUTES:
        multipliers = STD_MULTIPLIERS.get(name, [-1.0, 1.0])
        values = np.array([v for v in raw_attributes[name] if v is not None and np.isfinite(v)])
        if len(values) < 2:
            edges = np.array([-0.5, 0.5])
        else:
            mean, std = np.mean(values), np.std(values)
            if std < 1e-6:
                eps = 1e-3 * (abs(mean) if abs(mean) > 1e-6 else 1.0)
                edges = np.array([mean - eps, mean + eps])
            else:
                edges = np.array([mean + m * std for m in multipliers])
        out[name] = np.sort(np.unique(edges))
    return out


def save_bin_edges(edges: Dict[str, np.ndarray], path) -> None:
    """a small JSON file to keep next to a checkpoint: {attribute: [edges]} (``repr`` round-trips every double)"""
    Path(path).write_text(json.dumps({n: [float(x) for x in edges.get(n, ())] for n in MODEL_ATTRIBUTES}, indent=1) + "\n")


def load_bin_edges(path) -> Dict[str, np.ndarray]:
    d = json.loads(Path(path).read_text())
    return {n: np.asarray(d.get(n, []), np.float64) for n in MODEL_ATTRIBUTES}


def digitize(value: float, edges) -> int:
    """``_get_attribute_bin_id``: no edges -> the default bin 1"""
    if edges is None or len(edges) == 0:
        return 1
    return np.digitize(value, edges).item()


# ---------------------------------------------------------------------------------------------------------------- the dataset
class EtudeDataset(torch.utils.data.Dataset):
    """``EtudeDataset`` of the reference (etude/data/dataset.py) with its signature and surface: ``attribute_bin_edges``, ``len``, ``[i]``, ``collate_fn``,
    ``get_dataloader``, ``get_attributes_for_model``.  Phase 1 packs every bar pair of the corpus and computes the raw attributes in ONE ``pairs_many`` call of
    ``engine`` (default: ``BarAttributes(vocab)``); edges, the sample map and sample assembly are the reference's host code."""

    _MODEL_ATTRIBUTES = MODEL_ATTRIBUTES
    _ATTRIBUTE_SHORT_NAME_MAP = ATTRIBUTE_SHORT_NAME_MAP

    def __init__(self, dataset_dir, vocab, max_seq_len: int, src_suffix: str = "_src.npy", tgt_suffix: str = "_tgt.npy", data_format: str = "npy",
                 num_attribute_bins: int = 3, context_num_past_xy_pairs: int = 4, engine=None):
        self.dataset_dir = Path(dataset_dir)
        self.vocab, self.max_seq_len = vocab, max_seq_len
        self.src_suffix, self.tgt_suffix, self.data_format = src_suffix, tgt_suffix, data_format
        self.num_attribute_bins, self.context_num_past_xy_pairs = num_attribute_bins, context_num_past_xy_pairs
        self.pad_id, self.bar_bos_id, self.bar_eos_id = vocab.get_pad_id(), vocab.get_bar_bos_id(), vocab.get_bar_eos_id()
        if self.pad_id == -1:
            raise ValueError("'<PAD>' not found in vocabulary.")
        if self.bar_bos_id == -1 or self.bar_eos_id == -1:
            raise ValueError("'Bar_BOS' or 'Bar_EOS' not found in vocab.")
        self._songs, self.sample_map = [], []
        file_pairs = self._find_file_pairs()
        if not file_pairs:
            return
        self._songs = self._load_and_preprocess_songs(file_pairs, engine)
        if not self._songs:
            return
        self.attribute_bin_edges = self._calculate_bin_edges([b for song in self._songs for b in song["bars"]])
        self._create_sample_map()

    def __len__(self) -> int:
        return len(self.sample_map)

    def __getitem__(self, idx: int) -> Dict[str, Any]:
        if idx >= len(self.sample_map):
            raise IndexError("Index out of bounds")
        e = self.sample_map[idx]
        full = self._get_full_sample_for_bar(e["song_idx"], e["bar_idx"])
        return {k: v[e["slice"]] for k, v in full.items()}

    @classmethod
    def get_attributes_for_model(cls) -> List[str]:
        return cls._MODEL_ATTRIBUTES

    def _find_file_pairs(self) -> List[Tuple[Path, Path]]:
        pairs = []
        for d in sorted(d for d in self.dataset_dir.iterdir() if d.is_dir() and d.name.isdigit()):
            s, t = d / f"{d.name}{self.src_suffix}", d / f"{d.name}{self.tgt_suffix}"
            if s.exists() and t.exists():
                pairs.append((s, t))
        return pairs

    def _load_sequence(self, filepath: Path) -> List[int]:
        if not filepath.exists():
            return []
        try:
            if self.data_format == "npy":
                return np.load(filepath, allow_pickle=True).tolist()
            if self.data_format == "pt":
                return torch.load(filepath).tolist()
            if self.data_format == "json":
                with open(filepath, "r") as f:
                    return json.load(f)
            raise ValueError(f"Unsupported data format: {self.data_format}")
        except Exception:      # noqa: BLE001  (as the reference: an unreadable file is an empty song)
            return []

    def _split_into_bars(self, id_sequence: List[int]) -> List[List[int]]:
        return split_into_bars(id_sequence, self.bar_bos_id, self.bar_eos_id)

    def _load_and_preprocess_songs(self, file_pairs, engine=None) -> List[Dict[str, Any]]:
        loaded, src_all, tgt_all = [], [], []
        for src_f, tgt_f in file_pairs:
            c_ids, t_ids = self._load_sequence(src_f), self._load_sequence(tgt_f)
            if not c_ids or not t_ids:
                continue
            c_bars, t_bars = self._split_into_bars(c_ids), self._split_into_bars(t_ids)
            n = min(len(c_bars), len(t_bars))
            if n:
                loaded.append((src_f.parent.name, c_bars[:n], t_bars[:n]))
                src_all += c_bars[:n]
                tgt_all += t_bars[:n]
        if not loaded:
            return []
        self.engine = engine if engine is not None else BarAttributes(self.vocab)
        res = self.engine.pairs_many(src_all, tgt_all)      # the whole corpus: ONE call
        bad = np.flatnonzero(res["status"] & (STATUS_BAD_ID | STATUS_BAD_INDEX))
        if bad.size:
            raise ValueError(f"bar pair {int(bad[0])} of the corpus holds a token id outside the vocabulary")
        self.raw = res
        songs, k = [], 0
        for name, c_bars, t_bars in loaded:
            bars = []
            for c, t in zip(c_bars, t_bars):
                bars.append({"attributes": {n: float(res["attributes"][k, j]) for j, n in enumerate(MODEL_ATTRIBUTES)}, "src_bar_ids": c, "tgt_bar_ids": t})
                k += 1
            songs.append({"song_name": name, "bars": bars})
        return songs

    def _calculate_bin_edges(self, all_bar_data) -> Dict[str, np.ndarray]:
        if not all_bar_data:
            return {n: np.array([]) for n in self.get_attributes_for_model()}
        return calculate_bin_edges({n: [b["attributes"].get(n) for b in all_bar_data] for n in self.get_attributes_for_model()})

    def _get_attribute_bin_id(self, value: float, attr_name: str) -> int:
        return digitize(value, self.attribute_bin_edges.get(attr_name))

    def _create_sample_map(self) -> None:
        self.sample_map = []
        empty_bar_len, n_ctx = 2, self.context_num_past_xy_pairs
        for song_idx, song in enumerate(self._songs):
            bars = song["bars"]
            for bar_idx in range(len(bars)):
                context_len = 0
                for k in range(n_ctx):
                    h = bar_idx - (n_ctx - k)
                    context_len += len(bars[h]["src_bar_ids"]) + len(bars[h]["tgt_bar_ids"]) if h >= 0 else 2 * empty_bar_len
                full_len = context_len + len(bars[bar_idx]["src_bar_ids"]) + len(bars[bar_idx]["tgt_bar_ids"])
                for start in range(0, full_len, self.max_seq_len):
                    end = min(start + self.max_seq_len, full_len)
                    if end - start >= 2:
                        self.sample_map.append({"song_idx": song_idx, "bar_idx": bar_idx, "slice": slice(start, end)})

    def _get_full_sample_for_bar(self, song_idx: int, bar_idx: int) -> Dict[str, List[Any]]:
        bars = self._songs[song_idx]["bars"]
        names = self.get_attributes_for_model()
        short = [self._ATTRIBUTE_SHORT_NAME_MAP[k] for k in names]
        empty_bar = [self.bar_bos_id, self.bar_eos_id]
        tokens, classes, attrs = [], [], defaultdict(list)

        def binned(bar):
            return {s: self._get_attribute_bin_id(bar["attributes"][k], k) for s, k in zip(short, names)}
        for k in range(self.context_num_past_xy_pairs):
            h = bar_idx - (self.context_num_past_xy_pairs - k)
            if h >= 0:
                past = binned(bars[h])
                items = [(bars[h]["src_bar_ids"], SRC_CLASS_ID), (bars[h]["tgt_bar_ids"], TGT_CLASS_ID)]
            else:
                past = {s: 1 for s in short}      # the middle bin is neutral
                items = [(empty_bar, SRC_CLASS_ID), (empty_bar, TGT_CLASS_ID)]
            for ids, cls in items:
                tokens.extend(ids)
                classes.extend([cls] * len(ids))
                for s in short:
                    attrs[f"{s}_bin_ids"].extend([past[s]] * len(ids))
        cur = bars[bar_idx]
        xi, yi = cur["src_bar_ids"], cur["tgt_bar_ids"]
        cur_bins = binned(cur)
        n_ctx_tokens = len(tokens)
        for s in short:
            attrs[f"{s}_bin_ids"].extend([cur_bins[s]] * (len(xi) + len(yi)))
        labels = [-100] * (n_ctx_tokens + len(xi)) + yi[1:] + [-100]
        full = {"input_ids": tokens + xi + yi, "class_ids": classes + [SRC_CLASS_ID] * len(xi) + [TGT_CLASS_ID] * len(yi), "labels": labels}
        full.update(attrs)
        return full

    def collate_fn(self, batch: List[Dict[str, Any]]) -> Dict[str, torch.Tensor]:
        batch = [item for item in batch if item and "input_ids" in item]
        if not batch:
            return {}
        max_len = max(len(item["input_ids"]) for item in batch)
        keys = ["input_ids", "class_ids", "labels"] + [f"{self._ATTRIBUTE_SHORT_NAME_MAP[k]}_bin_ids" for k in self.get_attributes_for_model()]
        pad_of = {"labels": -100, "input_ids": self.pad_id, "class_ids": PAD_CLASS_ID}
        padded = defaultdict(list)
        for item in batch:
            pad_len = max_len - len(item["input_ids"])
            for key in keys:
                padded[key].append(item.get(key, []) + [pad_of.get(key, ATTRIBUTE_PAD_ID)] * pad_len)
            padded["attention_mask"].append([1] * len(item["input_ids"]) + [0] * pad_len)
        return {k: torch.tensor(v, dtype=torch.long) for k, v in padded.items()}

    def get_dataloader(self, batch_size: int, shuffle: bool = True, num_workers: int = 0, **kwargs):
        from torch.utils.data import DataLoader
        if not self.sample_map:
            return DataLoader([])
        return DataLoader(self, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, collate_fn=self.collate_fn, **kwargs)


# ---------------------------------------------------------------------------------------------------------------- adherence
def requested_bins(attrs) -> np.ndarray:
    """a generate_many job's attributes (dicts, or the int32 [n_bars, 4] form in ``decoder.ABI_ATTR_KEYS`` order) -> int32 [n_bars, 4] in ``MODEL_ATTRIBUTES`` order"""
    if isinstance(attrs, np.ndarray):
        return np.ascontiguousarray(attrs.reshape(-1, 4)[:, _ABI_COLUMNS], np.int32)
    return np.asarray([[a[k] for k in JOB_ATTR_KEYS] for a in attrs], np.int32).reshape(-1, 4)


def attribute_adherence(jobs: Sequence, results: Sequence, vocab, edges, engine=None, device="cuda") -> Dict[str, Any]:
    """Does each generated cover realise the bins it was asked for?  jobs / results: those of ``EtudeDecoder.generate_many`` (condition bars as lists or ``PackedBars``,
    attributes as dicts or arrays; covers as lists of bars or ``(flat_ids, bar_lens)``).  Bar i of a cover is paired with condition bar i; a cover shorter than its
    conditions is judged on the bars it has.  ONE device call serves all jobs, and a song's condition bars, shared by its attribute tuples, are uploaded once.
    -> ``per_job``: [{"requested": int32 [n, 4], "realised": int32 [n, 4], "attributes": fp64 [n, 4]}] (``MODEL_ATTRIBUTES`` order), ``counts``: int64 [4][3][3]
    requested x realised, ``hit_rate``: fp64 [4] (nan with no bars), ``n_bars``."""
    if len(jobs) != len(results):
        raise ValueError("attribute_adherence: one result per job")
    engine = engine if engine is not None else BarAttributes(vocab, device=device)
    songs, song_base, n_src = {}, [], 0
    src_ids, src_lens, tgt_ids, tgt_lens, src_index, spans, req = [], [], [], [], [], [], []
    for (x_bars, attrs), res in zip(jobs, results):
        if id(x_bars) not in songs:      # the same object: the same song
            ids, off = pack_bars(x_bars)
            songs[id(x_bars)] = (n_src, len(off) - 1)
            song_base.append(x_bars)
            src_ids.append(ids); src_lens.append(np.diff(off))
            n_src += len(off) - 1
        base, n_x = songs[id(x_bars)]
        r_ids, r_off = pack_bars(res)
        n = min(n_x, len(r_off) - 1)
        rq = requested_bins(attrs)
        if len(rq) < n:
            raise ValueError("attribute_adherence: a job has fewer attribute rows than bars")
        tgt_ids.append(r_ids[:r_off[n]]); tgt_lens.append(np.diff(r_off[:n + 1]))
        src_index.append(base + np.arange(n, dtype=np.int32))
        spans.append(n)
        req.append(rq[:n])
    total = int(sum(spans))
    counts = np.zeros((4, 3, 3), np.int64)
    if total == 0:
        return dict(per_job=[dict(requested=r, realised=np.zeros((0, 4), np.int32), attributes=np.zeros((0, 4))) for r in req], counts=counts,
                    hit_rate=np.full(4, np.nan), n_bars=0)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt, copy=False))      # noqa: E731
    out = engine.pairs_many((cat(src_ids, np.int32), cat(src_lens, np.int64)), (cat(tgt_ids, np.int32), cat(tgt_lens, np.int64)), edges=edges,
                            src_index=cat(src_index, np.int32))
    if (out["status"] & (STATUS_BAD_ID | STATUS_BAD_INDEX)).any():
        raise ValueError("attribute_adherence: a bar holds a token id outside the vocabulary")
    per_job, k = [], 0
    for n, rq in zip(spans, req):
        per_job.append(dict(requested=rq, realised=out["bins"][k:k + n].copy(), attributes=out["attributes"][k:k + n].copy()))
        k += n
    rq_all, rl_all = np.concatenate(req), out["bins"]
    if rq_all.min() < 0 or rq_all.max() > 2 or rl_all.min() < 0 or rl_all.max() > 2:
        raise ValueError("attribute_adherence: bins outside 0 .. 2 (three bins per attribute)")
    for j in range(4):
        np.add.at(counts[j], (rq_all[:, j], rl_all[:, j]), 1)
    hit = np.array([np.trace(counts[j]) / total for j in range(4)])
    return dict(per_job=per_job, counts=counts, hit_rate=hit, n_bars=total)
