"""Teacher-forced scoring, host side (no GPU): the sequence etd_decoder_score_jobs builds for a cover bar (etd_debug_assemble_scored) against
the oracle's prompt rule plus the forced tokens, the refusals of the C ABI, and EtudeDecoder.forward's checks of a right-padded batch."""
import ctypes as C

import numpy as np
import pytest

from etude_amd import _lib
from etude_amd.decoder import ABI_ATTR_KEYS, IGNORE_INDEX, right_padded_lengths
from oracle import neox

BOS, EOS = 4, 5


def _cfg(n_ctx=4, max_pos=1024, limit=512, ratio=0.5):
    return _lib.SchedCfg(bar_bos_id=BOS, bar_eos_id=EOS, n_ctx_pairs=n_ctx, max_position_embeddings=max_pos, max_output_tokens=25600,
                         max_bar_token_limit=limit, context_overlap_ratio=ratio, force_bar_tokens=0, max_streams=1, max_prefill_rows=4096,
                         steps_per_poll=8)


def _native_scored(hist, x, y, ya, sc, cap=4096):
    """etd_debug_assemble_scored: hist = [(xs, ys, attrs dict)], y = [Bar_BOS] + tokens.  Returns (rc, ids, cls, attrs dict, labels)."""
    lib = _lib.lib()
    n = len(hist)
    hx = [np.asarray(h[0], np.int32) for h in hist]
    hy = [np.asarray(h[1], np.int32) for h in hist]
    hxp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in hx])
    hyp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in hy])
    hxn = np.asarray([a.size for a in hx] or [0], np.int32)
    hyn = np.asarray([a.size for a in hy] or [0], np.int32)
    ha = np.ascontiguousarray(np.asarray([[h[2][k] for k in ABI_ATTR_KEYS] for h in hist] or [[0, 0, 0, 0]], np.int32))
    xa, yv = np.asarray(x, np.int32), np.asarray(y, np.int32)
    yat = np.asarray([ya[k] for k in ABI_ATTR_KEYS], np.int32)
    ids, cls, lab = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    at = np.zeros((4, cap), np.int32)
    T = C.c_int()
    rc = lib.etd_debug_assemble_scored(C.byref(sc), n, hxp, hxn.ctypes.data, hyp, hyn.ctypes.data, ha.ctypes.data, xa.ctypes.data, xa.size,
                                       yv.ctypes.data, yv.size, yat.ctypes.data, ids.ctypes.data, cls.ctypes.data, at.ctypes.data, lab.ctypes.data,
                                       cap, C.byref(T))
    t = T.value
    return rc, ids[:t].tolist(), cls[:t].tolist(), {k: at[j, :t].tolist() for j, k in enumerate(ABI_ATTR_KEYS)}, lab[:t].tolist()


def _oracle_scored(hist, x, y, ya, d, limit, ratio):
    """generate()'s prompt for the bar (oracle.neox.build_bar_prompt) + the tokens fed back while producing y; labels = the next token"""
    keys = sorted(ABI_ATTR_KEYS)
    toks, cls, al = neox.build_bar_prompt(hist, x, ya, keys, BOS, EOS, d, limit, ratio)
    if len(y) <= 1:
        return [], [], {k: [] for k in ABI_ATTR_KEYS}, []
    forced = list(y[1:-1])
    ids = toks + forced
    cls = cls + [2] * len(forced)
    at = {k: al[k] + [ya[k]] * len(forced) for k in ABI_ATTR_KEYS}
    labels = [IGNORE_INDEX] * (len(toks) - 1) + list(y[1:])
    return ids, cls, at, labels


@pytest.mark.parametrize("max_pos,limit,ratio", [(1024, 512, 0.5), (256, 100, 0.25)])
def test_scored_sequence_matches_oracle_prompt_plus_forced_tokens(max_pos, limit, ratio):
    """bars 0..6 of a song (the 4-pair history window fills, then slides); (256, 100, 0.25) truncates the prompt once the history has grown"""
    rng = np.random.default_rng(11)
    d = neox.NeoxDims(max_position_embeddings=max_pos, context_num_past_xy_pairs=4)
    sc = _cfg(4, max_pos, limit, ratio)
    hist = []
    truncated = 0
    for i in range(7):
        x = [BOS] + rng.integers(6, 150, int(rng.integers(4, 60))).tolist() + [EOS]
        n_tok = int(rng.integers(1, 41))
        y = [BOS] + rng.integers(6, 150, n_tok - 1).tolist() + [EOS]
        ya = {k: int(rng.integers(0, 3)) for k in ABI_ATTR_KEYS}
        rc, *got = _native_scored(hist, x, y, ya, sc)
        assert rc == 0, _lib.lib().etd_last_error()
        want = _oracle_scored(hist, x, y, ya, d, limit, ratio)
        assert tuple(got) == tuple(want), i
        ids, _, _, labels = got
        assert len(ids) == len(labels)
        assert sum(l != IGNORE_INDEX for l in labels) == len(y) - 1
        prompt = len(ids) - (len(y) - 2)
        assert labels[prompt - 1] == y[1] and ids[prompt - 1] == BOS
        truncated += len(neox.build_bar_prompt(hist, x, ya, sorted(ABI_ATTR_KEYS), BOS, EOS, d, -10 ** 6, ratio)[0]) != prompt
        hist.append((x, y, ya))
    if limit == 100:
        assert truncated >= 3
    else:
        assert truncated == 0


def test_bos_only_bar_scores_nothing_and_long_bar_is_refused():
    sc = _cfg(4, 1024, 16, 0.5)
    ya = {k: 1 for k in ABI_ATTR_KEYS}
    x = [BOS, 7, 8, EOS]
    rc, ids, cls, at, lab = _native_scored([], x, [BOS], ya, sc)
    assert rc == 0 and ids == [] and lab == []
    rc, ids, _, _, lab = _native_scored([], x, [BOS] + [9] * 15 + [EOS], ya, sc)      # 16 tokens = the limit: fine
    assert rc == 0 and sum(l != IGNORE_INDEX for l in lab) == 16
    rc, *_ = _native_scored([], x, [BOS] + [9] * 16 + [EOS], ya, sc)                   # 17 tokens
    assert rc == -22 and b"max_bar_token_limit" in _lib.lib().etd_last_error()
    rc, *_ = _native_scored([], x, [9, 10, EOS], ya, sc)                               # not a generated bar
    assert rc == -22 and b"Bar_BOS" in _lib.lib().etd_last_error()


def test_score_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib.lib()
    T = np.asarray([3], np.int32)
    z = np.zeros(12, np.int32)
    out = np.zeros(1, np.float64)
    assert lib.etd_decoder_score(None, 1, T.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                 out.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, None, None) == -22
    assert b"score" in lib.etd_last_error()
    sc = _cfg()
    assert lib.etd_decoder_score_jobs(None, C.byref(sc), None, 0, None, None, None, None) == -22


def test_forward_padding_checks():
    m = np.asarray([[1, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0]])
    assert right_padded_lengths((3, 4), m).tolist() == [3, 4, 1]
    assert right_padded_lengths((2, 5)).tolist() == [5, 5]
    lab = np.full((3, 4), IGNORE_INDEX)
    lab[1, 2] = 7
    assert right_padded_lengths((3, 4), m, lab).tolist() == [3, 4, 1]
    with pytest.raises(ValueError, match="right padding"):
        right_padded_lengths((2, 3), np.asarray([[0, 1, 1], [1, 1, 1]]))          # left padding
    with pytest.raises(ValueError, match="right padding"):
        right_padded_lengths((1, 4), np.asarray([[1, 0, 1, 0]]))                  # a hole
    with pytest.raises(ValueError, match="0 / 1"):
        right_padded_lengths((1, 2), np.asarray([[1, 2]]))
    bad = lab.copy()
    bad[2, 3] = 9                                                                  # label on a padded position
    with pytest.raises(ValueError, match="padded position"):
        right_padded_lengths((3, 4), m, bad)
    import torch
    assert right_padded_lengths((3, 4), torch.from_numpy(m), torch.from_numpy(lab)).tolist() == [3, 4, 1]


def test_forward_refuses_unsupported_arguments_before_touching_a_gpu():
    from etude_amd.decoder import EtudeDecoder
    dec = object.__new__(EtudeDecoder)         # no device needed: the refusals come first
    ids = np.zeros((1, 4), np.int64)
    with pytest.raises(NotImplementedError):
        dec.forward(ids, ids, ids, ids, ids, ids, past_key_values=((None, None),))
    with pytest.raises(NotImplementedError):
        dec.forward(ids, ids, ids, ids, ids, ids, inputs_embeds=np.zeros((1, 4, 8), np.float32))
