"""tests/attn3_np.py pinned without a GPU: the float64 reference against torch, the plane emulation against the fp32 yardstick, the fixtures' power to show a mask
that slips by one key, and the refusals of the two test hooks (they validate on the host before anything is launched, so a CPU-only machine can ask)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn3_np as A
from etude_amd import _lib

CASES = A.all_cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("causal", [False, True])
def test_ref64_is_torch_float64_attention(causal):
    f = A.prompt(97) if causal else A.strided(88, 129)[0]
    t = [torch.from_numpy(A._heads(f[x].astype(np.float64)))[None] for x in "qkv"]
    want = torch.nn.functional.scaled_dot_product_attention(*t, is_causal=causal)[0].transpose(0, 1).reshape(f["Sq"], -1).numpy()
    assert np.abs(A.ref64(f["q"], f["k"], f["v"], causal) - want).max() <= 1e-13


def test_mutants_differ_from_ref64_by_exactly_one_key():
    f = A.prompt(33)
    q, k, v = f["q"], f["k"], f["v"]
    many, few, ref = (A.ref64(q, k, v, True, m) for m in ("many", "few", None))
    for t in (0, 5, 31):                        # query t of the "many" mutant is query t + 1's key set; of the "few" mutant query t - 1's
        assert np.abs(many[t] - A.ref64(q[t:t + 1], k[:t + 2], v[:t + 2])[0]).max() <= 1e-13
        if t:
            assert np.abs(few[t] - A.ref64(q[t:t + 1], k[:t], v[:t])[0]).max() <= 1e-13
    assert not few[0].any()
    k2, v2 = np.concatenate([k, k[-1:]]), np.concatenate([v, v[-1:]])                  # no further key: the last one twice
    assert np.abs(many[32] - A.ref64(q[32:], k2, v2)[0]).max() <= 1e-13
    s = A.strided(31, 63)[0]
    k2, v2 = np.concatenate([s["k"], s["k"][-1:]]), np.concatenate([s["v"], s["v"][-1:]])
    assert np.abs(A.ref64(s["q"], s["k"], s["v"], False, "many") - A.ref64(s["q"], k2, v2)).max() <= 1e-13
    assert np.abs(A.ref64(s["q"], s["k"], s["v"], False, "few") - A.ref64(s["q"], s["k"][:-1], s["v"][:-1])).max() <= 1e-13
    assert np.abs(many - ref).max() > 0.1 and np.abs(few - ref).max() > 0.1


def test_split_is_the_planes_arithmetic():
    """hi + lo restores an fp32 value to 2^-22 of itself while lo is a normal f16, to 2^-25 of a plane unit below; nothing overflows at the scale of a bound"""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-12, 2, 4096))).astype(np.float32)
    l2 = A.scale_log2(np.abs(x).max())
    hi, lo = A._split(x, l2)
    t = x.astype(np.float64) * 2.0 ** l2
    assert np.isfinite(hi).all() and np.abs(hi).max() < 2.0 ** 15 and np.abs(t).max() >= 2.0 ** 13
    assert (np.abs(hi + lo - t) <= np.maximum(np.abs(t) * 2.0 ** -22, 2.0 ** -25)).all()
    assert (np.abs(lo) > 0).any() and (np.abs(lo[lo != 0]) < 2.0 ** -14).any()        # subnormal lo values are kept, not flushed


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_emu_has_the_error_of_fp32_torch(case):
    _, kind, key, _ = case
    ys, l2 = A.yardsticks(kind, *key)                                            # tight bounds: the data's own maximum
    for f, (_, e32, es) in zip(A.fixtures(kind, *key), ys):
        assert es <= 3.0 * e32, (f["Sq"], f["Sk"], l2, es, e32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_mask_slips_exceed_the_device_bound_tenfold_at_every_edge_query(case):
    _, kind, key, mult = case
    ys, _ = A.yardsticks(kind, *key, mult=mult)
    for f, (ref, e32, es) in zip(A.fixtures(kind, *key), ys):
        b = A.bound(e32, es)
        for mut in ("many", "few"):
            if A.mutant_is_identity(mut, f["Sk"]):
                continue
            m = A.ref64(f["q"], f["k"], f["v"], f["causal"], mut)
            for t in f["edges"]:
                e = A.err(m, ref, f["v"], rows=[t])
                assert e >= 10.0 * b, (mut, f["Sq"], f["Sk"], t, e, b)


def test_the_cases_cover_what_they_must():
    sq = {p[0] for p in A.STRIDED_PAIRS}
    assert sq == set(A.SQ) and 25 <= len(A.STRIDED_PAIRS) <= 40
    for s in A.SQ:                                                               # every Sq with a key tail and without one
        assert any(p[0] == s and p[1] % 64 for p in A.STRIDED_PAIRS) and any(p[0] == s and p[1] % 64 == 0 for p in A.STRIDED_PAIRS)
    assert {(s, k) for s in (65, 88, 96) for k in (1, 65, 256)} <= set(A.STRIDED_PAIRS)
    for n in (32, 64, 96, 128, 192):
        assert {n - 1, n, n + 1} <= set(A.RAGGED_SINGLES)
    assert {1, 2} <= set(A.RAGGED_SINGLES)
    in_batches = {L for lens, nh in A.RAGGED_BATCHES.values() if nh == 2 for L in lens}
    assert in_batches == set(A.RAGGED_SINGLES)                                   # every length also inside a batch
    mx = sorted(max(lens) for lens, _ in A.RAGGED_BATCHES.values())
    assert any(64 < m <= 96 for m in mx) and 97 in mx


# ---------------------------------------------------------------------------------------------------------------------------------------- the hooks' refusals
FAKE = 0x7f0000000000          # a 16-byte aligned non-null "device pointer": every case below is refused before anything touches it


def _strided_case(**kw):
    H = 128
    d = dict(n_seq=2, n_heads=2, Sq=5, Sk=7, Q=FAKE, K=FAKE, V=FAKE, O=FAKE, ldq=H, ldk=H, ldv=H, ldo=H, q_seq=5 * H, k_seq=7 * H, v_seq=7 * H, o_seq=5 * H,
             q_elems=10 * H, k_elems=14 * H, v_elems=14 * H, o_elems=10 * H, q_bound=1.0, k_bound=1.0, v_bound=1.0)
    d.update(kw)
    return _lib.Attn3Case(**d)


def _ragged_case(lens=(3, 5), slots=(2, 0), **kw):
    H = 128
    lens, slots = np.asarray(lens, np.int32), np.asarray(slots, np.int32)
    d = dict(n_seq=len(lens), n_heads=2, Q=FAKE, K=FAKE, V=FAKE, O=FAKE, ldq=H, ldo=H, q_elems=9 * H, o_elems=9 * H, k_elems=3 * 2 * 8 * 64, v_elems=3 * 2 * 8 * 64,
             q_bound=1.0, k_bound=1.0, v_bound=1.0, seq_len=lens.ctypes.data, slot_of_seq=slots.ctypes.data, slot_stride=2 * 8 * 64, max_ctx=8, n_slots=3, row0=1)
    d.update(kw)
    c = _lib.Attn3Case(**d)
    c._keep = (lens, slots)
    return c


REFUSED3 = {
    "q rows past q_elems": lambda: _strided_case(q_elems=10 * 128 - 1),
    "k rows past k_elems": lambda: _strided_case(k_elems=14 * 128 - 1),
    "v row stride past v_elems": lambda: _strided_case(ldv=384, v_seq=7 * 384),
    "o rows past o_elems": lambda: _strided_case(o_elems=10 * 128 - 1),
    "overlapping o sequences": lambda: _strided_case(o_seq=4 * 128),
    "ld below the row": lambda: _strided_case(ldk=64),
    "ld no multiple of 4": lambda: _strided_case(ldq=130, q_elems=10 ** 6),
    "sequence stride no multiple of 4": lambda: _strided_case(k_seq=7 * 128 + 2, k_elems=10 ** 6),
    "misaligned pointer": lambda: _strided_case(K=FAKE + 4),
    "null pointer": lambda: _strided_case(O=None),
    "no keys": lambda: _strided_case(Sk=0),
    "nan bound": lambda: _strided_case(k_bound=float("nan")),
    "wrong struct size": lambda: _strided_case(),
    "ragged: prompt longer than max_ctx": lambda: _ragged_case(lens=(3, 9), q_elems=10 ** 6, o_elems=10 ** 6),
    "ragged: empty prompt": lambda: _ragged_case(lens=(0, 5)),
    "ragged: slot outside n_slots": lambda: _ragged_case(slots=(3, 0)),
    "ragged: cache smaller than n_slots": lambda: _ragged_case(k_elems=3 * 2 * 8 * 64 - 1),
    "ragged: slot stride below a slot": lambda: _ragged_case(slot_stride=2 * 8 * 64 - 4),
    "ragged: rows past q_elems": lambda: _ragged_case(q_elems=9 * 128 - 1),
    "ragged: rows past o_elems": lambda: _ragged_case(o_elems=9 * 128 - 1),
    "ragged: negative row0": lambda: _ragged_case(row0=-1),
    "ragged: no slots given": lambda: _ragged_case(slot_of_seq=None),
}


@pytest.mark.parametrize("name", list(REFUSED3))
def test_attn3_case_refuses_what_would_leave_the_stated_sizes(name):
    c = REFUSED3[name]()
    if name == "wrong struct size":
        c.struct_bytes = 8
    assert _lib.lib().etd_debug_attn3_case(C.byref(c), None) == -22, name
    assert b"debug_attn3_case" in _lib.lib().etd_last_error()


def test_scale_log2_is_the_librarys():
    """the hook reports its plane scales as soon as the bounds are accepted, also for a case it then refuses: g3_scale_log2 without a GPU"""
    out = np.zeros(3, np.int32)
    rng = np.random.default_rng(2)
    bounds = list(np.exp(rng.uniform(-20, 20, 60)).astype(np.float32)) + [2.0 ** e for e in range(-8, 9)] + [np.nextafter(np.float32(4.0), np.float32(0)), 0.0, 3.99964]
    for b in bounds:
        c = _strided_case(q_bound=float(b), k_bound=float(b) * 8, v_bound=float(b) * 64, o_elems=1, log2_out3=out.ctypes.data)
        assert _lib.lib().etd_debug_attn3_case(C.byref(c), None) == -22
        assert tuple(out) == tuple(A.scale_log2(np.float32(b) * np.float32(m)) for m in (1, 8, 64)), b
        if b > 0:
            assert float(b) * 2.0 ** float(out[0]) < 2.0 ** 15 <= float(b) * 2.0 ** float(out[0] + 2)


def _dattn(M=3, nh=2, n_slots=4, max_ctx=64, slots=(0, 1, 2), pos=(0, 5, 99), form=0, q=FAKE, kc=FAKE, vc=FAKE, o=FAKE, qo=None, kv=None):
    slots, pos = np.asarray(slots, np.int32), np.asarray(pos, np.int32)
    qo = M * nh * 64 if qo is None else qo
    kv = n_slots * nh * max_ctx * 64 if kv is None else kv
    return _lib.lib().etd_debug_dattn_f32(q, kc, vc, o, qo, kv, M, nh, n_slots, max_ctx, slots.ctypes.data, pos.ctypes.data, form, None)


@pytest.mark.parametrize("kw", [dict(qo=3 * 128 - 1), dict(kv=4 * 2 * 64 * 64 - 1), dict(slots=(0, 1, 4)), dict(slots=(0, -1, 2)), dict(pos=(0, -1, 3)), dict(form=3),
                                dict(form=2, slots=(0, 2, 1)), dict(form=2, max_ctx=63), dict(o=FAKE + 8), dict(kc=None), dict(M=0, slots=(), pos=())],
                         ids=["q/o short", "cache short", "slot past n_slots", "negative slot", "negative pos", "unknown form", "identity with permuted slots",
                              "identity below 64 positions", "misaligned o", "null cache", "no rows"])
def test_dattn_hook_refuses(kw):
    assert _dattn(**kw) == -22
    assert b"debug_dattn_f32" in _lib.lib().etd_last_error()
