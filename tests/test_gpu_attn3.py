"""The exact-parity attention kernels on the device against float64, at every tile, mask and layout edge production reaches: `k_attn3` (strided: the fp32 extractor;
ragged causal: the decoder's fp32 prefill) through etd_debug_attn3_case, `k_dattn<float>` (the fp32 decode step) through etd_debug_dattn_f32.

Figure and bound are tests/attn3_np.py's: per (sequence, head) max|o - ref64| / max|v|, held to 3 max(e_fp32cpu, e_split) + 8 * 2^-24 for k_attn3 and to
3 e_fp32cpu + 8 * 2^-24 for k_dattn<float> (plain fp32 with expf).  The inputs carry edge keys, so a mask that slips by one key at a tile edge moves the figure by
four orders of magnitude (tests/test_attn3_np_cpu.py proves that of every fixture without a GPU).  Memory the kernels must not read holds NaN, memory they must not
write holds a pattern that has to come back bit for bit.  Every figure is printed; with ETD_ATTN3_REPORT=dir they are also kept as JSON (how
profiles/attn3_device.json is made; summary in DESIGN.md next to the gemm3 section)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import attn3_np as A
from etude_amd import _lib

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def report(name, rows):
    for r in rows:
        print(name, r)
    out = os.environ.get("ETD_ATTN3_REPORT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(rows, f, indent=1)


def _pattern(shape, seed):
    """finite floats of no particular value: what must come back bit for bit"""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * 1e3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _row(case, seq, f, o, ref, e32, es, l2, mult=(1, 1, 1), split=True):
    e = A.err(o, ref, f["v"])
    b = A.bound(e32, es if split else 0.0)
    return dict(case=case, seq=seq, heads=f["nh"], Sq=f["Sq"], Sk=f["Sk"], bounds_x=list(mult), log2=list(l2) if split else None, e_dev=e, e_fp32cpu=e32,
                e_split=es if split else None, bound=b, dev_over_fp32=(e / e32 if e32 > 0 else None), held=bool(e <= b))


def _check(name, rows):
    report(name, rows)
    bad = [r for r in rows if not r["held"]]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------------- k_attn3, strided
def run_strided(fx, mult=(1, 1, 1), layout="contiguous"):
    """one launch over the sequences of fx -> o [n][Sq][H]"""
    n, nh, Sq, Sk = len(fx), fx[0]["nh"], fx[0]["Sq"], fx[0]["Sk"]
    H = nh * 64
    q, k, v = (np.stack([f[x] for f in fx]) for x in "qkv")
    c = _lib.Attn3Case(n_seq=n, n_heads=nh, Sq=Sq, Sk=Sk)
    c.q_bound, c.k_bound, c.v_bound = A.case_bounds(fx, mult)
    keep = []
    if layout == "qkv":                                                          # the extractor's self attention: one [rows][3 H] buffer, Q | K | V at 0, H, 2 H
        assert Sq == Sk
        buf = _to(np.concatenate([q, k, v], -1))
        keep.append(buf)
        for i, x in enumerate("qkv"):
            setattr(c, x.upper(), buf.data_ptr() + 4 * i * H); setattr(c, "ld" + x, 3 * H); setattr(c, x + "_seq", Sq * 3 * H); setattr(c, x + "_elems", buf.numel() - i * H)
    else:
        qd = _to(q)
        keep.append(qd)
        c.Q, c.ldq, c.q_seq, c.q_elems = qd.data_ptr(), H, Sq * H, qd.numel()
        if layout == "cross":                                                    # the extractor's cross attention: Sq != Sk, K | V interleaved in a buffer of their own
            buf = _to(np.concatenate([k, v], -1))
            keep.append(buf)
            for i, x in enumerate("kv"):
                setattr(c, x.upper(), buf.data_ptr() + 4 * i * H); setattr(c, "ld" + x, 2 * H); setattr(c, x + "_seq", Sk * 2 * H); setattr(c, x + "_elems", buf.numel() - i * H)
        else:
            kd, vd = _to(k), _to(v)
            keep += [kd, vd]
            c.K, c.ldk, c.k_seq, c.k_elems = kd.data_ptr(), H, Sk * H, kd.numel()
            c.V, c.ldv, c.v_seq, c.v_elems = vd.data_ptr(), H, Sk * H, vd.numel()
    ldo, extra = (H + 64, 3) if layout == "wide_o" else (H, 0)                   # wide_o: columns past H and rows past Sq belong to somebody else
    o0 = _pattern((n, Sq + extra, ldo), 5)
    o0[:, :Sq, :H] = np.nan
    od = _to(o0)
    c.O, c.ldo, c.o_seq, c.o_elems = od.data_ptr(), ldo, (Sq + extra) * ldo, od.numel()
    l2 = np.zeros(3, np.int32)
    c.log2_out3 = l2.ctypes.data
    _lib.check(_lib.lib().etd_debug_attn3_case(C.byref(c), _stream()), "etd_debug_attn3_case")
    assert tuple(l2) == A.case_log2(fx, mult)
    full = od.cpu().numpy()
    o = full[:, :Sq, :H].copy()
    assert np.isfinite(o).all()
    full[:, :Sq, :H] = 0
    o0[:, :Sq, :H] = 0
    assert np.array_equal(_bits(full), _bits(o0)), "the kernel wrote outside its rows"
    return o


def strided_rows(case, key, mult=(1, 1, 1), layout="contiguous"):
    fx = A.fixtures("strided", *key)
    ys, l2 = A.yardsticks("strided", *key, mult=mult)
    o = run_strided(fx, mult, layout)
    return [_row(case, s, f, o[s], r, e32, es, l2, mult) for s, (f, (r, e32, es)) in enumerate(zip(fx, ys))]


@pytest.mark.parametrize("Sq,Sk", A.STRIDED_PAIRS)
def test_strided_tile_and_tail_edges(Sq, Sk):
    _check("strided_%dx%d" % (Sq, Sk), strided_rows("strided", (Sq, Sk)))


@pytest.mark.parametrize("layout,pair", A.LAYOUTS)
def test_strided_layouts_of_the_extractor(layout, pair):
    rows = strided_rows(layout, pair, layout=layout)
    _check("layout_%s_%dx%d" % ((layout,) + pair), rows)
    plain = run_strided(A.fixtures("strided", *pair))                            # strides change addresses, never arithmetic
    assert np.array_equal(_bits(plain), _bits(run_strided(A.fixtures("strided", *pair), layout=layout)))


def test_strided_eight_heads():
    _check("strided_heads8", strided_rows("heads8", (97, 129, 8, 2)))


def test_strided_rows_of_very_different_magnitude():
    _check("strided_spread", strided_rows("spread", (129, 129, 2, 2, True)))


@pytest.mark.parametrize("pair", A.LOOSE_PAIRS)
def test_strided_plane_scales_from_loose_bounds(pair):
    """bounds 8 x and 64 x the data's maximum on each operand in turn: what production's provable bounds cost (the 64 x rows are kept apart)"""
    tight = strided_rows("bounds", pair)
    rows = [r for m in A.LOOSE for r in strided_rows("bounds", pair, mult=m)]
    for r in rows:
        r["dev_over_tight"] = r["e_dev"] / tight[r["seq"]]["e_dev"]
    report("bounds64_%dx%d" % pair, [r for r in rows if 64 in r["bounds_x"]])
    _check("bounds_%dx%d" % pair, tight + rows)


# ---------------------------------------------------------------------------------------------------------------------------------------- k_attn3, ragged causal
def run_ragged(lens, nh, slots, n_slots, row0):
    """one launch over prompts A.prompt(L, nh) in the given slots of a NaN-filled cache -> list of o [L][H]"""
    fx = [A.prompt(L, nh) for L in lens]
    H, M, max_ctx, tail = nh * 64, int(sum(lens)), max(lens) + 37, 3
    q = np.full((row0 + M + tail, H), np.nan, np.float32)                        # rows of other calls: not this launch's to read
    o0 = _pattern((row0 + M + tail, H), 6)
    o0[row0:row0 + M] = np.nan
    kc = np.full((n_slots, nh, max_ctx, 64), np.nan, np.float32)                 # hipMalloc clears nothing: positions past a prompt and unused slots hold anything
    vc = kc.copy()
    r = row0
    for f, L, s in zip(fx, lens, slots):
        q[r:r + L] = f["q"]
        kc[s, :, :L], vc[s, :, :L] = A._heads(f["k"]), A._heads(f["v"])
        r += L
    qd, kd, vd, od = _to(q), _to(kc), _to(vc), _to(o0)
    lens32, slots32, l2 = np.asarray(lens, np.int32), np.asarray(slots, np.int32), np.zeros(3, np.int32)
    c = _lib.Attn3Case(n_seq=len(lens), n_heads=nh, Q=qd.data_ptr(), q_elems=qd.numel(), ldq=H, K=kd.data_ptr(), k_elems=kd.numel(), V=vd.data_ptr(), v_elems=vd.numel(),
                       O=od.data_ptr(), o_elems=od.numel(), ldo=H, seq_len=lens32.ctypes.data, slot_of_seq=slots32.ctypes.data, slot_stride=nh * max_ctx * 64,
                       max_ctx=max_ctx, n_slots=n_slots, row0=row0, log2_out3=l2.ctypes.data)
    c.q_bound, c.k_bound, c.v_bound = A.case_bounds(A.scale_scope("ragged", tuple(lens), nh))
    _lib.check(_lib.lib().etd_debug_attn3_case(C.byref(c), _stream()), "etd_debug_attn3_case")
    assert tuple(l2) == A.case_log2(A.scale_scope("ragged", tuple(lens), nh))
    full = od.cpu().numpy()
    assert np.isfinite(full[row0:row0 + M]).all(), "a NaN of the cache or of a neighbouring row reached the output"
    assert np.array_equal(_bits(full[:row0]), _bits(o0[:row0])) and np.array_equal(_bits(full[row0 + M:]), _bits(o0[row0 + M:])), "the kernel wrote outside its rows"
    out, r = [], row0
    for L in lens:
        out.append(full[r:r + L].copy())
        r += L
    return out


@functools.lru_cache(maxsize=None)
def ragged_alone(L, nh):
    return run_ragged((L,), nh, (2,), 3, 5)[0]


def ragged_rows(case, lens, nh, outs):
    ys, l2 = A.yardsticks("ragged", tuple(lens), nh)
    return [_row(case, s, A.prompt(L, nh), o, r, e32, es, l2) for s, (L, o, (r, e32, es)) in enumerate(zip(lens, outs, ys))]


@pytest.mark.parametrize("L", A.RAGGED_SINGLES)
def test_ragged_prompt_alone(L):
    _check("ragged_alone_%d" % L, ragged_rows("alone", (L,), 2, [ragged_alone(L, 2)]))


@pytest.mark.parametrize("name", list(A.RAGGED_BATCHES))
def test_ragged_batch_and_its_prompts_alone_bit_for_bit(name):
    """fp32 logits do not depend on the batch shape: a prompt's rows are the same bits alone (slot 2, row0 5, the launch width its own length picks) and inside a
    batch (another slot, another row0, the width the longest prompt picks)"""
    lens, nh = A.RAGGED_BATCHES[name]
    n = len(lens)
    outs = run_ragged(lens, nh, tuple(n + 1 - s for s in range(n)), n + 2, 3)      # slots n + 1 .. 2: a permutation that is not the identity, slots 0 and 1 unused
    _check("ragged_" + name, ragged_rows(name, lens, nh, outs))
    for L, o in zip(lens, outs):
        assert np.array_equal(_bits(o), _bits(ragged_alone(L, nh))), (name, L)


# ---------------------------------------------------------------------------------------------------------------------------------------- k_dattn<float>
DEC_ROWS = tuple((c, c - 1) for c in A.DECODE_CTX) + ((A.DECODE_MAX_CTX, A.DECODE_MAX_CTX + 5),)       # (context the row must see, position it asks for: the last one past max_ctx)


@functools.lru_cache(maxsize=None)
def run_decode(form, nh=2):
    M, H, mc = len(DEC_ROWS), nh * 64, A.DECODE_MAX_CTX
    n_slots = M + 2
    slots = np.arange(M, dtype=np.int32) if form == 2 else (M + 1 - np.arange(M)).astype(np.int32)
    fx = [A.decode_row(c, nh) for c, _ in DEC_ROWS]
    kc = np.full((n_slots, nh, mc, 64), np.nan, np.float32)
    vc = kc.copy()
    for f, s in zip(fx, slots):
        kc[s, :, :f["Sk"]], vc[s, :, :f["Sk"]] = A._heads(f["k"]), A._heads(f["v"])
    qd, kd, vd = _to(np.concatenate([f["q"] for f in fx])), _to(kc), _to(vc)
    od = torch.full((M, H), float("nan"), dtype=torch.float32, device=_dev())
    pos = np.asarray([p for _, p in DEC_ROWS], np.int32)
    _lib.check(_lib.lib().etd_debug_dattn_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), qd.numel(), kd.numel(), M, nh, n_slots, mc, slots.ctypes.data,
                                              pos.ctypes.data, form, _stream()), "etd_debug_dattn_f32")
    o = od.cpu().numpy()
    assert np.isfinite(o).all(), "a NaN past a context reached the output"
    return o


@pytest.mark.parametrize("form", [0, 1, 2], ids=["rows", "pairs", "identity"])
def test_decode_step_attention_at_every_context_edge(form):
    o = run_decode(form)
    ys, _ = A.yardsticks("decode", tuple(c for c, _ in DEC_ROWS), 2)
    rows = [_row("decode_form%d" % form, i, A.decode_row(c, 2), o[i:i + 1], r, e32, es, None, split=False) for i, ((c, _), (r, e32, es)) in enumerate(zip(DEC_ROWS, ys))]
    _check("decode_form%d" % form, rows)


def test_decode_step_addressing_forms_agree_bit_for_bit():
    assert np.array_equal(_bits(run_decode(0)), _bits(run_decode(1))) and np.array_equal(_bits(run_decode(0)), _bits(run_decode(2)))
