"""numpy restatement of the exact-parity attention (csrc/gemm3.hip `k_attn3`, csrc/dec_kernels.hip `k_dattn<float>`) and the inputs its tests run on.

    ref64      float64 softmax(q k^T / 8) v per (sequence, head) -- the truth every figure is measured against
    split_emu  the same operation with k_attn3's OPERAND rounding (hi / lo f16 planes at the scales in use, three products per term, P carried at 2^15) and every
               sum in float64: what the plane arithmetic itself predicts at those scales, without the kernel's fp32 accumulation
    fp32_cpu   torch's CPU scaled_dot_product_attention in float32: the project's yardstick for "fp32 grade"
    err        the figure: per head max|o - ref64| / max|v| of that head, worst head
    bound      3 max(e_fp32cpu, e_split) + 8 * 2^-24: the 3 x fp32-torch rule of tests/test_gpu_gemm3.py next to what the planes predict, and a floor for the fp32
               rounding of the output and of its final normalisation (2^-24 each on values up to max|v|, with room for the reciprocal and the rescaled running sums)

A whole-tensor figure under sigma = 4 scores hides a mask that slips by one key: the slipped key usually carries next to no weight.  The fixtures therefore give
every sequence EDGE QUERIES (first / last query, the queries on either side of every 32-query wave edge counted from the front and -- ragged tiles are aligned to
the end of a prompt -- from the back) and turn each of them towards its edge keys: the last key it may see and, causal, the first one it may not, both at the
row's maximum score; those keys carry V rows of constant magnitude 2.5 unlike any random row.  `mutant` restates two slips:
    "many"  one key too many: causal `key <= qi + 1`; where no further key exists (strided, or the last query of a prompt) the last real key counts twice --
            exactly what k_attn3's clamped tile rows and k_dattn's clamped requests would deliver if a `key < Sk` mask slipped
    "few"   the last visible key dropped (no key left: zeros)
and tests/test_attn3_np_cpu.py requires each to exceed the fixture's bound 10 x at every edge query.  One slip cannot be seen by any input: a single visible key
counted twice is softmax over two equal scores of two equal V rows, the same output (`mutant_is_identity`)."""
import functools

import numpy as np
import torch

FLOOR = 8.0 * 2.0 ** -24
WAVE_EDGES = (0, 1, 31, 32, 63, 64, 95, 96, 127, 128, 191, 192)


# ---------------------------------------------------------------------------------------------------------------------------------------- the operation
def _heads(x):
    """[S][heads * 64] -> [heads][S][64]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], -1, 64).transpose(1, 0, 2))


def _softmax_v(sc, v, causal, mut=None):
    """rows of softmax(sc) v in float64; sc [Sq][Sk] scores (already / 8), query t of a causal call is the prompt's position t"""
    Sq, Sk = sc.shape
    key, qi = np.arange(Sk)[None, :], np.arange(Sq)[:, None]
    last = np.minimum(qi, Sk - 1) if causal else np.full((Sq, 1), Sk - 1)          # last visible key of each query
    w = (key <= last).astype(np.float64)                                         # multiplicity of each key in the sums
    if mut == "many":
        nxt = last + 1
        w = w + (key == np.minimum(nxt, Sk - 1))                                  # the next key; none left: the last real key a second time
    elif mut == "few":
        w = w - (key == last)
    elif mut is not None:
        raise ValueError(mut)
    m = np.where(w > 0, sc, -np.inf).max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.where(w > 0, np.exp(np.where(w > 0, sc - m, 0.0)), 0.0) * w
    den = p.sum(-1, keepdims=True)
    return np.where(den > 0, (p @ v) / np.where(den > 0, den, 1.0), 0.0)


def ref64(q, k, v, causal=False, mut=None):
    """q [Sq][H], k / v [Sk][H] (one sequence) -> float64 [Sq][H]; causal: Sq == Sk, query t sees keys 0 .. t"""
    q, k, v = (_heads(np.asarray(a, np.float64)) for a in (q, k, v))
    o = [_softmax_v(q[h] @ k[h].T / 8.0, v[h], causal, mut) for h in range(q.shape[0])]
    return np.stack(o, 1).reshape(q.shape[1], -1)


def scale_log2(bound):
    """g3_scale_log2 (csrc/gemm3.hip): log2 of the power of two that keeps |s x| < 2^15 for |x| <= bound"""
    b = np.float32(bound)
    if not (b > 0) or not np.isfinite(b):
        return 0
    return 15 - int(np.frexp(np.float32(b * np.float32(1.0001)))[1])


def _split(x, log2):
    """t = fp32(2^log2 x), hi = f16(t), lo = f16(t - hi) (np.float16: round to nearest even, subnormals kept -- as the planes) -> float64 hi, lo"""
    with np.errstate(over="ignore"):
        t = (np.asarray(x, np.float32) * np.float32(2.0 ** log2)).astype(np.float32)
        hi = t.astype(np.float16)
        lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def split_emu(q, k, v, q_log2, k_log2, v_log2, causal=False):
    """k_attn3's operand rounding with float64 sums (see the module text); same shapes as ref64"""
    (qh, ql), (kh, kl), (vh, vl) = (tuple(_heads(p) for p in _split(a, l2)) for a, l2 in ((q, q_log2), (k, k_log2), (v, v_log2)))
    nh, Sq, Sk = qh.shape[0], qh.shape[1], kh.shape[1]
    out = np.zeros((Sq, nh, 64))
    vis = np.arange(Sk)[None, :] <= (np.arange(Sq)[:, None] if causal else Sk - 1)
    for h in range(nh):
        s = (qh[h] @ kh[h].T + qh[h] @ kl[h].T + ql[h] @ kh[h].T) * 2.0 ** -(q_log2 + k_log2) / 8.0          # hi hi + hi lo + lo hi, in score units
        s = np.where(vis, s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)                # P in [0, 1], fp32 as the kernel holds it
        ph, pl = _split(p, 15)
        o = ph @ vh[h] + ph @ vl[h] + pl @ vh[h]
        out[:, h] = o / p.astype(np.float64).sum(-1, keepdims=True) * 2.0 ** -(15 + v_log2)
    return out.reshape(Sq, nh * 64)


def fp32_cpu(q, k, v, causal=False):
    """torch CPU scaled_dot_product_attention, float32"""
    t = [torch.from_numpy(_heads(np.asarray(a, np.float32)))[None] for a in (q, k, v)]
    o = torch.nn.functional.scaled_dot_product_attention(*t, is_causal=bool(causal))[0]
    return o.transpose(0, 1).reshape(o.shape[1], -1).numpy()


def err(o, ref, v, rows=None):
    """worst head's max|o - ref| / max|v| (o, ref [Sq][H]; v [Sk][H]); rows: only these queries"""
    d = np.abs(np.asarray(o, np.float64) - ref)
    if rows is not None:
        d = d[np.asarray(rows)]
    d = d.reshape(d.shape[0], -1, 64).max((0, 2))
    vm = np.abs(np.asarray(v, np.float64)).reshape(v.shape[0], -1, 64).max((0, 2))
    return float((d / vm).max())


def bound(e_fp32cpu, e_split):
    return 3.0 * max(e_fp32cpu, e_split) + FLOOR


def mutant_is_identity(mut, Sk):
    """a single visible key counted twice gives the same output: no input shows that slip"""
    return mut == "many" and Sk == 1


# ---------------------------------------------------------------------------------------------------------------------------------------- fixtures
def edge_queries(Sq, causal):
    """queries on either side of every wave edge from the front, and (causal: tiles are aligned to the prompt's end) from the back"""
    e = {t for t in WAVE_EDGES if t < Sq} | {Sq - 1}
    if causal:
        e |= {Sq - d for d in (32, 33, 64, 65, 96, 97, 128, 129) if Sq - d >= 0}
    return sorted(e)


def _edge_v(rng):
    return (2.5 * rng.choice([-1.0, 1.0], 64)).astype(np.float32)


def _turn(q, keys, others):
    """q (64,) + a combination of `keys` (rows) so that its score with each of them equals the largest score q has with `others` (none: 0)"""
    q, keys = q.astype(np.float64), keys.astype(np.float64)
    c = float((others.astype(np.float64) @ q).max() / 8.0) if len(others) else 0.0
    d = np.linalg.solve(keys @ keys.T, 8.0 * c - keys @ q)
    return (q + d @ keys).astype(np.float32)


def _make(Sq, Sk, nh, causal, seed, spread=False):
    rng = np.random.default_rng(seed)
    H = nh * 64
    q = (rng.standard_normal((Sq, H)) * 2.0).astype(np.float32)
    k = (rng.standard_normal((Sk, H)) * 2.0).astype(np.float32)                   # scores with sigma 4: a softmax with real contrast
    v = rng.standard_normal((Sk, H)).astype(np.float32)
    if spread:                                                                   # rows of very different magnitude (test_gemm3_has_the_error_of_an_fp32_product)
        q *= np.exp(rng.uniform(-3, 1, (Sq, 1))).astype(np.float32)
        k *= np.exp(rng.uniform(-3, 1, (Sk, 1))).astype(np.float32)
        v *= np.exp(rng.uniform(-3, 1, (Sk, 1))).astype(np.float32)
    edges = edge_queries(Sq, causal)
    ekeys = sorted({min(t + d, Sk - 1) for t in edges for d in (0, 1)}) if causal else [Sk - 1]
    for h in range(nh):
        c = slice(h * 64, (h + 1) * 64)
        for ke in ekeys:
            v[ke, c] = _edge_v(rng)
        for t in edges:
            mine = sorted({min(t, Sk - 1), min(t + 1, Sk - 1)}) if causal else [Sk - 1]
            rest = [j for j in range(min(t + 1, Sk) if causal else Sk) if j not in mine]
            q[t, c] = _turn(q[t, c], k[mine][:, c], k[rest][:, c])
    return dict(q=q, k=k, v=v, edges=edges, causal=causal, Sq=Sq, Sk=Sk, nh=nh)


@functools.lru_cache(maxsize=None)
def strided(Sq, Sk, nh=2, n_seq=2, spread=False):
    """n_seq independent sequences of Sq queries x Sk keys: list of fixtures"""
    return [_make(Sq, Sk, nh, False, 1000 * Sq + 7 * Sk + 100003 * s + nh, spread) for s in range(n_seq)]


@functools.lru_cache(maxsize=None)
def prompt(L, nh=2):
    """one causal prompt of L rows; the same (L, nh) is the same data alone and in every batch"""
    return _make(L, L, nh, True, 77000 + 13 * L + nh)


@functools.lru_cache(maxsize=None)
def decode_row(ctx, nh=2):
    """the decode step's row at context ctx: the LAST query of a prompt of ctx rows against all its keys"""
    f = prompt(ctx, nh)
    return dict(q=f["q"][-1:], k=f["k"], v=f["v"], edges=[0], causal=False, Sq=1, Sk=ctx, nh=nh)


@functools.lru_cache(maxsize=None)
def yardsticks(kind, *key, mult=(1, 1, 1)):
    """per fixture of a case: (ref64, e_fp32cpu, e_split, log2 scales) -- computed once, shared by the CPU and the device tests.  The plane scales of a case are
    those of mult x the largest |q|, |k|, |v| over ALL its fixtures, as one launch has one scale per operand."""
    fx = fixtures(kind, *key)
    l2 = case_log2(scale_scope(kind, *key), mult)
    out = []
    for f in fx:
        r = ref64(f["q"], f["k"], f["v"], f["causal"])
        e32 = err(fp32_cpu(f["q"], f["k"], f["v"], f["causal"]), r, f["v"])
        es = err(split_emu(f["q"], f["k"], f["v"], *l2, causal=f["causal"]), r, f["v"])
        out.append((r, e32, es))
    return out, l2


def fixtures(kind, *key):
    if kind == "strided":
        return strided(*key)
    if kind == "ragged":
        lens, nh = key
        return [prompt(L, nh) for L in lens]
    if kind == "decode":
        ctxs, nh = key
        return [decode_row(c, nh) for c in ctxs]
    raise ValueError(kind)


def scale_scope(kind, *key):
    """the fixtures a case's bounds are taken over.  Ragged: every prompt length of that head count, so that a prompt alone and inside any batch is split at the
    same scales -- its rows are then compared bit for bit"""
    if kind == "ragged":
        return [prompt(L, key[1]) for L in sorted(set(RAGGED_SINGLES) | set(key[0]))]
    return fixtures(kind, *key)


def case_bounds(fx, mult=(1, 1, 1)):
    return tuple(float(m) * max(float(np.abs(f[x]).max()) for f in fx) for m, x in zip(mult, "qkv"))


def case_log2(fx, mult=(1, 1, 1)):
    return tuple(scale_log2(b) for b in case_bounds(fx, mult))


# ---------------------------------------------------------------------------------------------------------------------------------------- the cases
SQ = (1, 31, 32, 33, 63, 64, 65, 88, 96, 97, 127, 128, 129)
SK_TAIL, SK_FULL = (1, 63, 65, 88, 129), (64, 256)


def _pairs():
    p = []
    for i, sq in enumerate(SQ):                                                  # every Sq with a key tail and without one
        p += [(sq, SK_TAIL[i % 5]), (sq, SK_FULL[i % 2])]
    p += [(sq, sk) for sq in (65, 88, 96) for sk in (1, 65, 256)]                # the three-wave launch against one key, a tail and four full tiles
    return sorted(set(p))


STRIDED_PAIRS = _pairs()                                                         # 33 of the 91 pairs
LOOSE = [m for f in (8, 64) for m in ((f, 1, 1), (1, f, 1), (1, 1, f))]           # a provable bound is 8 x .. 64 x the data's maximum, on each operand in turn
LOOSE_PAIRS = ((88, 256), (129, 65))
LAYOUTS = (("qkv", (88, 88)), ("qkv", (65, 65)), ("qkv", (129, 129)), ("cross", (88, 256)), ("wide_o", (97, 129)), ("wide_o", (88, 65)))
RAGGED_SINGLES = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193)
RAGGED_BATCHES = {                                                               # name -> (lens, heads)
    "three_waves": ((33, 1, 96, 64, 2), 2),                                     # max_len 96: 192 threads, qpw 96
    "flip_97": ((97, 31, 65, 32, 96), 2),                                       # max_len 97: four waves again; 65 and 96 alone take three
    "long": ((193, 127, 63, 129, 95, 128, 191, 192), 2),
    "heads8": ((65, 96, 1, 33), 8),
}
DECODE_CTX = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
DECODE_MAX_CTX = 260                                                             # one more row asks for a position past it: the clamp


def all_cases():
    """(id, kind, key, mult) of every fixture set the device tests run: what tests/test_attn3_np_cpu.py pins without a GPU"""
    c = [("strided-%dx%d" % p, "strided", p, (1, 1, 1)) for p in STRIDED_PAIRS]
    c += [("strided-%dx%d-bounds%dx%dx%d" % (p + m), "strided", p, m) for p in LOOSE_PAIRS for m in LOOSE]
    c += [("strided-%dx%d" % p, "strided", p, (1, 1, 1)) for p in sorted({p for _, p in LAYOUTS} - set(STRIDED_PAIRS))]
    c += [("strided-spread", "strided", (129, 129, 2, 2, True), (1, 1, 1)), ("strided-heads8", "strided", (97, 129, 8, 2), (1, 1, 1))]
    c += [("ragged-singles", "ragged", (RAGGED_SINGLES, 2), (1, 1, 1))]
    c += [("ragged-" + n, "ragged", b, (1, 1, 1)) for n, b in RAGGED_BATCHES.items() if b[1] != 2]
    c += [("decode", "decode", (DECODE_CTX + (DECODE_MAX_CTX,), 2), (1, 1, 1))]
    return c
