"""Every row and elementwise kernel of the decoder trainer (csrc/dec_train.hip) on its own input, through the stage taps of
include/etude_hip_debug.h -- each tap runs the launcher (kernel, grid, block) that etd_dtrain_forward_backward / etd_dtrain_clip_and_step run.

The yardstick is tests/test_gpu_train.py's, unchanged: ``err = max|dev - y64| / max|y64|`` per tensor against torch on the CPU in fp64 (tests/train_stage_np.py:
``F.layer_norm``, ``F.gelu``, ``F.cross_entropy``, ``F.embedding``, oracle/neox.py's rotary function, autograd for every backward), held to 4 x the same figure of
the same reference in fp32, with a floor of 4 * 2^-24.  Stages that only move or add in a fixed order are held bit for bit against fp32 numpy in that order.  The
optimizer is held per tensor to ``max(4 x the fp32 restatement's error, 1 ulp of the tensor's largest magnitude)`` (test_clip_and_step_against_the_restatement's
bound), the gradient norm to ``n * 2^-52`` relative against numpy longdouble: the squares are exact in fp64 and only the n additions round.
Every output sits between guard floats (tests/_util.py): nothing outside is written, every float inside is.  Every figure is printed before the first failure, and
kept under ETD_TRAIN_REPORT (how the stage figures of profiles/train_device.json are made).
"""
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_np as tn  # noqa: E402
import train_stage_np as ts  # noqa: E402
from _util import Guarded  # noqa: E402

from etude_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
EPS = 1e-5
OPT = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
_rows, _bad = [], []


def _rel(y, y64):
    return float((torch.as_tensor(y).to(F64) - y64).abs().max()) / float(y64.abs().max())


def _hold(what, dev, y32, y64, **tags):
    """record and print one figure; a violation is kept for _verdict so that every figure of the test is printed first"""
    dev, y32, y64 = torch.as_tensor(dev).reshape(-1), torch.as_tensor(y32).reshape(-1), torch.as_tensor(y64).reshape(-1)
    assert dev.shape == y64.shape, (what, tuple(dev.shape), tuple(y64.shape))
    assert bool(torch.isfinite(dev).all()), what
    if float(y64.abs().max()) == 0.0:                   # nothing to scale by: exact zeros
        e_dev, e_32 = float(dev.abs().max()), 0.0
        ok = e_dev == 0.0
    else:
        e_dev, e_32 = _rel(dev, y64), _rel(y32, y64)
        ok = e_dev <= max(4.0 * e_32, FLOOR)
    ratio = e_dev / max(e_32, 2.0 ** -24)
    print(f"DTRAIN_STAGE {what} {tags}: device {e_dev:.3e} yardstick {e_32:.3e} ratio {ratio:.2f}")
    _rows.append(dict(what=what, **tags, err_device=e_dev, err_fp32_cpu=e_32, ratio=ratio))
    if not ok:
        _bad.append((what, tags, e_dev, e_32))


def _note(what, **figures):
    print(f"DTRAIN_STAGE {what} {figures}")
    _rows.append(dict(what=what, **figures))


@pytest.fixture(autouse=True)
def _fresh():
    _rows.clear(); _bad.clear()
    yield
    _rows.clear(); _bad.clear()


def _verdict(name):
    out = os.environ.get("ETD_TRAIN_REPORT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(list(_rows), f, indent=1)
    bad = list(_bad)
    _bad.clear()
    assert not bad, bad


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _tap(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)
    torch.cuda.synchronize()


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("H", [1, 63, 64, 65, 256, 768])
def test_layer_norm_forward_and_backward(H, M):
    g = torch.Generator().manual_seed(1000 * H + M)
    x = torch.randn(M, H, generator=g)
    if M == 5:
        x[1] = 0.3                                                # variance 0: rstd = 1 / sqrt(eps)
        x[2] = 1e3 + torch.randn(H, generator=g)                  # the mean takes the leading bits of every element
    g1, b1, g2, b2 = (1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g), 1 + 0.1 * torch.randn(H, generator=g),
                      0.1 * torch.randn(H, generator=g))
    dy, dx0 = torch.randn(M, H, generator=g), torch.randn(M, H, generator=g)
    xd, g1d, b1d, g2d, b2d, dyd = (t.cuda() for t in (x, g1, b1, g2, b2, dy))

    def ref(dt):
        xx = x.to(dt)
        mean, rstd = ts.ln_stats(xx, EPS)
        return dict(y1=ts.ln_fwd(xx, g1.to(dt), b1.to(dt), EPS), y2=ts.ln_fwd(xx, g2.to(dt), b2.to(dt), EPS), mean=mean, rstd=rstd,
                    dx=dx0.to(dt) + ts.ln_bwd(xx, g1.to(dt), b1.to(dt), EPS, dy.to(dt))[0])
    r64, r32 = ref(F64), ref(F32)
    # the layer's first call: statistics and both outputs; the backward pass adds into a non-zero dx
    o = dict(y1=Guarded(M * H), y2=Guarded(M * H), mean=Guarded(M), rstd=Guarded(M), dx=Guarded(M * H, data=dx0))
    _tap("etd_debug_dtrain_ln", _p(xd), M, H, EPS, o["mean"].ptr, o["rstd"].ptr, _p(g1d), _p(b1d), o["y1"].ptr, _p(g2d), _p(b2d), o["y2"].ptr, _p(dyd), o["dx"].ptr)
    for k, buf in o.items():
        buf.check(f"ln {k}")
        _hold("ln_" + k, buf.floats(), r32[k], r64[k], H=H, M=M)
    # the final LayerNorm's call (statistics, one output) and the backward pass's recomputation (one output, no statistics): the same bits
    p = dict(y1=Guarded(M * H), mean=Guarded(M), rstd=Guarded(M))
    _tap("etd_debug_dtrain_ln", _p(xd), M, H, EPS, p["mean"].ptr, p["rstd"].ptr, _p(g1d), _p(b1d), p["y1"].ptr, None, None, None, None, None)
    q = Guarded(M * H)
    _tap("etd_debug_dtrain_ln", _p(xd), M, H, EPS, None, None, _p(g1d), _p(b1d), q.ptr, None, None, None, None, None)
    for k, buf in list(p.items()) + [("y1", q)]:
        buf.check(f"ln {k}")
        assert _same_bits(buf.floats(), o[k].floats()), k
    _verdict(f"stage_ln_H{H}_M{M}")


# ------------------------------------------------------------------ GELU, the residual sum
def _gelu_points(n, seed):
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))      # the fp32 neighbours of 0
    special = [0.7, 0.0, tiny, -tiny, 10.0, -10.0, 12.0, -12.0, -0.0]      # (at -10 the density underflows in fp32)
    grid = np.linspace(-12.0, 12.0, 193)
    rnd = 3.0 * np.random.default_rng(seed).standard_normal(max(n, 1))
    return torch.tensor(np.concatenate([special, grid, rnd])[:n].astype(np.float32))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_gelu_forward_and_backward(n):
    x = _gelu_points(n, n)
    dy = torch.randn(n, generator=torch.Generator().manual_seed(n))
    y, d, xd = Guarded(n), Guarded(n, data=dy), x.cuda()
    _tap("etd_debug_dtrain_gelu", _p(xd), n, y.ptr, d.ptr)
    y.check("gelu y"); d.check("gelu dy")
    _hold("gelu_y", y.floats(), ts.gelu_fwd(x), ts.gelu_fwd(x.to(F64)), n=n)
    _hold("gelu_dx", d.floats(), ts.gelu_bwd(x, dy), ts.gelu_bwd(x.to(F64), dy.to(F64)), n=n)
    # forward only: the backward pass is not run, dy's buffer is not needed
    y2 = Guarded(n)
    _tap("etd_debug_dtrain_gelu", _p(xd), n, y2.ptr, None)
    y2.check("gelu y alone")
    assert _same_bits(y2.floats(), y.floats())
    _verdict(f"stage_gelu_n{n}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_add3_is_the_parallel_residual_bit_for_bit(n):
    g = torch.Generator().manual_seed(n)
    m, a, h = (torch.randn(n, generator=g) * s for s in (1.0, 0.3, 10.0))
    out, md, ad, hd = Guarded(n), m.cuda(), a.cuda(), h.cuda()
    _tap("etd_debug_dtrain_add3", _p(md), _p(ad), _p(hd), n, out.ptr)
    out.check("add3")
    want = (m.numpy() + a.numpy()) + h.numpy()
    assert want.dtype == np.float32 and _same_bits(out.floats(), torch.from_numpy(want))


# ------------------------------------------------------------------ RoPE
@pytest.fixture(scope="module")
def handle_1024():
    """a trainer whose rotary table runs to position 1023 (the default decoder's), otherwise as small as the limits allow"""
    from etude_amd.train import DecoderTrainer
    cfg = tn.tiny_config(max_position_embeddings=1024, num_hidden_layers=1, vocab_size=11)
    tr = DecoderTrainer(cfg, tn.seeded_state(cfg, 1), max_rows=16)
    yield tr, tn.dims_of(cfg)
    tr.close()


@pytest.mark.parametrize("nh", [1, 4])
def test_rope_both_signs_to_position_1023(handle_1024, nh):
    tr, dims = handle_1024
    pos = np.random.default_rng(nh).permutation(np.array([0, 1, 255, 256, 1023] * 2))
    M = len(pos)
    x = torch.randn(M, nh * 192, generator=torch.Generator().manual_seed(nh))
    pos_d = torch.tensor(pos, dtype=torch.int32).cuda()
    untouched = torch.ones(M, nh, 3, 64, dtype=torch.bool)
    untouched[:, :, :2, :16] = False
    for sign in (1, -1):
        buf = Guarded(x.numel(), data=x)
        _tap("etd_debug_dtrain_rope", tr._h, buf.ptr, nh, M, _p(pos_d), sign)
        buf.check("rope")
        got = buf.floats().view(M, nh, 3, 64)
        assert _same_bits(got[untouched], x.view(M, nh, 3, 64)[untouched]), "dims 16..63 of q and k and all of v pass through"
        _hold("rope", got, ts.rope(x, pos, nh, dims, sign), ts.rope(x.to(F64), pos, nh, dims, sign), nh=nh, sign=sign)
        assert not _same_bits(got[:, :, :2, :16], x.view(M, nh, 3, 64)[:, :, :2, :16])
    # forward, then the inverse: the input again
    buf = Guarded(x.numel(), data=x)
    for sign in (1, -1):
        _tap("etd_debug_dtrain_rope", tr._h, buf.ptr, nh, M, _p(pos_d), sign)
    buf.check("rope round trip")
    rt = lambda t: ts.rope(ts.rope(t, pos, nh, dims, 1), pos, nh, dims, -1)      # noqa: E731
    assert _rel(rt(x.to(F64)), x.to(F64)) < 1e-7                 # (the fp32 cos / sin of the angle are not a rotation to more than fp32)
    _hold("rope_round_trip", buf.floats(), rt(x), x.to(F64), nh=nh)
    _verdict(f"stage_rope_nh{nh}")


def test_rope_refuses_a_position_past_the_table(handle_1024):
    tr, _ = handle_1024
    x = torch.zeros(2, 192, device="cuda")
    for bad in (1024, -1):
        pos = torch.tensor([0, bad], dtype=torch.int32).cuda()
        assert _lib.lib().etd_debug_dtrain_rope(tr._h, _p(x), 1, 2, _p(pos), 1, None) == -22
    assert _lib.lib().etd_debug_dtrain_rope(tr._h, _p(x), 1, 2, _p(pos), 0, None) == -22


# ------------------------------------------------------------------ embeddings, forward
@pytest.mark.parametrize("E", [1, 24, 64, 65])
def test_embed_gathers_and_sums_bit_for_bit(E):
    H, M, V, NC, NB = 256, 9, 157, 4, 5
    rng = np.random.default_rng(E)
    word, cemb = rng.standard_normal((V, H)).astype(np.float32), rng.standard_normal((NC, H)).astype(np.float32)
    tabs = [rng.standard_normal((NB, E)).astype(np.float32) for _ in range(4)]
    h_in = rng.standard_normal((M, H)).astype(np.float32)
    ids = np.array([0, V - 1, 5, 0, 156, 77, 1, V - 1, 100])            # the pad row (0) and the last row of every table
    cls = np.array([0, NC - 1, 1, 2, 0, NC - 1, 1, 2, 3])
    attrs4 = np.stack([np.roll(np.array([0, NB - 1, 1, 2, 3, 0, NB - 1, 4, 2]), k) for k in range(4)])
    dev = [torch.from_numpy(a).cuda() for a in [word, cemb] + tabs + [h_in]]
    A4, h = Guarded(M * 4 * E), Guarded(M * H)
    (_, ip), (_, cp), (_, ap) = keep = _i32(ids), _i32(cls), _i32(attrs4)
    _tap("etd_debug_dtrain_embed", M, H, E, V, NC, NB, ip, cp, ap, *(_p(t) for t in dev), A4.ptr, h.ptr)
    del keep
    A4.check("embed A4"); h.check("embed h")
    want_A4 = np.concatenate([tabs[k][attrs4[k]] for k in range(4)], axis=1)
    want_h = (word[ids] + cemb[cls]) + h_in
    assert _same_bits(A4.floats().view(M, 4 * E), torch.from_numpy(want_A4))
    assert _same_bits(h.floats().view(M, H), torch.from_numpy(want_h))
    # torch's own embedding states the same
    assert torch.equal(ts.embed_gather([torch.from_numpy(t) for t in tabs], attrs4), torch.from_numpy(want_A4))
    assert torch.equal(ts.embed_sum(torch.from_numpy(word), torch.from_numpy(cemb), ids, cls, torch.from_numpy(h_in)), torch.from_numpy(want_h))
    # an id outside its table is refused
    bad, bp = _i32(np.where(np.arange(M) == 3, NB, attrs4))
    assert _lib.lib().etd_debug_dtrain_embed(M, H, E, V, NC, NB, ip, cp, bp, *(_p(t) for t in dev), A4.ptr, h.ptr, None) == -22


# ------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("V", [1, 63, 64, 65, 157, 1000])
def test_cross_entropy_rows(V):
    g = torch.Generator().manual_seed(V)
    kinds = ["random", "sharp", "equal", "label_0", "label_last", "ignored", "random"]
    M = len(kinds)
    lg = torch.randn(M, V, generator=g)
    lg[1] *= 30.0
    lg[2] = 0.37
    labels = torch.randint(0, V, (M,), generator=g).numpy()
    labels[3], labels[4], labels[5] = 0, V - 1, -100
    scored = int((labels != -100).sum())
    scale = 0.5 / scored
    buf, rl = Guarded(M * V, data=lg), Guarded(M)
    lab, lp = _i32(labels)
    _tap("etd_debug_dtrain_ce", buf.ptr, M, V, lp, scale, rl.ptr)
    buf.check("ce gradient"); rl.check("ce row_loss")
    (l64, d64), (l32, d32) = ts.ce(lg.to(F64), labels, scale), ts.ce(lg, labels, scale)
    got_d, got_l = buf.floats().view(M, V), rl.floats()
    _hold("ce_row_loss", got_l, l32, l64, V=V)
    _hold("ce_dlogits", got_d, d32, d64, V=V)
    assert not _bits(got_d[5]).any() and not _bits(got_l[5:6]).any()      # the ignored row: +0.0 in every bit
    _verdict(f"stage_ce_V{V}")


# ------------------------------------------------------------------ column reductions
@pytest.mark.parametrize("M", [1, 7, 8, 9, 65])
def test_column_reductions_into_non_zero_gradients(M):
    for N in (1, 31, 32, 33, 256):
        g = torch.Generator().manual_seed(1000 * M + N)
        ld = N + 3
        dy_full, x = torch.randn(M, ld, generator=g), torch.randn(M, N, generator=g)
        dy = dy_full[:, :N]
        g0, g1 = torch.randn(N, generator=g), torch.randn(N, generator=g)
        mean, rstd = ts.ln_stats(x, EPS)                          # the statistics the forward pass saved: fp32
        dyd, xd, md, rd = dy_full.cuda(), x.cuda(), mean.cuda(), rstd.cuda()
        # mode 0
        o0 = Guarded(N, data=g0)
        _tap("etd_debug_dtrain_colred", 0, _p(dyd), ld, M, N, None, None, None, o0.ptr, None)
        o0.check("colred g0")
        _hold("colred0", o0.floats(), ts.colred(dy, g0), ts.colred(dy.to(F64), g0.to(F64)), M=M, N=N)
        # mode 1
        o0, o1 = Guarded(N, data=g0), Guarded(N, data=g1)
        _tap("etd_debug_dtrain_colred", 1, _p(dyd), ld, M, N, _p(xd), _p(md), _p(rd), o0.ptr, o1.ptr)
        o0.check("colred g0"); o1.check("colred g1")
        b32, w32 = ts.colred(dy, g0, x, EPS, g1)
        b64, w64 = ts.colred(dy.to(F64), g0.to(F64), x.to(F64), EPS, g1.to(F64))
        _hold("colred1_bias", o0.floats(), b32, b64, M=M, N=N)
        _hold("colred1_gain", o1.floats(), w32, w64, M=M, N=N)
    _verdict(f"stage_colred_M{M}")


# ------------------------------------------------------------------ embedding gradients
def _index_patterns(M, n_rows, pad):
    rng = np.random.default_rng(M)
    free = np.array([i for i in range(n_rows) if i != pad])
    mix = np.full(M, pad)                                         # segments of 1, 4, 5 and 37 rows, the rest on the padding row, interleaved
    where = rng.permutation(M)
    for row, (lo, hi) in zip((7, 0, n_rows - 1, 100), ((0, 1), (1, 5), (5, 10), (10, 47))):
        mix[where[lo:hi]] = row
    return {"one_row": np.full(M, 9), "all_pad": np.full(M, pad), "distinct": rng.permutation(free)[:M], "mix": mix}


@pytest.mark.parametrize("col0", [0, 24])
@pytest.mark.parametrize("width", [1, 24, 64, 65])
def test_embedding_gradient_segments(width, col0):
    M, n_rows, pad = 200, 256, 2
    ld = col0 + width + 5
    g = torch.Generator().manual_seed(100 * width + col0)
    src, grad0 = torch.randn(M, ld, generator=g), torch.randn(n_rows, width, generator=g)
    src_d = src.cuda()
    for name, idx in _index_patterns(M, n_rows, pad).items():
        out = Guarded(n_rows * width, data=grad0)
        ix, ixp = _i32(idx)
        _tap("etd_debug_dtrain_embed_grad", _p(src_d), ld, col0, width, M, ixp, n_rows, pad, out.ptr)
        out.check("embed_grad")
        got = out.floats().view(n_rows, width)
        idle = np.setdiff1d(np.arange(n_rows), idx[idx != pad])      # the padding row and every row no batch row points at keep their bits
        assert _same_bits(got[idle], grad0[idle]), name
        if name == "all_pad":
            assert _same_bits(got, grad0)
            continue
        _hold("embed_grad_" + name, got, ts.embed_grad(src, col0, width, idx, n_rows, pad, grad0),
              ts.embed_grad(src.to(F64), col0, width, idx, n_rows, pad, grad0.to(F64)), width=width, col0=col0)
    _verdict(f"stage_embed_grad_w{width}_c{col0}")


# ------------------------------------------------------------------ optimizer
def _adamw_case(n, seed):
    rng = np.random.default_rng(seed)
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m, v = (0.1 * rng.standard_normal(n)).astype(np.float32), (1e-3 * rng.random(n) + 1e-6).astype(np.float32)
    i = np.arange(0, n, 7)
    g[i] = np.array([1e4, 0.0, 1e-30], np.float32)[(i // 7) % 3]      # a huge gradient, an exact zero, one whose square underflows ...
    fresh = i[(i // 21) % 2 == 0]
    m[fresh] = 0.0; v[fresh] = 0.0                                  # ... half of them on zero moments: sqrt(v) = 0 or underflows, denom = eps
    return p, g, m, v


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_adamw_at_later_steps_with_moments(n):
    p0, g0, m0, v0 = _adamw_case(n, n)
    norm = tn.grad_norm({"x": g0})
    for step in (1, 2, 1000, 100000):
        for max_norm in (1.0, 1e9):
            assert (norm > max_norm) == (max_norm == 1.0)
            bufs = [Guarded(n, data=a) for a in (p0, g0, m0, v0)]
            _tap("etd_debug_dtrain_adamw", *(b.ptr for b in bufs), n, max_norm, norm, OPT["lr"], *OPT["betas"], OPT["eps"], OPT["weight_decay"], step)
            res = {}
            for dt in (np.float64, np.float32):                      # tn.clip_and_adamw: the restatement, in place, in the dtype of its arrays
                t = [{"x": np.array(a, dt)} for a in (p0, g0, m0, v0)]
                assert tn.clip_and_adamw(*t, step, max_norm, **OPT) == norm
                res[dt] = [d["x"] for d in t]
            for k, buf, r64, r32 in zip("pgmv", bufs, res[np.float64], res[np.float32]):
                buf.check("adamw " + k)
                got = buf.floats().numpy()
                assert np.isfinite(got).all(), k
                ulp = float(np.spacing(np.float32(np.abs(r64).max())))
                e_dev, e_32 = float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max())
                same = int((got.view(np.int32) == r32.view(np.int32)).sum())
                _note("adamw_" + k, n=n, step=step, max_norm=max_norm, err_device=e_dev, err_fp32_cpu=e_32, ulp=ulp, ratio=e_dev / max(e_32, ulp),
                      same_bits_as_fp32_restatement=same)
                if not e_dev <= max(4.0 * e_32, ulp):
                    _bad.append(("adamw_" + k, n, step, max_norm, e_dev, e_32, ulp))
    _verdict(f"stage_adamw_n{n}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537, 3000007])
def test_gradient_norm_against_longdouble(n):
    g = (np.random.default_rng(n).standard_normal(n) * 3.0).astype(np.float32)
    want = np.sqrt((g.astype(np.longdouble) ** 2).sum(dtype=np.longdouble))
    got, gd = C.c_double(), torch.from_numpy(g).cuda()
    _tap("etd_debug_dtrain_sumsq", _p(gd), n, C.byref(got))
    err = float(abs(np.longdouble(got.value) - want) / want)
    _note("sumsq", n=n, err_device=err, bound=n * 2.0 ** -52, ratio=err / (n * 2.0 ** -52))
    _verdict(f"stage_sumsq_n{n}")
    assert err <= n * 2.0 ** -52, (got.value, float(want), err)
