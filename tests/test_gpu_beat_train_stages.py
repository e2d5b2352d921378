"""Stage edges of the Beat-Transformer trainer through the taps of include/etude_hip_debug.h (etd_debug_btrain_*), which call the engine's own launchers on the
test's inputs.  Every output sits between guard floats that must survive.  The reference is fp64 autograd of the per-kernel functions of tests/beat_train_np.py; the
bound is DESIGN.md 4j's rule per output: ``max|x - x64| / max|x64|`` at most 4 x the same figure of fp32 torch on the CPU, never asked below 4 * 2^-24, and exact
zeros where fp64 is exactly zero by structure (masked taps, head 7's key columns, unscored cells).  The conv2 fold adds at most 12 fp32 terms in ascending kw: it is
compared bit for bit with that sum.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import beat_train_np as bt
from etude_amd import _lib
from etude_amd._engine import i64

pytestmark = pytest.mark.gpu

FLOOR = 4.0 * 2.0 ** -24
GUARD, SENTINEL = 64, 12345.0


class Guarded:
    """a device buffer of n floats between two runs of GUARD sentinels"""

    def __init__(self, n, fill=None):
        self.full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.n = n
        if fill is not None:
            self.view()[:] = torch.as_tensor(fill, dtype=torch.float32).reshape(-1).cuda()

    def view(self):
        return self.full[GUARD:GUARD + self.n]

    def ptr(self):
        return C.c_void_p(self.view().data_ptr())

    def get(self, *shape):
        torch.cuda.synchronize()
        f = self.full.cpu().numpy()
        assert (f[:GUARD] == SENTINEL).all() and (f[GUARD + self.n:] == SENTINEL).all(), "a guard float was overwritten"
        return f[GUARD:GUARD + self.n].reshape(*shape).copy()


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda().contiguous()
    return t, C.c_void_p(t.data_ptr())


def held(x, x64, x32, what):
    e, e32 = bt.rel_err(x, x64), bt.rel_err(x32, x64)
    print(what, dict(err=e, err32=e32))
    assert e <= max(4.0 * e32, FLOOR), (what, e, e32)


def ok(rc, what):
    _lib.check(rc, what)


# ------------------------------------------------------------------------------------------------ dilated attention, backward and the dEr reduction
def dattn_ref(qkv, Er, dO, layer, dtype):
    q = torch.tensor(qkv, dtype=dtype, requires_grad=True)
    e = torch.tensor(Er, dtype=dtype, requires_grad=True)
    skip = bt.dattn_from_qkv(q, e, layer)
    (skip * torch.tensor(dO, dtype=dtype)).sum().backward()
    return skip.detach().numpy(), q.grad.numpy(), e.grad.numpy()


@pytest.mark.parametrize("layer", [0, 1, 8])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 63, 64, 65, 129])
def test_dilated_attention_backward(T, layer):
    """one stem of T frames: T = 63, 64, 65 and 129 put one row less, exactly, one row more than one and two 64-row slices of the dEr reduction"""
    I = 1 if T >= 63 else 2
    rng = np.random.default_rng(1000 * layer + T)
    R = I * T
    qkv = rng.standard_normal((I, T, 768)).astype(np.float32)
    Er = rng.standard_normal((8, 32, 5)).astype(np.float32)
    xin = rng.standard_normal((R, 256)).astype(np.float32)
    dO = rng.standard_normal((I, T, 256)).astype(np.float32)
    s64, dq64, de64 = dattn_ref(qkv, Er, dO, layer, torch.float64)
    s32, dq32, de32 = dattn_ref(qkv, Er, dO, layer, torch.float32)
    keep = [dev(a) for a in (qkv, Er, xin, dO)]
    prob, skip, xout, dl, dqkv = Guarded(R * 40), Guarded(R * 256), Guarded(R * 256), Guarded(R * 40), Guarded(R * 768)
    part, dEr = Guarded((R + 63) // 64 * 1280), Guarded(1280, np.zeros(1280))
    ok(_lib.lib().etd_debug_btrain_dattn(1, i64([T]), I, layer, keep[0][1], keep[1][1], keep[2][1], keep[3][1], prob.ptr(), skip.ptr(), xout.ptr(), dl.ptr(), dqkv.ptr(),
                                         part.ptr(), dEr.ptr(), None), "etd_debug_btrain_dattn")
    sk, g, de, pr = skip.get(I, T, 256), dqkv.get(I, T, 768), dEr.get(8, 32, 5), prob.get(I, T, 8, 5)
    xo = xout.get(R, 256)
    part.get(-1); dl.get(-1)
    assert np.array_equal(xo, xin + sk.reshape(R, 256))
    held(sk, s64, s32, f"skip T={T} l={layer}")
    held(g, dq64, dq32, f"dqkv T={T} l={layer}")
    held(de, de64, de32, f"dEr T={T} l={layer}")
    assert not g[..., 256 + 224:512].any()                                  # head 7's keys are read by no query
    t = np.arange(T)
    for h in range(8):
        for j, o in enumerate(bt.OFFSETS[h]):
            out = (t + o * 2 ** layer < 0) | (t + o * 2 ** layer >= T)
            assert not pr[:, out, h, j].any()                                # a tap outside the song has probability exactly 0
            if out.all():
                assert not de[h, :, j].any()                                 # ... and leaves its column of dEr exactly 0


# ------------------------------------------------------------------------------------------------ conv2 fold
@pytest.mark.parametrize("R", [1, 2, 3])
def test_conv2_fold_is_the_ascending_kw_sum(R):
    rng = np.random.default_rng(R)
    dpatch = rng.standard_normal((R, 24, 12, 32)).astype(np.float32)
    c1 = np.maximum(rng.standard_normal((R, 42, 32)), 0).astype(np.float32)
    want = np.zeros((R, 42, 32), np.float32)
    for kw in range(12):                                                     # fp32, ascending kw: the kernel's own order
        for col in range(24):
            want[:, col + kw] = want[:, col + kw] + dpatch[:, col, kw]
    want = np.where(c1 > 0, want, np.float32(0))
    keep = [dev(dpatch), dev(c1)]
    out = Guarded(R * 42 * 32)
    ok(_lib.lib().etd_debug_btrain_fold2(R, keep[0][1], keep[1][1], out.ptr(), None), "etd_debug_btrain_fold2")
    assert np.array_equal(out.get(R, 42, 32).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ conv1 weight reduction
def conv1_ref(feat, w, b, g, dtype):
    wt = torch.tensor(w, dtype=dtype, requires_grad=True)
    bb = torch.tensor(b, dtype=dtype, requires_grad=True)
    x = F.conv2d(torch.tensor(feat, dtype=dtype)[:, None], wt, bb, padding=(2, 0))                     # [I][32][T][126]
    c1 = torch.relu(F.max_pool2d(x, (1, 3), (1, 3)))                                                   # [I][32][T][42]
    (c1 * torch.tensor(g, dtype=dtype)).sum().backward()
    top = x.detach().reshape(*x.shape[:-1], 42, 3).sort(-1).values
    return wt.grad.numpy(), bb.grad.numpy(), c1.detach().numpy(), float(min((top[..., 2] - top[..., 1]).min(), top[..., 2].abs().min()))


@pytest.mark.parametrize("R", [1, 15, 16, 17, 31, 32, 33])
def test_conv1_weight_reduction_at_slice_edges(R):
    """R rows of one stem (R x 126 conv columns): 1 row, and one row less, exactly, one row more than one and two 16-row slices"""
    for seed in range(100 * R, 100 * R + 50):                                # the first seed at which every pool choice is decidable in fp32 (values below 10: fp32 resolves 1e-6)
        rng = np.random.default_rng(seed)
        feat = rng.uniform(-80, 0, (1, R, 128)).astype(np.float32)
        w = (0.1 * rng.uniform(-0.26, 0.26, (32, 1, 5, 3))).astype(np.float32)
        b = rng.uniform(0.5, 2.5, 32).astype(np.float32)
        g = rng.standard_normal((1, 32, R, 42)).astype(np.float32)
        dw64, db64, c1, margin = conv1_ref(feat, w, b, g, torch.float64)
        if margin > 1e-5:
            break
    dw32, db32, _, _ = conv1_ref(feat, w, b, g, torch.float32)
    assert margin > 1e-5, margin
    dc1 = np.where(c1 > 0, g, 0).transpose(0, 2, 3, 1).reshape(R, 42, 32)    # the device's [row][p][co], masked by the ReLU as k_bt_fold2 leaves it
    keep = [dev(feat), dev(dc1), dev(w.reshape(32, 15)), dev(b)]
    part, dw, db = Guarded((R + 15) // 16 * 512), Guarded(480, np.zeros(480)), Guarded(32, np.zeros(32))
    ok(_lib.lib().etd_debug_btrain_conv1_bwd(1, i64([R]), 1, keep[0][1], keep[1][1], keep[2][1], keep[3][1], part.ptr(), dw.ptr(), db.ptr(), None),
       "etd_debug_btrain_conv1_bwd")
    part.get(-1)
    held(dw.get(32, 1, 5, 3), dw64, dw32, f"conv1 dw R={R}")
    held(db.get(32), db64, db32, f"conv1 db R={R}")


# ------------------------------------------------------------------------------------------------ instrument attention
def iattn_ref(qkv, dao, dtype):
    a = torch.tensor(qkv, dtype=dtype, requires_grad=True)
    o = bt.iattn_from_qkv(a)
    (o * torch.tensor(dao, dtype=dtype)).sum().backward()
    return o.detach().numpy(), a.grad.numpy()


@pytest.mark.parametrize("I", [1, 3, 5, 8])
def test_instrument_attention_backward(I):
    Ts = [3, 1, 6]                                                           # three songs: rows of a frame are T_s apart, different per song
    rng = np.random.default_rng(I)
    per = [(rng.standard_normal((I, T, 768)).astype(np.float32), rng.standard_normal((I, T, 256)).astype(np.float32)) for T in Ts]
    R = I * sum(Ts)
    keep = [dev(np.concatenate([p[0].reshape(-1, 768) for p in per])), dev(np.concatenate([p[1].reshape(-1, 256) for p in per]))]
    ao, dqkv = Guarded(R * 256), Guarded(R * 768)
    ok(_lib.lib().etd_debug_btrain_iattn(len(Ts), i64(Ts), I, keep[0][1], keep[1][1], ao.ptr(), dqkv.ptr(), None), "etd_debug_btrain_iattn")
    o, g = ao.get(R, 256), dqkv.get(R, 768)
    r0 = 0
    for (qkv, dao), T in zip(per, Ts):
        o64, g64 = iattn_ref(qkv, dao, torch.float64)
        o32, g32 = iattn_ref(qkv, dao, torch.float32)
        held(o[r0:r0 + I * T].reshape(I, T, 256), o64, o32, f"iattn out I={I} T={T}")
        held(g[r0:r0 + I * T].reshape(I, T, 768), g64, g32, f"iattn dqkv I={I} T={T}")
        r0 += I * T


# ------------------------------------------------------------------------------------------------ the two loss kernels
@pytest.mark.parametrize("scored", ["none", "one", "all"])
def test_beat_loss_kernel(scored):
    rng = np.random.default_rng(7)
    Fr, nt = 37, 3
    z = (4 * rng.standard_normal((Fr, nt))).astype(np.float32)
    y = rng.choice(np.array([0.0, 0.25, 0.75, 1.0], np.float32), (Fr, nt))
    m = np.zeros((Fr, nt), bool)
    if scored == "one":
        m[11, 2] = True
    elif scored == "all":
        m[:] = True
    y = np.where(m, y, np.float32(-1))
    pw, coef = np.array([3.0, 7.0, 2.0], np.float32), np.array([0.5, 0.125, 0.03125], np.float32)

    def ref(dtype):
        zt = torch.tensor(z, dtype=dtype, requires_grad=True)
        yt = torch.tensor(np.where(m, y, 0), dtype=dtype)
        cell = (1 + (torch.tensor(pw, dtype=dtype) - 1) * yt) * F.binary_cross_entropy_with_logits(zt, yt, reduction="none") * torch.tensor(m, dtype=dtype)
        (cell * torch.tensor(coef, dtype=dtype)).sum().backward()
        return cell.detach().numpy(), zt.grad.numpy()
    c64, d64 = ref(torch.float64)
    c32, d32 = ref(torch.float32)
    keep = [dev(z), dev(y), dev(pw), dev(coef)]
    cell, dz = Guarded(Fr * nt), Guarded(Fr * nt)
    ok(_lib.lib().etd_debug_btrain_bce(keep[0][1], keep[1][1], keep[2][1], keep[3][1], Fr, nt, cell.ptr(), dz.ptr(), None), "etd_debug_btrain_bce")
    c, d = cell.get(Fr, nt), dz.get(Fr, nt)
    assert not c[~m].any() and not d[~m].any()
    if scored != "none":
        held(c, c64, c32, f"bce cell {scored}")
        held(d, d64, d32, f"bce dz {scored}")


@pytest.mark.parametrize("scored", ["none", "one", "all"])
def test_tempo_loss_kernel(scored):
    rng = np.random.default_rng(9)
    n = 3
    t = (3 * rng.standard_normal((n, 300))).astype(np.float32)
    p = rng.random((n, 300)) ** 8
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    has = np.array({"none": [0, 0, 0], "one": [0, 1, 0], "all": [1, 1, 1]}[scored], np.int32)
    coef = 0.375

    def ref(dtype):
        tt = torch.tensor(t, dtype=dtype, requires_grad=True)
        row = -(torch.tensor(p, dtype=dtype) * torch.log_softmax(tt, -1)).sum(-1) * torch.tensor(has, dtype=dtype)
        (row.sum() * coef).backward()
        return row.detach().numpy(), tt.grad.numpy()
    r64, d64 = ref(torch.float64)
    r32, d32 = ref(torch.float32)
    keep = [dev(t), dev(p)]
    hd = torch.as_tensor(has).cuda()
    row, dt = Guarded(n), Guarded(n * 300)
    ok(_lib.lib().etd_debug_btrain_tempo_ce(keep[0][1], keep[1][1], C.c_void_p(hd.data_ptr()), coef, n, row.ptr(), dt.ptr(), None), "etd_debug_btrain_tempo_ce")
    r, d = row.get(n), dt.get(n, 300)
    assert not r[has == 0].any() and not d[has == 0].any()
    if scored != "none":
        held(r, r64, r32, f"tempo row {scored}")
        held(d, d64, d32, f"tempo dt {scored}")


def test_taps_refuse_malformed_arguments_before_any_launch():
    lib, d = _lib.lib(), C.c_void_p(4096)      # a device pointer that is never read
    bad = {
        "dattn: T = 0": lib.etd_debug_btrain_dattn(1, i64([0]), 1, 0, d, d, d, None, d, d, d, None, None, None, None, None),
        "dattn: layer 16": lib.etd_debug_btrain_dattn(1, i64([4]), 1, 16, d, d, d, None, d, d, d, None, None, None, None, None),
        "dattn: dO without dqkv": lib.etd_debug_btrain_dattn(1, i64([4]), 1, 0, d, d, d, d, d, d, d, d, None, d, d, None),
        "iattn: instr 9": lib.etd_debug_btrain_iattn(1, i64([4]), 9, d, None, d, None, None),
        "fold2: rows 0": lib.etd_debug_btrain_fold2(0, d, d, d, None),
        "conv1_bwd: no part": lib.etd_debug_btrain_conv1_bwd(1, i64([4]), 1, d, d, d, d, None, d, d, None),
        "bce: ntoken 65": lib.etd_debug_btrain_bce(d, d, d, d, 4, 65, d, d, None),
        "tempo_ce: n 0": lib.etd_debug_btrain_tempo_ce(d, d, d, 1.0, 0, d, d, None),
        "read_rows: no handle": lib.etd_debug_btrain_read_rows(None, 0, d, 4, None),
    }
    assert all(rc == -22 for rc in bad.values()), bad
