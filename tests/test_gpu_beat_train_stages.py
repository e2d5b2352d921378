"""Stage edges of the Beat-Transformer trainer through the taps of include/etude_hip_debug.h (etd_debug_btrain_*), which call the engine's own launchers on the
test's inputs.  Every output sits between guard floats that must survive, and every float of an output must be written (tests/_util.py's Guarded).  The reference is
fp64 autograd of the per-kernel functions of tests/beat_train_np.py and tests/beat_train_stage_np.py; the bound is DESIGN.md 4j's rule per output:
``max|x - x64| / max|x64|`` at most 4 x the same figure of fp32 torch on the CPU, never asked below 4 * 2^-24, and exact zeros where fp64 is exactly zero by structure
(masked taps, head 7's key columns, unscored cells, a time tap outside the song, a maximum that is not positive).  Kernels that select or copy are compared bit for
bit; kernels that add a handful of fp32 terms in a stated order bit for bit with that sum.  The checks from "front end" on live in tests/beat_train_stage_np.py
(check_*), where tests/test_beat_train_stage_ref_cpu.py runs them on planted mistakes; they print every figure before the first one fails the test.

  kernel / pipeline                      test
  k_bt_conv1                             test_front_end_forward (random, each song alone, built routes)
  k_bt_patch2, k_bt_patch3, k_bt_pool3   test_front_end_forward
  k_bt_pool3_bwd, k_bt_patch3_bwd        test_front_end_backward
  k_bt_repack (both directions)          test_repack
  k_bt_fold2                             test_conv2_fold_is_the_ascending_kw_sum
  k_bt_conv1_bwd (+ k_bt_slice_sum)      test_conv1_weight_reduction_at_slice_edges (257 rows: 17 slices)
  k_bt_colsum_part, k_bt_slice_sum       test_column_sums, test_tempo_bias_column_sums, test_slice_sum_groups
  launch_bt_conv_wgrad                   test_conv_weight_gradient_segments
  k_bt_dattn, _dq, _dkv, k_bt_der_part   test_dilated_attention_backward (1025 rows: 17 slices)
  k_bt_iattn, k_bt_iattn_bwd             test_instrument_attention_backward
  k_bt_skipacc                           test_skip_mean_over_three_layers
  k_bt_dskip, k_bt_hmean, _hmean_bwd     test_instrument_means
  k_bt_tmean, k_bt_tmean_bwd             test_tempo_mean_at_segment_edges
  k_bt_relu, k_bt_relu_bwd               test_relu
  k_bt_bce, k_bt_tempo_ce                test_beat_loss_kernel, test_tempo_loss_kernel
  ffn_backward, proj_backward            test_feed_forward_backward, test_projection_backward
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import beat_train_np as bt
import beat_train_stage_np as S
from _util import Guarded
from etude_amd import _lib
from etude_amd._engine import i64

pytestmark = pytest.mark.gpu

def taken(g, *shape, what="an output"):
    """the floats of a Guarded buffer once its guards were found untouched and every float inside written"""
    g.check(what)
    return g.floats().numpy().reshape(*shape).copy()


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda().contiguous()
    return t, C.c_void_p(t.data_ptr())


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
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 63, 64, 65, 129, 16 * 64 + 1])
def test_dilated_attention_backward(T, layer):
    """one stem of T frames: T = 63, 64, 65 and 129 put one row less, exactly, one row more than one and two 64-row slices of the dEr reduction; 1025 rows are 17
    slices, one more than a group of k_bt_slice_sum"""
    I = 1 if T >= 63 else 2
    rep = S.Report("MI355X")
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
    part, dEr = Guarded((R + 63) // 64 * 1280), Guarded(1280, fill=0)
    ok(_lib.lib().etd_debug_btrain_dattn(1, i64([T]), I, layer, keep[0][1], keep[1][1], keep[2][1], keep[3][1], prob.ptr, skip.ptr, xout.ptr, dl.ptr, dqkv.ptr,
                                         part.ptr, dEr.ptr, None), "etd_debug_btrain_dattn")
    sk, g, de, pr = taken(skip, I, T, 256), taken(dqkv, I, T, 768), taken(dEr, 8, 32, 5), taken(prob, I, T, 8, 5)
    xo = taken(xout, R, 256)
    taken(part, -1); taken(dl, -1)
    rep.true("xout = xin + skip, one add", np.array_equal(xo, xin + sk.reshape(R, 256)))
    rep.hold(f"skip T={T} l={layer}", sk, s64, s32)
    rep.hold(f"dqkv T={T} l={layer}", g, dq64, dq32)
    rep.hold(f"dEr T={T} l={layer}", de, de64, de32)
    rep.true("head 7's key columns are exactly 0", not g[..., 256 + 224:512].any())      # read by no query
    t = np.arange(T)
    for h in range(8):
        for j, o in enumerate(bt.OFFSETS[h]):
            out = (t + o * 2 ** layer < 0) | (t + o * 2 ** layer >= T)
            rep.true(f"a tap outside the song has probability exactly 0 (head {h}, tap {j})", not pr[:, out, h, j].any())
            if out.all():
                rep.true(f"... and leaves its column of dEr exactly 0 (head {h}, tap {j})", not de[h, :, j].any())
    rep.done()


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
    dc1 = Guarded(R * 42 * 32)
    ok(_lib.lib().etd_debug_btrain_fold2(R, keep[0][1], keep[1][1], dc1.ptr, None), "etd_debug_btrain_fold2")
    assert np.array_equal(taken(dc1, R, 42, 32).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ conv1 weight reduction
def conv1_ref(feat, w, b, g, dtype):
    wt = torch.tensor(w, dtype=dtype, requires_grad=True)
    bb = torch.tensor(b, dtype=dtype, requires_grad=True)
    x = F.conv2d(torch.tensor(feat, dtype=dtype)[:, None], wt, bb, padding=(2, 0))                     # [I][32][T][126]
    c1 = torch.relu(F.max_pool2d(x, (1, 3), (1, 3)))                                                   # [I][32][T][42]
    (c1 * torch.tensor(g, dtype=dtype)).sum().backward()
    top = x.detach().reshape(*x.shape[:-1], 42, 3).sort(-1).values
    return wt.grad.numpy(), bb.grad.numpy(), c1.detach().numpy(), float(min((top[..., 2] - top[..., 1]).min(), top[..., 2].abs().min()))


@pytest.mark.parametrize("R", [1, 15, 16, 17, 31, 32, 33, 16 * 16 + 1])
def test_conv1_weight_reduction_at_slice_edges(R):
    """R rows of one stem (R x 126 conv columns): 1 row, and one row less, exactly, one row more than one and two 16-row slices; 257 rows are 17 slices, one more
    than a group of k_bt_slice_sum"""
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
    rep = S.Report("MI355X")
    dc1 = np.where(c1 > 0, g, 0).transpose(0, 2, 3, 1).reshape(R, 42, 32)    # the device's [row][p][co], masked by the ReLU as k_bt_fold2 leaves it
    keep = [dev(feat), dev(dc1), dev(w.reshape(32, 15)), dev(b)]
    part, dw, db = Guarded((R + 15) // 16 * 512), Guarded(480, fill=0), Guarded(32, fill=0)
    ok(_lib.lib().etd_debug_btrain_conv1_bwd(1, i64([R]), 1, keep[0][1], keep[1][1], keep[2][1], keep[3][1], part.ptr, dw.ptr, db.ptr, None),
       "etd_debug_btrain_conv1_bwd")
    taken(part, -1)
    rep.hold(f"conv1 dw R={R}", taken(dw, 32, 1, 5, 3), dw64, dw32)
    rep.hold(f"conv1 db R={R}", taken(db, 32), db64, db32)
    rep.done()


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
    ok(_lib.lib().etd_debug_btrain_iattn(len(Ts), i64(Ts), I, keep[0][1], keep[1][1], ao.ptr, dqkv.ptr, None), "etd_debug_btrain_iattn")
    o, g = taken(ao, R, 256), taken(dqkv, R, 768)
    rep, r0 = S.Report("MI355X"), 0
    for (qkv, dao), T in zip(per, Ts):
        o64, g64 = iattn_ref(qkv, dao, torch.float64)
        o32, g32 = iattn_ref(qkv, dao, torch.float32)
        rep.hold(f"iattn out I={I} T={T}", o[r0:r0 + I * T].reshape(I, T, 256), o64, o32)
        rep.hold(f"iattn dqkv I={I} T={T}", g[r0:r0 + I * T].reshape(I, T, 768), g64, g32)
        r0 += I * T
    rep.done()


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
    ok(_lib.lib().etd_debug_btrain_bce(keep[0][1], keep[1][1], keep[2][1], keep[3][1], Fr, nt, cell.ptr, dz.ptr, None), "etd_debug_btrain_bce")
    c, d = taken(cell, Fr, nt), taken(dz, Fr, nt)
    rep = S.Report("MI355X")
    rep.true("an unscored cell has loss and gradient exactly 0", not c[~m].any() and not d[~m].any())
    if scored != "none":
        rep.hold(f"bce cell {scored}", c, c64, c32)
        rep.hold(f"bce dz {scored}", d, d64, d32)
    rep.done()


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
    ok(_lib.lib().etd_debug_btrain_tempo_ce(keep[0][1], keep[1][1], C.c_void_p(hd.data_ptr()), coef, n, row.ptr, dt.ptr, None), "etd_debug_btrain_tempo_ce")
    r, d = taken(row, n), taken(dt, n, 300)
    rep = S.Report("MI355X")
    rep.true("a song without a tempo target has loss and gradient exactly 0", not r[has == 0].any() and not d[has == 0].any())
    if scored != "none":
        rep.hold(f"tempo row {scored}", r, r64, r32)
        rep.hold(f"tempo dt {scored}", d, d64, d32)
    rep.done()


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


# ------------------------------------------------------------------------------------------------ every other kernel: the taps behind the interface of S.RefDevice
class TapDevice:
    """numpy fp32 in, numpy fp32 out, through etd_debug_btrain_*; every output between guard floats"""

    def _run(self, name, n_out, call, data=None, shape=None):
        o = Guarded(n_out, data=data)
        ok(call(o.ptr), name)
        return taken(o, *(shape or (-1,)), what=name)

    def _front_fwd(self, which, a, Ts, I, n_out, shape, w=None, b=None):
        k = [dev(a)] + ([dev(w), dev(b)] if w is not None else [])
        wp, bp = (k[1][1], k[2][1]) if w is not None else (None, None)
        return self._run("etd_debug_btrain_front_fwd", n_out, lambda p: _lib.lib().etd_debug_btrain_front_fwd(which, len(Ts), i64(Ts), I, k[0][1], wp, bp, p, None), shape=shape)

    def conv1(self, feat, w, b, Ts, I):
        R = S.rows_of(Ts, I)
        return self._front_fwd(0, feat, Ts, I, R * 42 * 32, (R, 42, 32), w, b)

    def patch2(self, c1, Ts, I):
        R = S.rows_of(Ts, I)
        return self._front_fwd(1, c1, Ts, I, R * 24 * 384, (R * 24, 384))

    def patch3(self, c2, Ts, I):
        R = S.rows_of(Ts, I)
        return self._front_fwd(2, c2, Ts, I, R * 3 * 1152, (R * 3, 1152))

    def pool3(self, c3, Ts, I):
        R = S.rows_of(Ts, I)
        return self._front_fwd(3, c3, Ts, I, R * 256, (R, 256))

    def _front_bwd(self, which, c, g, Ts, I, shape):
        k = [dev(c), dev(g)]
        return self._run("etd_debug_btrain_front_bwd", int(np.prod(shape)), lambda p: _lib.lib().etd_debug_btrain_front_bwd(which, len(Ts), i64(Ts), I, k[0][1], k[1][1], p, None),
                         shape=shape)

    def pool3_bwd(self, c3, dx, Ts, I):
        return self._front_bwd(0, c3, dx, Ts, I, (S.rows_of(Ts, I), 3, 256))

    def patch3_bwd(self, c2, dx3, Ts, I):
        return self._front_bwd(1, c2, dx3, Ts, I, (S.rows_of(Ts, I), 24, 64))

    def repack(self, native):
        co, ci, kk = native.shape
        k = dev(native)
        return self._run("etd_debug_btrain_repack", native.size, lambda p: _lib.lib().etd_debug_btrain_repack(0, co, ci, kk, k[1], p, None), shape=(co, kk, ci))

    def unpack_add(self, native, packed):
        co, ci, kk = native.shape
        k = dev(packed)
        return self._run("etd_debug_btrain_repack", native.size, lambda p: _lib.lib().etd_debug_btrain_repack(1, co, ci, kk, p, k[1], None), data=native, shape=(co, ci, kk))

    def colsum(self, dy, ld, M, N, base, out0):
        k = dev(dy)
        part = Guarded((M + 255) // 256 * N)
        got = self._run("etd_debug_btrain_colsum", N, lambda p: _lib.lib().etd_debug_btrain_colsum(C.c_void_p(k[0].data_ptr() + 4 * base), ld, M, N, part.ptr, p, None), data=out0)
        part.check("colsum's scratch")
        return got

    def slice_sum(self, part, out0):
        k = dev(part)
        return self._run("etd_debug_btrain_slice_sum", part.shape[1], lambda p: _lib.lib().etd_debug_btrain_slice_sum(k[1], part.shape[0], part.shape[1], p, None), data=out0)

    def conv_wgrad(self, dY, X):
        (K, M), N = dY.shape, X.shape[1]
        k = [dev(dY), dev(X)]
        seg = Guarded((K + 4095) // 4096 * M * N)
        got = self._run("etd_debug_btrain_conv_wgrad", M * N, lambda p: _lib.lib().etd_debug_btrain_conv_wgrad(M, N, K, k[0][1], k[1][1], seg.ptr, p, None),
                        data=np.full(M * N, 12345.0, np.float32), shape=(M, N))      # overwritten, not added to
        seg.check("conv_wgrad's scratch")
        return got

    def _means(self, which, a, b, Ts, I, shape, first=0, data=None):
        k = [dev(a)] + ([dev(b)] if b is not None else [])
        bp = k[1][1] if b is not None else None
        return self._run("etd_debug_btrain_means", int(np.prod(shape)), lambda p: _lib.lib().etd_debug_btrain_means(which, len(Ts), i64(Ts), I, k[0][1], bp, first, p, None),
                         data=data, shape=shape)

    def skipacc(self, skip, tacc, Ts, I, first):
        return self._means(0, skip, None, Ts, I, (sum(Ts), 256), first, data=tacc)

    def dskip(self, dx, dtf, Ts, I):
        return self._means(1, dx, dtf, Ts, I, (S.rows_of(Ts, I), 256))

    def hmean(self, x, Ts, I):
        return self._means(2, x, None, Ts, I, (sum(Ts), 256))

    def hmean_bwd(self, x, dhm, Ts, I):
        return self._means(3, x, dhm, Ts, I, (S.rows_of(Ts, I), 256))

    def tmean(self, tacc, Ts, I):
        return self._means(4, tacc, None, Ts, I, (len(Ts), 256))

    def tmean_bwd(self, tacc, dtm, Ts, I):
        return self._means(5, tacc, dtm, Ts, I, (sum(Ts), 256))

    def relu(self, x):
        k = dev(x)
        return self._run("etd_debug_btrain_relu", x.size, lambda p: _lib.lib().etd_debug_btrain_relu(k[1], x.size, p, None, None), shape=x.shape)

    def relu_bwd(self, x, dy):
        k = dev(x)
        return self._run("etd_debug_btrain_relu", x.size, lambda p: _lib.lib().etd_debug_btrain_relu(k[1], x.size, None, p, None), data=dy, shape=x.shape)

    def ffn_bwd(self, x, params, dy, act, H):
        tr = trainer(H)
        mean, rstd = S.ln_stats(x)
        pre = S.ffn_pre(*(S.T(v, S.F64) for v in [x] + list(params[:4])))
        k = [dev(x), dev(mean), dev(rstd), dev(pre.numpy()), dev(np.concatenate([np.asarray(p).reshape(-1) for p in params]))]
        R, n = x.shape[0], sum(np.asarray(p).size for p in params)
        G, dx = Guarded(n, fill=0), Guarded(R * 256, data=dy)
        ok(_lib.lib().etd_debug_btrain_ffn_bwd(tr.h, R, act, k[0][1], k[1][1], k[2][1], k[3][1], k[4][1], G.ptr, dx.ptr, None), "etd_debug_btrain_ffn_bwd")
        g, res, o = taken(G, -1, what="ffn_bwd's gradients"), [taken(dx, R, 256, what="ffn_bwd's dx")], 0
        for p in params:
            res.append(g[o:o + np.asarray(p).size].reshape(np.asarray(p).shape))
            o += np.asarray(p).size
        return res

    def proj_bwd(self, x, params, dqkv, dx0):
        tr = trainer(256)
        mean, rstd = S.ln_stats(x)
        k = [dev(x), dev(mean), dev(rstd), dev(dqkv), dev(np.concatenate([np.asarray(p).reshape(-1) for p in params]))]
        R, n = x.shape[0], sum(np.asarray(p).size for p in params)
        g0 = np.zeros(n, np.float32)
        g0[n - 512:n - 256] = 7.25                                                   # the key third of the bias gradient: never touched
        G, dx = Guarded(n, data=g0), Guarded(R * 256, data=dx0)
        ok(_lib.lib().etd_debug_btrain_proj_bwd(tr.h, R, k[0][1], k[1][1], k[2][1], k[3][1], k[4][1], G.ptr, dx.ptr, None), "etd_debug_btrain_proj_bwd")
        g, o = taken(G, -1, what="proj_bwd's gradients"), 0
        res = [taken(dx, R, 256, what="proj_bwd's dx")]
        for p in params:
            res.append(g[o:o + np.asarray(p).size].reshape(np.asarray(p).shape))
            o += np.asarray(p).size
        return res + [bool((g[n - 512:n - 256] == 7.25).all())]


@functools.lru_cache(maxsize=None)
def trainer(H):
    """a one-layer engine whose scratch the two pipeline taps run on (its own parameters and gradients are not involved)"""
    from etude_amd.beat_train import BeatTrainer
    from etude_amd.config import BeatDetectorModelConfig
    return BeatTrainer(BeatDetectorModelConfig(attn_len=5, instr=1, ntoken=2, dmodel=256, nhead=8, d_hid=H, nlayers=1, norm_first=True), max_rows=max(S.PIPE_ROWS), max_seqs=1)


def run(check, *args):
    rep = S.Report("MI355X")
    check(rep, TapDevice(), *args)
    rep.done()
    return rep.worst


@pytest.mark.parametrize("I", S.INSTR)
def test_front_end_forward(I):
    """three songs of 2, 1 and 7 frames: conv1 under the rule, alone and batched the same bits, and exact on built pool triples; the patches and pool3 bit for bit"""
    run(S.check_conv1, I)
    run(S.check_patches_and_pool, I)


@pytest.mark.parametrize("I", S.INSTR)
def test_front_end_backward(I):
    """pool routes on triples decidable by construction (two and three equal maxima, a maximum of 0.0 and of -0.0, all negative, the maximum in each position), exact;
    patch3_bwd per pooled column against its ordered fp32 sum, and nothing from a time tap outside the song"""
    run(S.check_pool3_bwd, I)
    run(S.check_patch3_bwd, I)


def test_repack():
    run(S.check_repack)


@pytest.mark.parametrize("M", S.COLSUM_M)
def test_column_sums(M):
    """M = 4097 is 17 slices: one more than a group of k_bt_slice_sum.  out starts non-zero (the launch adds); columns outside [0, N) hold 1e30"""
    run(S.check_colsum, M)


def test_tempo_bias_column_sums():
    """N = 300 over M = 1 .. 8 rows: the tempo head's bias over the songs of a call, the eight sub-slices of k_bt_colsum_part partly filled"""
    run(S.check_colsum_tempo)


def test_slice_sum_groups():
    run(S.check_slice_sum)


@pytest.mark.parametrize("M,N,K", S.WGRAD_CASES)
def test_conv_weight_gradient_segments(M, N, K):
    """K one less than, exactly and one more than a segment of 4 096 rows, and 17 segments; dw starts as sentinels and is overwritten"""
    run(S.check_conv_wgrad, M, N, K)


@pytest.mark.parametrize("I", S.INSTR)
def test_skip_mean_over_three_layers(I):
    run(S.check_skipacc, I)


@pytest.mark.parametrize("I", S.INSTR)
def test_instrument_means(I):
    run(S.check_means, I)


@pytest.mark.parametrize("I", S.INSTR)
def test_tempo_mean_at_segment_edges(I):
    """songs of 129, 1, 127, 128 and 257 frames in one call"""
    run(S.check_tmean, I)


def test_relu():
    run(S.check_relu)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("R", S.PIPE_ROWS)
def test_feed_forward_backward(R, H, act):
    """every gradient of one sublayer against fp64 autograd, the LayerNorm gain and bias (k_tcolred, mode 1) among them; 4097 rows are 17 slices of the bias sums"""
    run(S.check_ffn_bwd, R, H, act)


@pytest.mark.parametrize("R", S.PIPE_ROWS)
def test_projection_backward(R):
    run(S.check_proj_bwd, R)


def test_new_taps_refuse_malformed_arguments_before_any_launch():
    lib, d = _lib.lib(), C.c_void_p(4096)      # a device pointer that is never read
    bad = {
        "front_fwd: which 4": lib.etd_debug_btrain_front_fwd(4, 1, i64([4]), 1, d, d, d, d, None),
        "front_fwd: conv1 without weights": lib.etd_debug_btrain_front_fwd(0, 1, i64([4]), 1, d, None, None, d, None),
        "front_fwd: T = 0": lib.etd_debug_btrain_front_fwd(1, 1, i64([0]), 1, d, None, None, d, None),
        "front_bwd: no gradient": lib.etd_debug_btrain_front_bwd(0, 1, i64([4]), 1, d, None, d, None),
        "front_bwd: instr 9": lib.etd_debug_btrain_front_bwd(1, 1, i64([4]), 9, d, d, d, None),
        "repack: dir 2": lib.etd_debug_btrain_repack(2, 4, 4, 4, d, d, None),
        "repack: kk 0": lib.etd_debug_btrain_repack(0, 4, 4, 0, d, d, None),
        "colsum: ld < N": lib.etd_debug_btrain_colsum(d, 3, 4, 4, d, d, None),
        "colsum: M 0": lib.etd_debug_btrain_colsum(d, 4, 0, 4, d, d, None),
        "slice_sum: no slices": lib.etd_debug_btrain_slice_sum(d, 0, 4, d, None),
        "means: which 6": lib.etd_debug_btrain_means(6, 1, i64([4]), 1, d, d, 0, d, None),
        "means: dskip without dtf": lib.etd_debug_btrain_means(1, 1, i64([4]), 1, d, None, 0, d, None),
        "means: first_layer 2": lib.etd_debug_btrain_means(0, 1, i64([4]), 1, d, None, 2, d, None),
        "relu: no output": lib.etd_debug_btrain_relu(d, 4, None, None, None),
        "conv_wgrad: K 0": lib.etd_debug_btrain_conv_wgrad(4, 4, 0, d, d, d, d, None),
        "ffn_bwd: no handle": lib.etd_debug_btrain_ffn_bwd(None, 4, 0, d, d, d, d, d, d, d, None),
        "proj_bwd: no handle": lib.etd_debug_btrain_proj_bwd(None, 4, d, d, d, d, d, d, d, None),
    }
    assert all(rc == -22 for rc in bad.values()), bad
