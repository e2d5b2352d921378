"""Every epilogue, row stride and tile edge of the fp32-grade GEMM family (csrc/gemm3.hip: k_gemm3, k_gemm3_s, k_ln_rows_f32) at the OPERATION level, through
etd_debug_gemm3_case / etd_debug_ln_rows_f32: the path G3Lin -> g3_lin_args -> launch_gemm3 / launch_gemm3_s every engine's exact-parity linear layer takes.

The reference is always float64 numpy of the same operation on the same fp32 inputs (bias, activation, residual, RoPE and LayerNorm in float64 too).  The yardstick
is tests/test_gpu_gemm3.py's: the kernel's error next to the error of a plain fp32 computation of the same thing against float64, with that file's multiples and
floors (1.5 x / 2e-7 of mean sum |x w| on a 96 x 96 corner against the k-ordered fp32 chain; 1e-6 of sum |x w| + |b| everywhere; 2 x / 1e-6 for LayerNorm + product).
Every output buffer is pre-filled with a NaN bit pattern and carries spare rows: exactly the addressed block may change, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from etude_amd import _lib

pytestmark = pytest.mark.gpu

T, S, AUTO = _lib.G3_KERNEL_TILE, _lib.G3_KERNEL_SMALL, _lib.G3_KERNEL_AUTO
CANARY = np.uint32(0x7FC0BEEF)            # a quiet NaN with a payload no computation produces
SPARE = 3                                 # whole rows allocated (and checked) past M


def _dev():
    return torch.device("cuda:0")


def _canary(n):
    return torch.from_numpy(np.full(int(n), CANARY, np.uint32).view(np.float32)).to(_dev())


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(_dev())


def _ptr(a):
    return None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _call(**kw):
    """fill a G3Case from keywords (arrays / tensors become pointers) and run it; returns the return code"""
    c = _lib.G3Case()
    keep = []
    for k, v in kw.items():
        if isinstance(v, (np.ndarray, torch.Tensor)):
            keep.append(v)
            v = _ptr(v)
        setattr(c, k, v)
    return _lib.lib().etd_debug_gemm3_case(C.byref(c), torch.cuda.current_stream(_dev()).cuda_stream)


def _inputs(rng, M, N, K):
    """the generator of tests/test_gpu_gemm3.py: rows of very different magnitude, weights ~ 0.05 N(0, 1), a non-trivial bias"""
    x = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 1, (M, 1)))).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    return x, w, b


def _chain(x, w, r, c):
    """the k-ordered fp32 multiply-add chain on the [r][c] corner"""
    acc = np.zeros((r, c), np.float32)
    for kk in range(x.shape[1]):
        acc = acc + x[:r, kk:kk + 1] * w[None, :c, kk]
    return acc


def _gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(u)) / np.sqrt(2.0)).numpy())


def _gelu32(u):
    t = torch.from_numpy(np.ascontiguousarray(u, np.float32))
    return (0.5 * t * (1.0 + torch.erf(t * np.float32(0.70710678118654752440)))).numpy()


def _linear_case(kernel, epi, M, N, K, seed, ldx=None, ldy=None, x=None, xbuf=None, bound=None, w=None, b=None):
    """run one BIAS / GELU / RELU / LOGITS / RESID case and return everything the assertions need; `epi` is 'bias', 'gelu', 'relu', 'logits' (bias NULL),
    'resid0' (add NULL), 'resid' (add set) or 'resid_inplace' (hin == hout)"""
    rng = np.random.default_rng(seed)
    x0, w0, b0 = _inputs(rng, M, N, K)
    x = x0 if x is None else x
    w = w0 if w is None else w
    b = b0 if b is None else b
    ldx = K if ldx is None else ldx
    ldy = N if ldy is None else ldy
    if xbuf is None:                                      # rows inside a buffer of row stride ldx >= K; the gap holds finite garbage no result may depend on
        xbuf = np.full((M - 1) * ldx + K, 1e30, np.float32)
        for i in range(M):
            xbuf[i * ldx:i * ldx + K] = x[i]
    xd = _up(xbuf)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    u = x64 @ w64.T
    full = np.abs(x64) @ np.abs(w64).T
    r, c = min(M, 96), min(N, 96)
    ch = _chain(x, w, r, c)
    scale = full[:r, :c].mean() or 1.0                   # (an all-zero operand: the exact-equality tests)
    resid = epi.startswith("resid")
    kw = dict(kernel=kernel, epi=_lib.G3_EPI["resid" if resid else epi], M=M, N=N, K=K, ldx=ldx, ldy=ldy, X=xd, x_elems=xbuf.size, W=w,
              bias=None if epi == "logits" else b, x_bound=float(np.abs(x).max() if bound is None else bound))
    if epi != "logits":
        u = u + b
        full = full + np.abs(b)
        ch = ch + b[:c]
    if epi == "gelu":
        ref, y32 = _gelu64(u), _gelu32(ch)
    elif epi == "relu":
        ref, y32 = np.maximum(u, 0.0), np.maximum(ch, np.float32(0))
        frac = (u < 0).mean()
        assert 0.4 <= frac <= 0.6, frac                   # roughly half of the pre-activations are negative
    elif resid:
        add = None if epi == "resid0" else (rng.standard_normal((M, N)) * 0.5).astype(np.float32)
        hin = (rng.standard_normal((M, N)) * 2.0).astype(np.float32)
        ref = (u + (0.0 if add is None else add.astype(np.float64))) + hin
        y32 = ((ch + add[:r, :c]) if add is not None else ch) + hin[:r, :c]
        full = full + (0.0 if add is None else np.abs(add)) + np.abs(hin)
        rows = M + SPARE
        hin_d = _canary(rows * N)
        hin_d[:M * N] = torch.from_numpy(hin.reshape(-1)).to(_dev())
        hout_d = hin_d if epi == "resid_inplace" else _canary(rows * N)
        kw.update(add=None if add is None else _up(add), hin=hin_d, hout=hout_d, h_elems=rows * N)
    else:
        ref, y32 = u, ch
    assert np.isfinite(ref).all() and np.isfinite(y32).all() and np.isfinite(full).all()
    if not resid:
        yd = _canary((M + SPARE) * ldy)
        kw.update(Y=yd, y_elems=yd.numel())
    rc = _call(**kw)
    _lib.check(rc, "etd_debug_gemm3_case")
    if resid:
        out = _bits(kw["hout"]).reshape(M + SPARE, N)
        assert (out[M:] == CANARY).all(), "rows past M were written"
        if epi != "resid_inplace":
            assert np.array_equal(_bits(hin_d)[:M * N].view(np.float32), hin.reshape(-1)), "hin was modified"
        y = out[:M].view(np.float32)
    else:
        out = _bits(yd).reshape(M + SPARE, ldy)
        assert (out[M:] == CANARY).all(), "rows past M were written"
        assert (out[:M, N:] == CANARY).all(), "the gap between N and ldy was written"
        y = out[:M, :N].view(np.float32)
    assert not (y.view(np.uint32) == CANARY).any(), "part of the [M][N] block was not written"
    assert np.isfinite(y).all()
    e3, e32 = np.abs(y[:r, :c] - ref[:r, :c]).max() / scale, np.abs(y32 - ref[:r, :c]).max() / scale
    worst = (np.abs(y - ref) / full).max()
    print(f"case {kernel} {epi} M={M} N={N} K={K} ldx={ldx} ldy={ldy}: e3={e3:.3e} e32={e32:.3e} everywhere={worst:.3e}")
    return dict(y=y, ref=ref, e3=e3, e32=e32, worst=worst, x=x, w=w, b=b, full=full)


def _assert_fp32_grade(res):
    assert res["e3"] <= max(1.5 * res["e32"], 2e-7), (res["e3"], res["e32"])
    assert res["worst"] <= 1e-6, res["worst"]


# ---- a. epilogue x shape matrix.  k_gemm3 (T) takes everything; k_gemm3_s (S) 2 .. 512 rows (.. 2 048 when Npad <= 512) with K % 512 == 0.  Every M of
# {1, 2, 31, 33, 127, 129, 513, 1100, 2048}, N of {64, 131, 384, 512, 1536} and K of {32, 96, 384, 512, 1024, 1152, 2048} appears per kernel that takes it;
# k_gemm3's row tiles (RT) x column tiles (NT): 9 x 1, 9 x 3, 9 x 12, 16 x 4, 17 x 3, 5 x 2 ...; k_gemm3_s's FT = Npad / 32 of 4, 8, 12, 16, 48.
MATRIX = [
    (T, "relu", 1, 64, 32), (T, "relu", 2, 131, 96), (T, "relu", 31, 384, 384), (T, "resid0", 33, 512, 1152), (T, "resid", 127, 1536, 512),
    (T, "resid_inplace", 129, 384, 1024), (T, "logits", 513, 131, 2048), (T, "bias", 1100, 64, 96), (T, "gelu", 1100, 384, 384), (T, "resid", 1100, 1536, 96),
    (T, "relu", 2048, 512, 32), (T, "bias", 2100, 384, 32), (T, "resid0", 1100, 64, 1152), (T, "logits", 129, 1536, 1024), (T, "gelu", 2, 131, 2048),
    (AUTO, "relu", 1, 131, 512),                                                    # one row is not k_gemm3_s's: gemm3_s_takes sends it to k_gemm3
    (S, "relu", 2, 64, 512), (S, "relu", 31, 131, 1024), (S, "resid", 33, 384, 2048), (S, "resid_inplace", 127, 512, 512), (S, "logits", 129, 1536, 512),
    (S, "bias", 513, 131, 512), (S, "gelu", 1100, 384, 1024), (S, "resid", 2048, 512, 512), (S, "relu", 1100, 64, 2048), (S, "bias", 2, 1536, 2048),
    (S, "gelu", 31, 1536, 512), (S, "logits", 2048, 131, 1024),
]


@pytest.mark.parametrize("kernel,epi,M,N,K", MATRIX)
def test_epilogue_shape_matrix(kernel, epi, M, N, K):
    _assert_fp32_grade(_linear_case(kernel, epi, M, N, K, seed=1000 * kernel + M + N + K))


def test_small_kernel_refuses_a_null_residual_addend():
    """dgemm_epilogue<RESID> reads `add` unconditionally (the decoder's parallel residual always has one): launch_gemm3_s refuses a null one instead of faulting"""
    M, N, K = 33, 384, 512
    x, w, b = _inputs(np.random.default_rng(3), M, N, K)
    h = _canary(M * N)
    rc = _call(kernel=S, epi=_lib.G3_EPI["resid"], M=M, N=N, K=K, ldx=K, ldy=N, X=_up(x), x_elems=M * K, W=w, bias=b, x_bound=8.0, hin=_up(np.zeros((M, N))), hout=h, h_elems=M * N)
    assert rc == -22
    assert (_bits(h) == CANARY).all()


def test_case_hook_refuses_what_would_be_a_stray_access():
    """a test's mistake is ETD_EINVAL on the host, never a launch"""
    M, N, K, nh = 40, 768, 512, 4
    x, w, b = _inputs(np.random.default_rng(4), M, N, K)
    xd, yd = _up(x), _canary(M * N)
    base = dict(kernel=AUTO, epi=_lib.G3_EPI["bias"], M=M, N=N, K=K, ldx=K, ldy=N, X=xd, x_elems=M * K, W=w, bias=b, x_bound=8.0, Y=yd, y_elems=M * N)
    assert _call(**base) == 0
    assert _call(**{**base, "x_elems": M * K - 1}) == -22                           # the last row would end past X
    assert _call(**{**base, "ldx": K + 64}) == -22
    assert _call(**{**base, "ldy": N + 4}) == -22                                   # ... past Y
    assert _call(**{**base, "ldy": N - 4}) == -22
    assert _call(**{**base, "kernel": S, "M": 1, "x_elems": K, "y_elems": N}) == -22          # k_gemm3_s forced on shapes it does not take
    xs = _up(x[:, :96])
    assert _call(**{**base, "kernel": S, "K": 96, "ldx": 96, "X": xs, "x_elems": M * 96, "W": np.ascontiguousarray(w[:, :96])}) == -22
    assert _call(**{**base, "kernel": T, "ln_g": np.ones(K, np.float32), "ln_b": np.zeros(K, np.float32), "ln_eps": 1e-5}) == -22      # the fused LayerNorm is k_gemm3_s's
    c = _lib.G3Case(); c.struct_bytes -= 4
    assert _lib.lib().etd_debug_gemm3_case(C.byref(c), None) == -22
    ctx, slots = 16, 2
    pos, slot, act = (np.arange(M) % ctx).astype(np.int32), (np.arange(M) % slots).astype(np.int32), np.ones(M, np.int32)
    tab = np.ones((ctx, 8), np.float32)
    q, kc, vc = _canary(M * nh * 64), _canary(slots * nh * ctx * 64), _canary(slots * nh * ctx * 64)
    qkv = dict(kernel=AUTO, epi=_lib.G3_EPI["qkv"], M=M, N=N, K=K, ldx=K, X=xd, x_elems=M * K, W=w, bias=b, x_bound=8.0, pos=pos, slot=slot, active=act, n_heads=nh, max_ctx=ctx,
               n_slots=slots, rope_rows=ctx, rope_cos=tab, rope_sin=tab, Q=q, q_elems=q.numel(), Kc=kc, Vc=vc, kv_elems=kc.numel())
    bad_pos, bad_slot = pos.copy(), slot.copy()
    bad_pos[M - 1] = ctx; bad_slot[3] = slots
    assert _call(**{**qkv, "pos": bad_pos}) == -22                                  # a position the RoPE table does not cover
    assert _call(**{**qkv, "slot": bad_slot}) == -22
    assert _call(**{**qkv, "kv_elems": kc.numel() - 1}) == -22
    assert _call(**{**qkv, "n_heads": 8}) == -22
    assert (_bits(q) == CANARY).all() and (_bits(kc) == CANARY).all() and (_bits(vc) == CANARY).all()
    assert _call(**qkv) == 0


# ---- b. strides and canaries (every case above already checks the spare rows; here the gaps)
@pytest.mark.parametrize("kernel", [T, S])
@pytest.mark.parametrize("epi,dldy", [("bias", 12), ("relu", 3), ("logits", 3), ("gelu", 12)])
def test_row_strides_leave_the_gaps_alone(kernel, epi, dldy):
    """ldx = K + 64: rows inside a wider buffer (the gap holds 1e30: nothing may read it into a result).  ldy = N + 12: vector stores next to a gap;
    ldy = N + 3: ldy % 4 != 0, the scalar store path.  N = 131: N % 4 != 0 and a padded last tile."""
    M, N, K = 130, 131, 512
    _assert_fp32_grade(_linear_case(kernel, epi, M, N, K, seed=77 + dldy + kernel, ldx=K + 64, ldy=N + dldy))


@pytest.mark.parametrize("R", [7, 1])
def test_overlapping_rows_of_the_conv2_shape(R):
    """Beat's conv2 as a GEMM: ldx = 32 < K = 384, N = 64 (Npad = 128): row i is the 384 floats starting at 32 i.  M = 42 R: 294 rows = two tiles and 38 rows; 42 = a third of one"""
    M, N, K, ldx = 42 * R, 64, 384, 32
    rng = np.random.default_rng(R)
    n = (M - 1) * ldx + K
    buf = (rng.standard_normal(n) * np.repeat(np.exp(rng.uniform(-3, 1, (n + 31) // 32)), 32)[:n]).astype(np.float32)
    x = np.lib.stride_tricks.as_strided(buf, (M, K), (ldx * 4, 4)).copy()
    _assert_fp32_grade(_linear_case(T, "relu", M, N, K, seed=R, ldx=ldx, ldy=N + 12, x=x, xbuf=buf))


# ---- c. QKV: partial RoPE + the KV-cache scatter
def _rope_tables(rows, theta=10000.0):
    """as etd_decoder_create builds them: fp32 inv_freq = 1 / theta^(2 i / 16), angle = pos * inv_freq, cosf / sinf"""
    inv = (np.float32(1.0) / np.power(np.float32(theta), (2 * np.arange(8)).astype(np.float32) / np.float32(16.0))).astype(np.float32)
    ang = (np.arange(rows, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _rotate(u, cos, sin, nh):
    """u [M][nh * 192] laid out [head][q | k | v][64]: dims (d, d + 8), d < 8, of every q and k rotated by the row's angle; cos / sin [M][8] (same dtype as u)"""
    o = u.copy().reshape(u.shape[0], nh, 3, 64)
    x1, x2 = o[:, :, :2, 0:8].copy(), o[:, :, :2, 8:16].copy()
    c, s = cos[:, None, None, :], sin[:, None, None, :]
    o[:, :, :2, 0:8] = x1 * c - x2 * s
    o[:, :, :2, 8:16] = x2 * c + x1 * s
    return o.reshape(u.shape)


QKV = [(T, 4, 33, 512), (T, 8, 130, 512), (T, 4, 600, 512), (T, 8, 130, 96), (S, 4, 33, 512), (S, 8, 130, 512), (S, 4, 490, 1024)]


@pytest.mark.parametrize("kernel,nh,M,K", QKV)
def test_qkv_rope_and_cache_scatter(kernel, nh, M, K):
    """Q rows to [M][heads * 64]; K / V rows to [slot][head][max_ctx][64] by (slot, pos), RoPE on dims 0 .. 15 of Q and K only.  Positions are not monotone, rows share
    slots, a quarter of the rows is inactive (some of them on an active row's very (slot, pos)), and two rows -- one active, one not -- sit at pos == max_ctx, where a
    finished stream's row sits when its bar ended at the context limit: they store no K / V, and the RoPE table rows from max_ctx on (NaN here) are never read."""
    N, n_slots, ctx = nh * 192, 5, 160
    rng = np.random.default_rng(kernel * 100 + nh + M + K)
    x, w, b = _inputs(rng, M, N, K)
    perm = rng.permutation(n_slots * ctx)[:M]                     # distinct (slot, pos) pairs in a random order
    slot, pos = (perm // ctx).astype(np.int32), (perm % ctx).astype(np.int32)
    active = (rng.uniform(size=M) >= 0.25).astype(np.int32)
    idle = np.flatnonzero(active == 0)
    busy = np.flatnonzero(active == 1)
    for i in idle[::2]:                                           # every other inactive row aims at an active row's cache position
        j = busy[int(rng.integers(busy.size))]
        slot[i], pos[i] = slot[j], pos[j]
    over = [int(busy[busy.size // 2]), int(idle[-1])]
    pos[over] = ctx                                               # (covered by the table passed below: rope_rows = ctx + 1)
    live = (active == 1) & (pos < ctx)
    assert 0.10 <= (active == 0).mean() <= 0.50, (active == 0).mean()
    pairs = list(zip(slot[live].tolist(), pos[live].tolist()))
    assert len(set(pairs)) == len(pairs)                          # no two active rows write the same cache row
    assert (np.diff(pos) < 0).any() and max(np.bincount(slot[live])) > 1
    cos, sin = _rope_tables(ctx + 1)
    cos[ctx:] = np.nan; sin[ctx:] = np.nan
    pt = np.minimum(pos, ctx - 1)                                 # rows at max_ctx: Q is not used by anything; it must only be finite
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    u = x64 @ w64.T + b
    ref = _rotate(u, cos[pt].astype(np.float64), sin[pt].astype(np.float64), nh)
    full = np.abs(x64) @ np.abs(w64).T + np.abs(b)
    fr = full.reshape(M, nh, 3, 64).copy()                        # a rotated output mixes the errors of its pair: |c|, |s| <= 1
    pair = fr[:, :, :2, 0:8] + fr[:, :, :2, 8:16]
    fr[:, :, :2, 0:8] = pair; fr[:, :, :2, 8:16] = pair
    full = fr.reshape(M, N)
    r, c = min(M, 96), 96
    y32 = _rotate(np.concatenate([_chain(x, w, r, c) + b[:c], np.zeros((r, N - c), np.float32)], 1), cos[pt[:r]], sin[pt[:r]], nh)[:, :c]
    assert np.isfinite(ref).all() and np.isfinite(y32).all()
    q = _canary((M + SPARE) * nh * 64)
    kv_n = n_slots * nh * ctx * 64
    kc, vc = _canary(kv_n + 64 * SPARE), _canary(kv_n + 64 * SPARE)
    _lib.check(_call(kernel=kernel, epi=_lib.G3_EPI["qkv"], M=M, N=N, K=K, ldx=K, X=_up(x), x_elems=M * K, W=w, bias=b, x_bound=float(np.abs(x).max()), pos=pos, slot=slot,
                     active=active, n_heads=nh, max_ctx=ctx, n_slots=n_slots, rope_rows=ctx + 1, rope_cos=cos, rope_sin=sin, Q=q, q_elems=M * nh * 64, Kc=kc, Vc=vc,
                     kv_elems=kv_n), "etd_debug_gemm3_case")
    qb = _bits(q).reshape(M + SPARE, nh * 64)
    assert (qb[M:] == CANARY).all(), "Q rows past M were written"
    kb, vb = _bits(kc), _bits(vc)
    assert (kb[kv_n:] == CANARY).all() and (vb[kv_n:] == CANARY).all()
    kb, vb = kb[:kv_n].reshape(n_slots, nh, ctx, 64), vb[:kv_n].reshape(n_slots, nh, ctx, 64)
    written = np.zeros((n_slots, ctx), bool)
    written[slot[live], pos[live]] = True
    for name, cb in (("K", kb), ("V", vb)):
        untouched = (cb == CANARY).all(axis=(1, 3))              # [slot][pos]: all heads, all 64 floats still the pattern
        assert (untouched == ~written).all(), f"{name} cache: a position no active row addresses was written, or an addressed one was not"
        assert not (cb.transpose(0, 2, 1, 3)[written] == CANARY).any()
    # the kernel's outputs gathered back into [M][N]; K / V of rows that store nothing: the reference itself (they have no output to compare)
    y = ref.astype(np.float32).reshape(M, nh, 3, 64)
    y[:, :, 0] = qb[:M].view(np.float32).reshape(M, nh, 64)
    rows = np.flatnonzero(live)
    y[rows, :, 1] = kb.view(np.float32)[slot[rows], :, pos[rows]]
    y[rows, :, 2] = vb.view(np.float32)[slot[rows], :, pos[rows]]
    y = y.reshape(M, N)
    assert np.isfinite(y).all()                                   # incl. Q of the rows at max_ctx: the NaN table rows were not used
    chk = np.ones((M, nh, 3, 64), bool)
    chk[~live, :, 1:] = False
    chk[pos >= ctx, :, 0] = False                                 # (Q of a row past the context: finite, checked above; no value is specified)
    chk = chk.reshape(M, N)
    err = np.abs(y - ref)
    scale = (np.abs(x64[:r]) @ np.abs(w64[:c]).T).mean()
    e3, e32 = (err[:r, :c] * chk[:r, :c]).max() / scale, (np.abs(y32 - ref[:r, :c]) * chk[:r, :c]).max() / scale
    worst = (err / full)[chk].max()
    print(f"qkv {kernel} heads={nh} M={M} K={K}: e3={e3:.3e} e32={e32:.3e} everywhere={worst:.3e} live={live.sum()}")
    assert chk[:r, :c].sum() > 0.6 * r * c
    assert e3 <= max(1.5 * e32, 2e-7), (e3, e32)
    assert worst <= 1e-6, worst


# ---- d. LOGITS with the fused LayerNorm on k_gemm3_s: the lm-head path
@pytest.mark.parametrize("M,N", [(2, 154), (54, 154), (54, 131)])
def test_lm_head_logits_with_fused_layernorm(M, N):
    rng = np.random.default_rng(M + N)
    K = 512
    x = (rng.standard_normal((M, K)) * 3.0 + 0.5).astype(np.float32)
    g = rng.uniform(0.5, 1.5, K).astype(np.float32); be = (rng.standard_normal(K) * 0.1).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.04).astype(np.float32)
    x64 = x.astype(np.float64)
    xn = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * g + be
    ref = xn @ w.astype(np.float64).T
    bound = np.sqrt(K - 1) * np.abs(g).max() + np.abs(be).max()           # g3_bound_ln
    ldy = N + 3
    yd = _canary((M + SPARE) * ldy)
    _lib.check(_call(kernel=S, epi=_lib.G3_EPI["logits"], M=M, N=N, K=K, ldx=K, ldy=ldy, X=_up(x), x_elems=M * K, W=w, bias=None, x_bound=float(bound), ln_g=g, ln_b=be,
                     ln_eps=1e-5, Y=yd, y_elems=yd.numel()), "etd_debug_gemm3_case")
    out = _bits(yd).reshape(M + SPARE, ldy)
    assert (out[M:] == CANARY).all() and (out[:M, N:] == CANARY).all()
    y = out[:M, :N].view(np.float32)
    xn32 = torch.nn.functional.layer_norm(torch.from_numpy(x), (K,), torch.from_numpy(g), torch.from_numpy(be), 1e-5)
    y32 = (xn32 @ torch.from_numpy(w).T).numpy()
    assert np.isfinite(ref).all() and np.isfinite(y32).all()
    e3, e32 = np.abs(y - ref).max(), np.abs(y32 - ref).max()
    print(f"ln+logits M={M} N={N}: e3={e3:.3e} e32={e32:.3e}")
    assert e3 <= max(2.0 * e32, 1e-6), (e3, e32)


# ---- e. launch_ln_rows_f32
LN_POOL = 1000


def _ln_pool(H):
    """1 000 rows in a fixed order: rows 0 mod 4 have mean >> std (100 + 0.01 N(0, 1)), rows 1 mod 8 are the constant 2.5, rows 5 mod 8 the constant 0.1, the rest ordinary
    (N(0, 1) x exp(U(-3, 1)) + N(0, 1) offsets).  The first M rows are the kernel's input; the yardstick's error is taken per kind over the whole pool."""
    rng = np.random.default_rng(H)
    h = (rng.standard_normal((LN_POOL, H)) * np.exp(rng.uniform(-3, 1, (LN_POOL, 1))) + rng.standard_normal((LN_POOL, 1))).astype(np.float32)
    i = np.arange(LN_POOL)
    kind = np.where(i % 4 == 0, 0, np.where(i % 8 == 1, 1, np.where(i % 8 == 5, 2, 3)))
    h[kind == 0] = (100.0 + 0.01 * rng.standard_normal(((kind == 0).sum(), H))).astype(np.float32)
    h[kind == 1] = np.float32(2.5)
    h[kind == 2] = np.float32(0.1)
    params = [(rng.uniform(0.5, 1.5, H).astype(np.float32), (rng.standard_normal(H) * 0.1).astype(np.float32)) for _ in range(2)]
    return h, kind, params


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("M", [1, 7, 1000])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_ln_rows_f32(H, M, two):
    """Against float64 LayerNorm, next to torch-CPU fp32 F.layer_norm's own error, per kind of row (multiple 2 x, no floor):
      * mean >> std: what any fp32 LayerNorm loses is the rounding of its fp32 mean (half an ulp of 100 = 3.8e-6, against a std of 0.01: ~1e-3 of the output);
      * the constant 2.5: every partial sum k x 2.5 is exact in fp32 in any order, so mean = 2.5, variance = 0, eps decides (rstd = 1 / sqrt(eps), no 0 / 0) and the output is
        b EXACTLY -- the yardstick's error is 0 and so must the kernel's be;
      * the constant 0.1 is not exactly summable: a two-pass fp32 LayerNorm is left with (0.1 - mean32) / sqrt(eps) g, where torch's Welford update gives exactly b.  The
        bound is derived, not measured: the kernel's sum is a chain of H / 64 - 1 additions per lane and 6 butterfly stages, each off by <= 2^-24 of the partial sum, and the
        product with 1 / H (not a power of two at H = 768) adds two more: |mean32 - 0.1| <= (H / 64 + 7) 2^-24 x 0.1, times max |g| / sqrt(eps), plus the output's own rounding;
      * ordinary rows."""
    h, kind, params = _ln_pool(H)
    eps = 1e-5
    h64 = h.astype(np.float64)
    z = (h64 - h64.mean(-1, keepdims=True)) / np.sqrt(h64.var(-1, keepdims=True) + eps)
    hd = _up(h[:M])
    outs = [_canary((M + SPARE) * H) for _ in range(2 if two else 1)]
    (g1, b1), (g2, b2) = params
    _lib.check(_lib.lib().etd_debug_ln_rows_f32(hd.data_ptr(), M, H, g1.ctypes.data, b1.ctypes.data, g2.ctypes.data if two else None, b2.ctypes.data if two else None, eps,
                                                outs[0].data_ptr(), outs[1].data_ptr() if two else None, torch.cuda.current_stream(_dev()).cuda_stream), "etd_debug_ln_rows_f32")
    assert np.array_equal(hd.cpu().numpy(), h[:M])
    for o, (g, b) in zip(outs, params):
        ref = z * g + b
        y32 = torch.nn.functional.layer_norm(torch.from_numpy(h), (H,), torch.from_numpy(g), torch.from_numpy(b), eps).numpy()
        assert np.isfinite(ref).all() and np.isfinite(y32).all()
        ob = _bits(o).reshape(M + SPARE, H)
        assert (ob[M:] == CANARY).all(), "rows past M were written"
        y = ob[:M].view(np.float32)
        assert np.isfinite(y).all()
        for kd in range(4):
            sel = kind[:M] == kd
            if not sel.any():
                continue
            ek, e32 = np.abs(y - ref[:M])[sel].max(), np.abs(y32 - ref)[kind == kd].max()
            print(f"ln H={H} M={M} two={two} kind={kd}: kernel={ek:.3e} fp32={e32:.3e}")
            if kd == 2:
                assert ek <= (H / 64 + 7) * 2.0 ** -24 * 0.1 * np.abs(g).max() / np.sqrt(eps) * (1 + 1e-6) + 2.0 ** -23 * np.abs(ref[:M][sel]).max(), ek
            else:
                assert ek <= 2.0 * e32, (kd, ek, e32)


# ---- f. row independence, bit for bit
def _rows_of(kernel, x, w, b, bound, N, K):
    M = x.shape[0]
    xd, yd = _up(x), _canary(M * N)
    _lib.check(_call(kernel=kernel, epi=_lib.G3_EPI["bias"], M=M, N=N, K=K, ldx=K, ldy=N, X=xd, x_elems=M * K, W=w, bias=b, x_bound=float(bound), Y=yd, y_elems=M * N), "case")
    return yd.cpu().numpy().reshape(M, N)


def test_tile_kernel_rows_do_not_depend_on_the_batch():
    """csrc/beat.hip relies on it: k_gemm3's result for a row depends neither on M nor on the row's place in its tile"""
    M, N, K = 1100, 384, 96
    x, w, b = _inputs(np.random.default_rng(11), M, N, K)
    bound = np.abs(x).max()
    big = _rows_of(T, x, w, b, bound, N, K)
    assert np.isfinite(big).all()
    for i in (0, 127, 128, 641, 1099):
        assert np.array_equal(_rows_of(T, x[i:i + 1], w, b, bound, N, K)[0], big[i]), i
    assert np.array_equal(_rows_of(T, x[301:338], w, b, bound, N, K), big[301:338])             # 37 rows from an unaligned offset: other lanes, other tile rows


def test_small_kernel_rows_do_not_depend_on_the_batch():
    """k_gemm3_s: the order of a row's additions (K over four waves, reduced 1, 2, 3 onto 0) is fixed, so 2, 54 and 512 rows give the same bits"""
    N, K = 384, 512
    x, w, b = _inputs(np.random.default_rng(12), 512, N, K)
    bound = np.abs(x).max()
    big = _rows_of(S, x, w, b, bound, N, K)
    assert np.isfinite(big).all()
    assert np.array_equal(_rows_of(S, x[:54], w, b, bound, N, K), big[:54])
    assert np.array_equal(_rows_of(S, x[:2], w, b, bound, N, K), big[:2])
    assert np.array_equal(_rows_of(S, x[333:335], w, b, bound, N, K), big[333:335])


# ---- g. operand-split edges
@pytest.mark.parametrize("kernel", [T, S])
def test_bound_a_power_of_two_with_elements_on_it(kernel):
    """x_bound = 4 exactly and elements at +-4: the scale must keep |s x| < 2^15 (g3_scale_log2 steps over the power of two), nothing saturates"""
    M, N, K = 130, 131, 512
    rng = np.random.default_rng(40 + kernel)
    x = rng.uniform(-4, 4, (M, K)).astype(np.float32)
    x[rng.uniform(size=(M, K)) < 0.05] = 4.0
    x[rng.uniform(size=(M, K)) < 0.05] = -4.0
    assert np.abs(x).max() == 4.0
    _assert_fp32_grade(_linear_case(kernel, "bias", M, N, K, seed=5, x=x, bound=4.0))


@pytest.mark.parametrize("kernel", [T, S])
def test_zero_operands_give_the_bias_exactly(kernel):
    M, N, K = 130, 131, 512
    x, w, b = _inputs(np.random.default_rng(50), M, N, K)
    res = _linear_case(kernel, "bias", M, N, K, seed=50, w=np.zeros_like(w))
    assert np.array_equal(res["y"], np.broadcast_to(b, (M, N)))
    res = _linear_case(kernel, "bias", M, N, K, seed=50, x=np.zeros_like(x), bound=1.0)
    assert np.array_equal(res["y"], np.broadcast_to(b, (M, N)))
    res = _linear_case(kernel, "bias", M, N, K, seed=50, x=np.zeros_like(x), bound=0.0)        # a zero bound: scale 1
    assert np.array_equal(res["y"], np.broadcast_to(b, (M, N)))


@pytest.mark.parametrize("kernel", [T, S])
def test_small_elements_under_a_loose_bound_keep_their_bits(kernel):
    """x_bound = 2^10 x the data's maximum: every |s x| < 2^5 of the planes' 2^15.  Derivation of the bound, in plane units t = s x, s = 2^x_log2:
    hi = f16(t) is off by <= 2^-11 |t|, so |t - hi| < 2^-6 here; lo = f16(t - hi) is off by <= 2^-11 |t - hi| <= 2^-22 |t| where lo is a normal f16 (>= 2^-14) and by
    <= 2^-25 (half the subnormal spacing 2^-24) where it is subnormal.  So |x - (hi + lo) / s| <= max(2^-22 |x|, 2^-25 / s), likewise for W with its own scale s_w, and per
    output  |y - ref| <= [sum_k |w_jk| 2^-25 / s + sum_k |x_ik| 2^-25 / s_w]  +  1e-6 (sum |x w| + |b|):  the second term is the file's fp32-grade bound and holds the 2^-22
    relative parts, the fp32 accumulation and the final rounding.  A device that flushed f16 subnormals would lose up to 2^-14 / s per element instead of 2^-25 / s
    (|t| ~ 1 is typical here, so that is ~6e-5 |x| against the 1e-6 |x| the second term allows).  gemm3.h's own (much weaker) statement, 2^-25 of the plane's range per element, is asserted as well."""
    M, N, K = 130, 131, 512
    x, w, b = _inputs(np.random.default_rng(60 + kernel), M, N, K)
    bound = float(np.abs(x).max()) * 1024.0
    res = _linear_case(kernel, "bias", M, N, K, seed=60 + kernel, bound=bound)
    s = 2.0 ** (15 - np.frexp(np.float32(bound) * np.float32(1.0001))[1])                      # g3_scale_log2
    sw = 2.0 ** (15 - np.frexp(np.abs(w).max())[1])                                            # g3_pack_weights_host
    assert np.abs(x).max() * s < 2.0 ** 5
    err = np.abs(res["y"] - res["ref"])
    w1, x1 = np.abs(w.astype(np.float64)).sum(1), np.abs(x.astype(np.float64)).sum(1)
    tight = 2.0 ** -25 / s * w1[None, :] + 2.0 ** -25 / sw * x1[:, None] + 1e-6 * res["full"]
    print(f"loose bound {kernel}: worst err / tight bound = {(err / tight).max():.3f}, subnormal-lo share of the bound = {(2.0 ** -25 / s * w1[None, :] / tight).max():.3e}")
    assert (err <= tight).all(), (err / tight).max()
    assert (err <= 2.0 ** -25 * bound * w1[None, :] + 1e-6 * res["full"]).all()               # gemm3.h: "an absolute error of at most 2^-25 of it"
    _assert_fp32_grade(res)
