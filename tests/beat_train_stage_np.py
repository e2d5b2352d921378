"""Per-kernel references of the Beat-Transformer trainer (csrc/beat_train.hip), one per tap of include/etude_hip_debug.h that tests/test_gpu_beat_train_stages.py
drives, with the inputs and the rule of that file, so that tests/test_beat_train_stage_ref_cpu.py can put a wrong variant in the device's place.

Every function takes torch tensors and runs in their dtype (fp64: the reference; fp32: the yardstick).  Backward references are autograd of the forward function.
A batch is ``Ts`` (frames per song) and ``I`` (instruments): song s owns rows [row0_s, row0_s + I T_s) laid out [I][T_s], frames are (song, t).  Kernels that only
select, copy or add a handful of terms in a stated order have an ``*_ordered`` restatement in numpy fp32 with the kernel's own order, for a bit-for-bit comparison.

``mutant`` plants a mistake: 'last' (a pool routes to the last maximum), 'leak0' (the gradient passes a maximum of 0), 'neighbour' (a time tap reads the
neighbouring song's row), 'T0' (the first song's T for every song), 'drop' (the last partial slice is dropped), 'add_first' (the first layer's skip is added, not
written), 'instr2' (divided by instr twice), 'swap' (ci and kk swapped in the repack).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
CS_ROWS, SEG_ROWS, SEG, GROUP = 256, 4096, 128, 16


# ------------------------------------------------------------------------------------------------ the rule and exact comparison
def rel_err(x, x64) -> float:
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    den = float(np.abs(x64).max()) if x64.size else 0.0
    num = float(np.abs(x - x64).max()) if x64.size else 0.0
    return 0.0 if num == 0.0 else (math.inf if den == 0.0 else num / den)


def held(x, x64, x32):
    """(verdict, err, err32, ratio to the bound): max|x - x64| / max|x64| at most 4 x the same figure of x32, never asked below 4 * 2^-24"""
    e, e32 = rel_err(x, x64), rel_err(x32, x64)
    bound = max(4.0 * e32, FLOOR)
    return e <= bound, e, e32, e / bound


def same_bits(a, b, zero_sign=True) -> bool:
    """a and b hold the same fp32 bits; zero_sign False: a zero may carry either sign (max(-0, +0) is either by IEEE 754)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    if zero_sign:
        return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    nz = (a != 0) | (b != 0)
    return bool(np.array_equal(a.view(np.uint32)[nz], b.view(np.uint32)[nz]))


def np32(t):
    return t.detach().to(F32).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)


def grad_of(fn, args, wrt, dy, dtype):
    """the gradient of sum(fn(*args) * dy) with respect to args[wrt], all in dtype"""
    a = [torch.as_tensor(np.asarray(v), dtype=dtype) if not isinstance(v, torch.Tensor) else v.to(dtype) for v in args]
    a[wrt] = a[wrt].clone().requires_grad_(True)
    (fn(*a) * torch.as_tensor(np.asarray(dy), dtype=dtype)).sum().backward()
    return a[wrt].grad


# ------------------------------------------------------------------------------------------------ songs
def tables(Ts, I):
    row0, frame0 = np.cumsum([0] + [I * T for T in Ts]), np.cumsum([0] + list(Ts))
    return row0, frame0


def row_map(Ts, I, mutant=None):
    """per row: t, T and the global frame, as a kernel with one thread per row finds them"""
    row0, frame0 = tables(Ts, I)
    t, Tr, fr = [], [], []
    for s, T in enumerate(Ts):
        Tm = Ts[0] if mutant == "T0" else T
        r = np.arange(I * T)
        t.append(r % Tm); Tr.append(np.full(I * T, Tm)); fr.append((frame0[s] + r % Tm) % frame0[-1])
    return np.concatenate(t), np.concatenate(Tr), np.concatenate(fr)


def frame_rows(Ts, I, mutant=None):
    """[frames][I]: the rows of every frame, as a kernel with one thread per frame finds them"""
    row0, _ = tables(Ts, I)
    out = []
    for s, T in enumerate(Ts):
        Tm = Ts[0] if mutant == "T0" else T
        out.append((row0[s] + np.arange(T)[:, None] + np.arange(I)[None, :] * Tm) % row0[-1])
    return np.concatenate(out)


def shift_rows(x, d, Ts, I, mutant=None):
    """out[r] = x[r + d] where t + d lies inside the row's song, else 0 ('neighbour': wherever r + d is a row of the call)"""
    R = x.shape[0]
    t, T, _ = row_map(Ts, I, "T0" if mutant == "T0" else None)
    r = np.arange(R) + d
    ok = (r >= 0) & (r < R) if mutant == "neighbour" else (t + d >= 0) & (t + d < T) & (r >= 0) & (r < R)
    idx = torch.as_tensor(np.clip(r, 0, R - 1))
    okt = torch.as_tensor(ok).reshape((R,) + (1,) * (x.dim() - 1))
    return torch.where(okt, x[idx], torch.zeros((), dtype=x.dtype))


# ------------------------------------------------------------------------------------------------ pool + ReLU
def pool_relu(x, dim, mutant=None):
    """max over the 3 entries of ``dim``, then ReLU: the gradient goes to the first maximal entry, nowhere when the maximum is not positive"""
    if mutant == "last":
        m = x.flip(dim).max(dim).values          # (torch.max(dim) returns, and routes to, the first maximal index)
    else:
        m = x.max(dim).values
    if mutant == "leak0":
        return m * (m >= 0).to(m.dtype)
    return torch.relu(m)


# triples whose route is decidable by construction: (values, the position that takes the gradient or -1)
ROUTES = [((1.0, 1.0, 0.5), 0), ((0.5, 1.0, 1.0), 1), ((1.0, 0.5, 1.0), 0), ((2.0, 2.0, 2.0), 0), ((0.0, -1.0, -2.0), -1), ((-0.0, -1.0, -0.0), -1),
          ((0.0, 0.0, 0.0), -1), ((-1.0, -2.0, -3.0), -1), ((-3.0, -0.5, -0.5), -1), ((3.0, 1.0, 2.0), 0), ((1.0, 3.0, 2.0), 1), ((1.0, 2.0, 3.0), 2),
          ((-1.0, 0.0, 0.25), 2), ((0.25, 0.0, -0.0), 0)]


def built_triples(n, seed):
    """n triples cycling through ROUTES from a random start, each scaled by a power of two: (values [n][3] fp32, route [n] int)"""
    rng = np.random.default_rng(seed)
    k = (np.arange(n) + int(rng.integers(len(ROUTES)))) % len(ROUTES)
    k = rng.permutation(k)
    scale = (2.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    vals = np.array([r[0] for r in ROUTES], np.float32)[k] * scale[:, None]
    return vals, np.array([r[1] for r in ROUTES])[k]


# ------------------------------------------------------------------------------------------------ conv front end
def conv1_pre(feat, w, b, Ts, I, mutant=None):
    """feat [R][128], w [32][15] ([kt][kw]), b [32] -> conv1 before pooling [R][126][32]; 0 outside the song in time"""
    acc = None
    for kt in range(5):
        xs = shift_rows(feat, kt - 2, Ts, I, mutant)
        for kw in range(3):
            term = xs[:, kw:kw + 126, None] * w[:, kt * 3 + kw]
            acc = term if acc is None else acc + term
    return acc + b


def conv1(feat, w, b, Ts, I, mutant=None):
    """k_bt_conv1: c1 [R][42][32] = relu(max_{u<3} conv1_pre[r][3 p + u])"""
    pre = conv1_pre(feat, w, b, Ts, I, mutant if mutant in ("neighbour", "T0") else None)
    return pool_relu(pre.reshape(-1, 42, 3, 32), 2, mutant)


def patch2(c1):
    """k_bt_patch2 (a copy): c1 [R][42][32] -> x2 [R 24][384], x2[r 24 + col][kw 32 + ci] = c1[r][col + kw][ci]"""
    return torch.stack([c1[:, kw:kw + 24] for kw in range(12)], 2).reshape(-1, 384)


def patch3(c2, Ts, I, mutant=None):
    """k_bt_patch3 (a selection): c2 [R][24][64] -> x3 [R 3][1152] = relu(max_{u<3} c2[r + kt - 1][3 (c + kw) + u][ci]) at [kt 384 + kw 64 + ci], 0 outside the song"""
    R = c2.shape[0]
    pooled = pool_relu(c2.reshape(R, 8, 3, 64), 2, mutant)                           # [R][8][64]
    per_kt = []
    for kt in range(3):
        ps = shift_rows(pooled, kt - 1, Ts, I, mutant)
        per_kt.append(torch.stack([ps[:, c:c + 6] for c in range(3)], 1))            # [R][3 c][6 kw][64]
    return torch.stack(per_kt, 2).reshape(R * 3, 1152)                                # [R][c][kt][kw][ci]


def pool3(c3, mutant=None):
    """k_bt_pool3 (a selection): c3 [R][3][256] -> x [R][256]"""
    return pool_relu(c3, 1, mutant)


def patch3_gather_ordered(dx3, Ts, I, mutant=None):
    """the sum k_bt_patch3_bwd forms per pooled cell, numpy fp32 in its order (kt ascending, then c ascending, at most 9 terms): dx3 [R 3][1152] -> g [R][8][64]"""
    R = dx3.shape[0] // 3
    d = np.asarray(dx3, np.float32).reshape(R, 3, 3, 6, 64)                           # [r][c][kt][kw][ci]
    t, T, _ = row_map(Ts, I, "T0" if mutant == "T0" else None)
    g = np.zeros((R, 8, 64), np.float32)
    for kt in range(3):
        rq = np.arange(R) - kt + 1
        ok = (rq >= 0) & (rq < R) if mutant == "neighbour" else (t - kt + 1 >= 0) & (t - kt + 1 < T) & (rq >= 0) & (rq < R)
        src = d[np.clip(rq, 0, R - 1)]
        for c in range(3):
            for pc in range(8):
                kw = pc - c
                if 0 <= kw < 6:
                    g[:, pc] = np.where(ok[:, None], g[:, pc] + src[:, c, kt, kw], g[:, pc])
    return g


def route_ordered(vals, g, mutant=None):
    """bt_pool_route in numpy: vals [..., 3], g [...] -> [..., 3]"""
    vals = np.asarray(vals, np.float32)
    m = vals.max(-1)
    pos = (2 - np.argmax(vals[..., ::-1] == m[..., None], -1)) if mutant == "last" else np.argmax(vals == m[..., None], -1)
    live = m >= 0 if mutant == "leak0" else m > 0
    out = np.zeros(vals.shape, np.float32)
    np.put_along_axis(out, pos[..., None], np.where(live, np.asarray(g, np.float32), np.float32(0))[..., None], -1)
    return out


def patch3_bwd_ordered(c2, dx3, Ts, I, mutant=None):
    """k_bt_patch3_bwd in numpy fp32: c2 [R][24][64], dx3 [R 3][1152] -> dc2 [R][24][64]"""
    R = np.asarray(c2).shape[0]
    g = patch3_gather_ordered(dx3, Ts, I, mutant)
    v = np.asarray(c2, np.float32).reshape(R, 8, 3, 64).transpose(0, 1, 3, 2)        # [r][pc][ci][u]
    return route_ordered(v, g, mutant).transpose(0, 1, 3, 2).reshape(R, 24, 64)


def repack(native, mutant=None):
    """k_bt_repack, dir 0: native [co][ci][kk] -> packed [co][kk][ci]"""
    co, ci, kk = native.shape
    return native.reshape(co, kk, ci) if mutant == "swap" else native.transpose(1, 2).contiguous()


def unpack_add(native, packed, mutant=None):
    """k_bt_repack, dir 1: native [co][ci][kk] + packed [co][kk][ci] (one add per element)"""
    co, ci, kk = native.shape
    return native + (packed.reshape(co, ci, kk) if mutant == "swap" else packed.transpose(1, 2))


# ------------------------------------------------------------------------------------------------ sliced reductions
def colsum(dy, N, out0, mutant=None):
    """launch_bt_colsum: out0 [N] + the column sums of dy [M][>= N]"""
    M = dy.shape[0]
    if mutant == "drop":
        M = M // CS_ROWS * CS_ROWS
    return out0 + dy[:M, :N].sum(0)


def slice_sum_ordered(part, out0, mutant=None):
    """k_bt_slice_sum in numpy fp32: out0 + the slices of part [n][width] added 16 at a time in order, then the groups in order"""
    part = np.asarray(part, np.float32)
    n = part.shape[0] // GROUP * GROUP if mutant == "drop" else part.shape[0]
    tot = np.zeros(part.shape[1], np.float32)
    for q0 in range(0, n, GROUP):
        grp = np.zeros(part.shape[1], np.float32)
        for q in range(q0, min(q0 + GROUP, n)):
            grp = grp + part[q]
        tot = tot + grp
    return np.asarray(out0, np.float32) + tot


def conv_wgrad(dY, X, mutant=None):
    """launch_bt_conv_wgrad: dY [K][M], X [K][N] -> dw [M][N] = dY^T X"""
    K = dY.shape[0]
    if mutant == "drop":
        K = K // SEG_ROWS * SEG_ROWS
    return dY[:K].T @ X[:K]


# ------------------------------------------------------------------------------------------------ the means
def skipacc(skip, tacc, Ts, I, first_layer, mutant=None):
    """k_bt_skipacc: tacc [frames][256] (+)= (sum_i skip[row(i, f)]) / I, instruments ascending (in fp32 this is the kernel's own order)"""
    idx = frame_rows(Ts, I, mutant)
    s = torch.zeros(idx.shape[0], skip.shape[1], dtype=skip.dtype)
    for i in range(I):
        s = s + skip[torch.as_tensor(idx[:, i])]
    m = s / I
    if mutant == "instr2":
        m = m / I
    return m if (first_layer and mutant != "add_first") else tacc + m


def dskip(dx, dtf, Ts, I, mutant=None):
    """k_bt_dskip: dsk[r] = dx[r] + dtf[frame of r]"""
    return dx + dtf[torch.as_tensor(row_map(Ts, I, mutant)[2])]


def hmean(x, Ts, I, mutant=None):
    """k_bt_hmean: hm[f] = (sum_i relu(x[row(i, f)])) / I, instruments ascending"""
    idx = frame_rows(Ts, I, mutant)
    s = torch.zeros(idx.shape[0], x.shape[1], dtype=x.dtype)
    for i in range(I):
        s = s + (x[torch.as_tensor(idx[:, i])] * (x[torch.as_tensor(idx[:, i])] >= 0) if mutant == "leak0" else torch.relu(x[torch.as_tensor(idx[:, i])]))
    m = s / I
    return m / I if mutant == "instr2" else m


def tmean(tacc, Ts, mutant=None):
    """k_bt_tmean: tm[s] = (sum over segments of 128 frames, in order, of the segment's sum of relu(tacc[f]) in frame order) / T"""
    out, f0 = [], 0
    for T in Ts:
        r = tacc[f0:f0 + T] * (tacc[f0:f0 + T] >= 0) if mutant == "leak0" else torch.relu(tacc[f0:f0 + T])
        Tm = Ts[0] if mutant == "T0" else T
        n = T // SEG * SEG if mutant == "drop" else T
        tot = torch.zeros(tacc.shape[1], dtype=tacc.dtype)
        for g0 in range(0, n, SEG):
            seg = torch.zeros(tacc.shape[1], dtype=tacc.dtype)
            for f in range(g0, min(g0 + SEG, n)):
                seg = seg + r[f]
            tot = tot + seg
        out.append(tot / Tm)
        f0 += T
    return torch.stack(out)


def tmean_bwd(tacc, dtm, Ts, I, mutant=None):
    """k_bt_tmean_bwd: autograd of tmean, divided by I once more (dtf is the gradient of every instrument's skip row, which k_bt_skipacc averaged)"""
    g = grad_of(lambda a: tmean(a, Ts, mutant), [tacc], 0, dtm, tacc.dtype) / I
    return g / I if mutant == "instr2" else g


# ------------------------------------------------------------------------------------------------ the two host pipelines
def ffn_params(H, seed):
    rng = np.random.default_rng(seed)
    u = lambda n, *s: rng.uniform(-1 / math.sqrt(n), 1 / math.sqrt(n), s).astype(np.float32)      # noqa: E731
    return [(1 + 0.1 * rng.standard_normal(256)).astype(np.float32), (0.1 * rng.standard_normal(256)).astype(np.float32), u(256, H, 256), u(256, H), u(H, 256, H), u(H, 256)]


def proj_params(seed):
    rng = np.random.default_rng(seed)
    u = lambda n, *s: rng.uniform(-1 / math.sqrt(n), 1 / math.sqrt(n), s).astype(np.float32)      # noqa: E731
    return [(1 + 0.1 * rng.standard_normal(256)).astype(np.float32), (0.1 * rng.standard_normal(256)).astype(np.float32), u(256, 768, 256), u(256, 768)]


def ln_stats(x):
    """mean and 1 / sqrt(var + 1e-5) of every row, in fp64"""
    x = np.asarray(x, np.float64)
    return x.mean(1), 1.0 / np.sqrt(x.var(1) + 1e-5)


def ffn(x, g, b, w1, b1, w2, b2, act):
    """x + W2 act(W1 LN(x) + b1) + b2, act 0 GELU (erf), 1 ReLU"""
    h = F.linear(F.layer_norm(x, (256,), g, b, 1e-5), w1, b1)
    return x + F.linear(F.gelu(h) if act == 0 else torch.relu(h), w2, b2)


def ffn_pre(x, g, b, w1, b1):
    return F.linear(F.layer_norm(x, (256,), g, b, 1e-5), w1, b1)


def ffn_bwd(x, params, dy, act, dtype, mutant=None):
    """[dx, dgain, dbias, dW1, db1, dW2, db2] of sum(ffn(x) dy)"""
    a = [torch.as_tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for v in [x] + list(params)]
    dyt = torch.as_tensor(np.asarray(dy), dtype=dtype)
    (ffn(*a, act) * dyt).sum().backward()
    out = [v.grad for v in a]
    if mutant == "drop":                                                              # the bias sums without the last partial slice of rows
        n = dyt.shape[0] // CS_ROWS * CS_ROWS
        out[6] = dyt[:n].sum(0)
    return out


def proj(x, g, b, w, bias):
    return F.linear(F.layer_norm(x, (256,), g, b, 1e-5), w, bias)


def proj_bwd(x, params, dqkv, dtype):
    """[dx, dgain, dbias, dW, db] of sum(proj(x) dqkv)"""
    a = [torch.as_tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for v in [x] + list(params)]
    (proj(*a) * torch.as_tensor(np.asarray(dqkv), dtype=dtype)).sum().backward()
    return [v.grad for v in a]


# ------------------------------------------------------------------------------------------------ the inputs both test files use
SONGS = [2, 1, 7]                  # T = 1 and T = 2: every time tap is out of range for some song; one T >= 6; the first song's T is no other song's
INSTR = [1, 3, 5, 8]
TMEAN_SONGS = [129, 1, 127, 128, 257]
COLSUM_M = [1, 8, 255, 256, 257, 16 * 256 + 1]
# (N, ld, base column): ld 768 from column 0 and from column 512 are proj_backward's query- and value-bias calls; ld > base + N puts OUTSIDE right of the columns
COLSUM_FORMS = [(256, 256, 0), (256, 768, 0), (256, 768, 512), (2, 2, 0), (3, 3, 0), (64, 64, 0), (33, 33, 0), (33, 40, 0)]
TEMPO_M = list(range(1, 9))        # songs of a call: the tempo bias is launch_bt_colsum over M = n_seq rows of N = 300 (the eight sub-slices partly filled)
WGRAD_CASES = [(24, 40, 4095), (24, 40, 4096), (24, 40, 4097), (24, 40, 16 * 4096 + 1), (64, 384, 4097)]
PIPE_ROWS = [1, 5, 257, 16 * 256 + 1]
OUTSIDE = 1e30                     # what a column outside [0, N) holds: seen at once if read


MARGIN = 1e-6                      # of a random pool triple: top-2 gap and distance of the maximum from the ReLU's kink


def random_triples(seed0, shape, axis):
    """the margin selection of test_conv1_weight_reduction_at_slice_edges: the first of 50 seeds whose every triple along ``axis`` has a top-2 gap and a distance of
    its maximum from 0 above MARGIN -> (values, the margin found).  These values reach the kernel as they are, so any margin above 0 makes the route decidable and the
    comparison exact; MARGIN only keeps the case away from a tie by a stated distance."""
    for seed in range(seed0, seed0 + 50):
        a = normal(seed, *shape)
        top = np.sort(a.astype(np.float64), axis)
        margin = float(min((top.take(2, axis) - top.take(1, axis)).min(), np.abs(top.take(2, axis)).min()))
        if margin > MARGIN:
            break
    return a, margin


def rows_of(Ts, I):
    return I * sum(Ts)


def normal(seed, *shape, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def colsum_case(M, N, ld, base, seed=0):
    """(dy [M][ld] with OUTSIDE outside the N columns from `base`, out0 [N] non-zero)"""
    rng = np.random.default_rng(1000 * M + 10 * N + seed)
    dy = np.full((M, ld), OUTSIDE, np.float32)
    dy[:, base:base + N] = rng.standard_normal((M, N)) + 0.25
    return dy, rng.standard_normal(N).astype(np.float32)


def wgrad_case(M, N, K):
    rng = np.random.default_rng(K + M)
    return rng.standard_normal((K, M)).astype(np.float32), (rng.standard_normal((K, N)) + 0.25).astype(np.float32)


def tmean_case(seed=5):
    """tacc over TMEAN_SONGS; columns 0 .. 7 are non-positive in every frame (zeros, -0.0 and negatives)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((sum(TMEAN_SONGS), 256)).astype(np.float32)
    a[:, :8] = -np.abs(a[:, :8])
    a[::3, :4] = 0.0
    a[1::3, :4] = -0.0
    return a


def means_case(I, seed=0):
    """x [rows][256] with exact zeros and -0.0 planted in column 0 and 1"""
    x = normal(100 + I + seed, rows_of(SONGS, I), 256)
    x[:, 0] = 0.0
    x[:, 1] = -0.0
    return x


def pipe_case(R, H, act, seed=0):
    """x, dy and the parameters of a feed-forward sublayer over R rows"""
    rng = np.random.default_rng(7 * R + H + act + seed)
    return (rng.standard_normal((R, 256)) * rng.uniform(0.5, 2.0, (R, 1)) + 0.3).astype(np.float32), rng.standard_normal((R, 256)).astype(np.float32), ffn_params(H, R + H)


# ------------------------------------------------------------------------------------------------ the checks, on anything that plays the device
class Report:
    """every figure is printed when it is measured; done() fails on the first that missed, after all of them were shown"""

    def __init__(self, name):
        self.name, self.failed, self.worst = name, [], 0.0

    def hold(self, what, x, x64, x32):
        ok, e, e32, ratio = held(np32(x), np32_64(x64), np32_64(x32))
        self.worst = max(self.worst, ratio)
        print(f"[measured] {self.name} {what}: err {e:.3e}, fp32 torch {e32:.3e}, {ratio:.3f} of the bound" + ("" if ok else "   <-- MISSED"))
        if not ok:
            self.failed.append((what, e, e32))

    def exact(self, what, got, want, zero_sign=True):
        ok = same_bits(got, want, zero_sign)
        if not ok:
            g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
            n = int((g != w).sum()) if g.shape == w.shape else -1
            print(f"[measured] {self.name} {what}: {n} floats differ from the exact expectation   <-- MISSED")
            self.failed.append((what, n))

    def true(self, what, cond):
        if not cond:
            print(f"[measured] {self.name} {what}: does not hold   <-- MISSED")
            self.failed.append((what,))

    def done(self):
        print(f"[measured] {self.name}: largest ratio to the bound {self.worst:.3f}")
        assert not self.failed, self.failed


def np32_64(t):
    return t.detach().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def T(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


class RefDevice:
    """the fp32 references in the device's place (numpy fp32 in and out), with a planted mutant or none"""

    def __init__(self, mutant=None):
        self.m = mutant

    def conv1(self, feat, w, b, Ts, I): return np32(conv1(T(feat, F32), T(w, F32), T(b, F32), Ts, I, self.m))
    def patch2(self, c1, Ts, I): return np32(patch2(T(c1, F32)))
    def patch3(self, c2, Ts, I): return np32(patch3(T(c2, F32), Ts, I, self.m))
    def pool3(self, c3, Ts, I): return np32(pool3(T(c3, F32), self.m))
    def pool3_bwd(self, c3, dx, Ts, I): return np32(grad_of(lambda a: pool3(a, self.m), [c3], 0, dx, F32))
    def patch3_bwd(self, c2, dx3, Ts, I): return patch3_bwd_ordered(c2, dx3, Ts, I, self.m)
    def repack(self, native): return np32(repack(T(native, F32), self.m))
    def unpack_add(self, native, packed): return np32(unpack_add(T(native, F32), T(packed, F32), self.m))
    def colsum(self, dy, ld, M, N, base, out0): return np32(colsum(T(dy[:, base:], F32), N, T(out0, F32), self.m))
    def slice_sum(self, part, out0): return slice_sum_ordered(part, out0, self.m)
    def conv_wgrad(self, dY, X): return np32(conv_wgrad(T(dY, F32), T(X, F32), self.m))
    def skipacc(self, skip, tacc, Ts, I, first): return np32(skipacc(T(skip, F32), T(tacc, F32), Ts, I, first, self.m))
    def dskip(self, dx, dtf, Ts, I): return np32(dskip(T(dx, F32), T(dtf, F32), Ts, I, self.m))
    def hmean(self, x, Ts, I): return np32(hmean(T(x, F32), Ts, I, self.m))
    def hmean_bwd(self, x, dhm, Ts, I): return np32(grad_of(lambda a: hmean(a, Ts, I, self.m), [x], 0, dhm, F32))
    def tmean(self, tacc, Ts, I): return np32(tmean(T(tacc, F32), Ts, self.m))
    def tmean_bwd(self, tacc, dtm, Ts, I): return np32(tmean_bwd(T(tacc, F32), dtm, Ts, I, self.m))
    def relu(self, x): return np32(torch.relu(T(x, F32)))
    def relu_bwd(self, x, dy): return np.where(np.asarray(x) >= 0 if self.m == "leak0" else np.asarray(x) > 0, dy, np.float32(0)).astype(np.float32)
    def ffn_bwd(self, x, params, dy, act, H): return [np32(g) for g in ffn_bwd(x, params, dy, act, F32, self.m)]
    def proj_bwd(self, x, params, dqkv, dx0):
        g = proj_bwd(x, params, dqkv, F32)
        return [np32(T(dx0, F32) + g[0])] + [np32(v) for v in g[1:]] + [None]


def _song_alone(Ts, I, arrays, per_row):
    """the rows of each song cut out of row-major arrays: yields (s, T, row slice, [array of the song alone ...])"""
    r0 = 0
    for s, Tn in enumerate(Ts):
        n = I * Tn
        yield s, Tn, slice(r0, r0 + n), [a[r0 * k:(r0 + n) * k] for a, k in zip(arrays, per_row)]
        r0 += n


def check_conv1(rep, dev, I):
    """random weights under the rule; each song alone gives the bits it gives inside the batch; a built input (one unit tap per channel, no bias: the convolution
    copies) whose pooled triples cover ROUTES, exact"""
    Ts, R = SONGS, rows_of(SONGS, I)
    rng = np.random.default_rng(I)
    feat = rng.uniform(-80, 0, (R, 128)).astype(np.float32)
    w, b = (0.1 * rng.uniform(-0.26, 0.26, (32, 15))).astype(np.float32), rng.uniform(0.5, 2.5, 32).astype(np.float32)
    got = dev.conv1(feat, w, b, Ts, I)
    rep.hold(f"conv1 I={I}", got, conv1(T(feat, F64), T(w, F64), T(b, F64), Ts, I), conv1(T(feat, F32), T(w, F32), T(b, F32), Ts, I))
    for s, Tn, rs, (f,) in _song_alone(Ts, I, [feat], [1]):
        rep.exact(f"conv1 I={I} song {s} alone", dev.conv1(f, w, b, [Tn], I), got[rs])
    vals, _ = built_triples(R * 42, 10 + I)
    feat = np.zeros((R, 128), np.float32)
    feat[:, :126] = vals.reshape(R, 126)
    feat[:, 126:] = 64.0                                                              # read by kw = 1, 2 of the last triple only
    w = np.zeros((32, 15), np.float32)
    for co in range(32):
        w[co, (co % 5) * 3 + co % 3] = 1.0
    want = np.zeros((R, 42, 32), np.float32)
    for co in range(32):
        xs = np32(shift_rows(T(feat, F32), co % 5 - 2, Ts, I))
        want[:, :, co] = np.maximum(xs[:, co % 3:co % 3 + 126].reshape(R, 42, 3).max(2), 0)
    rep.exact(f"conv1 I={I} built routes", dev.conv1(feat, w, np.zeros(32, np.float32), Ts, I), want, zero_sign=False)


def check_patches_and_pool(rep, dev, I):
    """patch2, patch3 and pool3 are copies and selections: bit for bit, on random inputs and on built triples; patch3 per song alone"""
    Ts, R = SONGS, rows_of(SONGS, I)
    c1 = normal(20 + I, R, 42, 32)
    rep.exact(f"patch2 I={I}", dev.patch2(c1, Ts, I), np32(patch2(T(c1, F32))))
    for name, c2 in (("random", normal(30 + I, R, 24, 64)), ("built", built_triples(R * 8 * 64, 31 + I)[0].reshape(R, 8, 64, 3).transpose(0, 1, 3, 2).reshape(R, 24, 64))):
        got = dev.patch3(c2, Ts, I)
        rep.exact(f"patch3 I={I} {name}", got, np32(patch3(T(c2, F32), Ts, I)), zero_sign=name == "random")
        for s, Tn, rs, (a,) in _song_alone(Ts, I, [c2], [1]):
            rep.exact(f"patch3 I={I} {name} song {s} alone", dev.patch3(a, [Tn], I), got[rs.start * 3:rs.stop * 3], zero_sign=name == "random")
    for name, c3 in (("random", normal(40 + I, R, 3, 256)), ("built", built_triples(R * 256, 41 + I)[0].reshape(R, 256, 3).transpose(0, 2, 1))):
        rep.exact(f"pool3 I={I} {name}", dev.pool3(np.ascontiguousarray(c3), Ts, I), np32(pool3(T(c3, F32))), zero_sign=name == "random")


def check_pool3_bwd(rep, dev, I):
    """built triples: the gradient sits at the position ROUTES states and nowhere else, exact; random triples under the margin selection (random_triples: the margin is
    asserted) against fp64 autograd, exact -- the inputs reach the kernel as they are, so fp64 decides every route as fp32 does"""
    Ts, R = SONGS, rows_of(SONGS, I)
    vals, pos = built_triples(R * 256, 50 + I)
    c3 = np.ascontiguousarray(vals.reshape(R, 256, 3).transpose(0, 2, 1))
    dx = normal(51 + I, R, 256)
    want = np.zeros((R, 256, 3), np.float32)
    live = pos.reshape(R, 256) >= 0
    np.put_along_axis(want, np.maximum(pos, 0).reshape(R, 256, 1), np.where(live, dx, np.float32(0))[..., None], -1)
    rep.exact(f"pool3_bwd I={I} built", dev.pool3_bwd(c3, dx, Ts, I), want.transpose(0, 2, 1))
    c3, margin = random_triples(1000 * I, (R, 3, 256), 1)
    rep.true(f"pool3_bwd I={I}: the random triples have a margin {margin:.2e} > {MARGIN}", margin > MARGIN)
    rep.exact(f"pool3_bwd I={I} random", dev.pool3_bwd(c3, dx, Ts, I), np32(grad_of(pool3, [c3], 0, dx, F64)))


def check_patch3_bwd(rep, dev, I):
    """built and random c2 against the ordered fp32 restatement, bit for bit; per pooled column; rows outside a song's time taps add nothing (each song alone gives
    the same bits); under the rule against fp64 autograd.  The random c2 comes from the margin selection (random_triples), its margin asserted"""
    Ts, R = SONGS, rows_of(SONGS, I)
    dx3 = normal(60 + I, R * 3, 1152)
    c2_random, margin = random_triples(2000 * I, (R, 8, 3, 64), 2)                    # the pooled triples are columns 3 pc .. 3 pc + 2
    rep.true(f"patch3_bwd I={I}: the random triples have a margin {margin:.2e} > {MARGIN}", margin > MARGIN)
    c2_random = c2_random.reshape(R, 24, 64)
    for name, c2 in (("built", built_triples(R * 8 * 64, 61 + I)[0].reshape(R, 8, 64, 3).transpose(0, 1, 3, 2).reshape(R, 24, 64)), ("random", c2_random)):
        c2 = np.ascontiguousarray(c2)
        got, want = dev.patch3_bwd(c2, dx3, Ts, I), patch3_bwd_ordered(c2, dx3, Ts, I)
        for pc in range(8):                                                           # columns 0 and 7 have one contributing (c, kw), 2 .. 5 three
            rep.exact(f"patch3_bwd I={I} {name} pooled column {pc}", got[:, 3 * pc:3 * pc + 3], want[:, 3 * pc:3 * pc + 3])
        rep.hold(f"patch3_bwd I={I} {name}", got, grad_of(lambda a: patch3(a, Ts, I), [c2], 0, dx3, F64), grad_of(lambda a: patch3(a, Ts, I), [c2], 0, dx3, F32))
        for s, Tn, rs, (a, g) in _song_alone(Ts, I, [c2, dx3], [1, 3]):
            rep.exact(f"patch3_bwd I={I} {name} song {s} alone", dev.patch3_bwd(a, g, [Tn], I), got[rs])


def check_repack(rep, dev):
    for co, ci, kk in ((64, 32, 12), (256, 64, 18), (5, 7, 3)):
        native, packed = normal(co + ci, co, ci, kk), normal(co + kk, co, kk, ci)
        rep.exact(f"repack {co}x{ci}x{kk} to packed", dev.repack(native), np32(repack(T(native, F32))))
        rep.exact(f"repack {co}x{ci}x{kk} add back", dev.unpack_add(native, packed), np32(unpack_add(T(native, F32), T(packed, F32))))


def check_colsum(rep, dev, M):
    for N, ld, base in COLSUM_FORMS:
        dy, out0 = colsum_case(M, N, ld, base)
        rep.hold(f"colsum M={M} N={N} ld={ld}", dev.colsum(dy, ld, M, N, base, out0), colsum(T(dy[:, base:], F64), N, T(out0, F64)), colsum(T(dy[:, base:], F32), N, T(out0, F32)))


def check_colsum_tempo(rep, dev):
    """N = 300 at every M = 1 .. 8: the tempo head's bias over the songs of a call"""
    for M in TEMPO_M:
        dy, out0 = colsum_case(M, 300, 300, 0)
        rep.hold(f"colsum M={M} N=300 ld=300", dev.colsum(dy, 300, M, 300, 0, out0), colsum(T(dy, F64), 300, T(out0, F64)), colsum(T(dy, F32), 300, T(out0, F32)))


def check_slice_sum(rep, dev):
    for n, width in ((1, 5), (15, 33), (16, 256), (17, 256), (33, 300), (16 * 16 + 1, 64)):
        part, out0 = normal(n + width, n, width), normal(n, width)
        rep.exact(f"slice_sum {n} slices of {width}", dev.slice_sum(part, out0), slice_sum_ordered(part, out0))


def check_conv_wgrad(rep, dev, M, N, K):
    dY, X = wgrad_case(M, N, K)
    rep.hold(f"conv_wgrad {M}x{N} K={K}", dev.conv_wgrad(dY, X), conv_wgrad(T(dY, F64), T(X, F64)), conv_wgrad(T(dY, F32), T(X, F32)))


def check_skipacc(rep, dev, I):
    """three successive layers, the first on a tacc of sentinels: bit for bit against the restatement (instruments ascending), and under the rule"""
    Ts = SONGS
    Fr = sum(Ts)
    tacc = np.full((Fr, 256), 12345.0, np.float32)
    t32, t64 = T(tacc, F32), T(tacc, F64)
    for layer in range(3):
        skip = normal(70 + 10 * I + layer, rows_of(Ts, I), 256)
        tacc = dev.skipacc(skip, tacc, Ts, I, 1 if layer == 0 else 0)
        t32, t64 = skipacc(T(skip, F32), t32, Ts, I, layer == 0), skipacc(T(skip, F64), t64, Ts, I, layer == 0)
        rep.exact(f"skipacc I={I} layer {layer}", tacc, np32(t32))
        rep.hold(f"skipacc I={I} layer {layer}", tacc, t64, t32)


def check_means(rep, dev, I):
    """dskip (one add: exact), hmean (exact against the ordered restatement, and under the rule), hmean_bwd (mask exact, values under the rule)"""
    Ts = SONGS
    R, Fr = rows_of(Ts, I), sum(Ts)
    dx, dtf = normal(80 + I, R, 256), normal(81 + I, Fr, 256)
    rep.exact(f"dskip I={I}", dev.dskip(dx, dtf, Ts, I), np32(dskip(T(dx, F32), T(dtf, F32), Ts, I)))
    x, dhm = means_case(I), normal(82 + I, Fr, 256)
    got = dev.hmean(x, Ts, I)
    rep.exact(f"hmean I={I}", got, np32(hmean(T(x, F32), Ts, I)))
    rep.hold(f"hmean I={I}", got, hmean(T(x, F64), Ts, I), hmean(T(x, F32), Ts, I))
    got = dev.hmean_bwd(x, dhm, Ts, I)
    rep.true(f"hmean_bwd I={I}: zero exactly where x <= 0", not got[~(x > 0)].any() and bool((got[x > 0] != 0).all()))
    rep.hold(f"hmean_bwd I={I}", got, grad_of(lambda a: hmean(a, Ts, I), [x], 0, dhm, F64), grad_of(lambda a: hmean(a, Ts, I), [x], 0, dhm, F32))


def check_tmean(rep, dev, I):
    """songs of 129, 1, 127, 128 and 257 frames; the forward reads frames only (instr reaches it through the song tables), the backward divides by instr"""
    Ts = TMEAN_SONGS
    tacc, dtm = tmean_case(), normal(90 + I, len(Ts), 256)
    got = dev.tmean(tacc, Ts, I)
    t32 = tmean(T(tacc, F32), Ts)
    rep.exact(f"tmean I={I}", got, np32(t32))
    rep.hold(f"tmean I={I}", got, tmean(T(tacc, F64), Ts), t32)
    rep.true(f"tmean I={I}: a column non-positive in every frame is exactly 0", not got[:, :8].any())
    got = dev.tmean_bwd(tacc, dtm, Ts, I)
    rep.true(f"tmean_bwd I={I}: zero exactly where tacc <= 0", not got[~(tacc > 0)].any() and bool((got[tacc > 0] != 0).all()))
    rep.hold(f"tmean_bwd I={I}", got, tmean_bwd(T(tacc, F64), dtm, Ts, I), tmean_bwd(T(tacc, F32), dtm, Ts, I))


def check_relu(rep, dev):
    x = normal(95, 1000)
    x[:10], x[10:20] = 0.0, -0.0
    dy = normal(96, 1000)
    rep.exact("relu", dev.relu(x), np.maximum(x, np.float32(0)), zero_sign=False)
    rep.exact("relu_bwd", dev.relu_bwd(x, dy), np.where(x > 0, dy, np.float32(0)))


FFN_NAMES = ["dx", "norm.weight", "norm.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]
PROJ_NAMES = ["dx", "norm.weight", "norm.bias", "weight", "bias"]


def check_ffn_bwd(rep, dev, R, H, act):
    x, dy, params = pipe_case(R, H, act)
    got = dev.ffn_bwd(x, params, dy, act, H)
    g64, g32 = ffn_bwd(x, params, dy, act, F64), ffn_bwd(x, params, dy, act, F32)
    for n, a, b, c in zip(FFN_NAMES, got, g64, g32):
        rep.hold(f"ffn_bwd R={R} H={H} act={act} {n}", a, b, c)


def check_proj_bwd(rep, dev, R):
    x, _, _ = pipe_case(R, 256, 2)
    params, dqkv, dx0 = proj_params(R), normal(R, R, 768), normal(R + 1, R, 256)
    got = dev.proj_bwd(x, params, dqkv, dx0)                                          # dx0 on entry: the launch adds
    g64, g32 = proj_bwd(x, params, dqkv, F64), proj_bwd(x, params, dqkv, F32)
    g64[0], g32[0] = T(dx0, F64) + g64[0], T(dx0, F32) + g32[0]
    for n, a, b, c in zip(PROJ_NAMES, got, g64, g32):
        if n == "bias":                                                               # the key third is left alone (its gradient is identically zero)
            a, b, c = (np.concatenate([np32_64(v).reshape(-1)[:256], np32_64(v).reshape(-1)[512:]]) for v in (a, b, c))
        rep.hold(f"proj_bwd R={R} {n}", a, b, c)
    if got[5] is not None:
        rep.true(f"proj_bwd R={R}: the key-bias slice keeps every bit", bool(got[5]))
