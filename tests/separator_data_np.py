"""Separator training data and decoder dropout (DESIGN.md 4o and the dropout paragraph of 4n), restated: Philox4x32-10 in numpy integers, the dropout mask, the
augmenting gather in a dtype of the caller's choice (fp64 is the truth, fp32 the yardstick a device tensor is measured against), and the training-mode U-Net of
tests/separator_train_np.py with the masks applied (its convolutions, norm and loss are imported, not copied).

``variant`` switches ONE deliberate mistake on: "no_backward_mask" (the mask scales the forward only; the gradient passes as if nothing was dropped) and
"mask_before_norm" (the drop is applied to the norm's input, so the batch statistics see it)."""
from __future__ import annotations

import math

import numpy as np
import torch

import separator_np as sp
import separator_train_np as st
from separator_train_np import conv_down, conv_up, head, loss_fn, norm  # noqa: F401  (the pieces the masked forward is made of)

LEVELS = sp.LEVELS
DROP_LEVELS = 3
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays; every product in uint64"""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK32), p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def drop_threshold(p: float) -> int:
    return min(2 ** 32 - 1, int(math.floor((1.0 - p) * 2.0 ** 32)))


def drop_scale(p: float) -> np.float32:
    """1 / (1 - p) formed in double and rounded once"""
    return np.float32(1.0 / (1.0 - p))


def dropout_keep(n: int, j: int, call: int, seed: int, p: float) -> np.ndarray:
    """keep [n] (bool) for flat elements 0 .. n - 1 of y_j: counter (lo32(e >> 2), hi32(e >> 2), j, call), key (lo32(seed), hi32(seed)), word e & 3 < thr"""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), j, call & MASK32), (seed & MASK32, (seed >> 32) & MASK32))
    flat = np.stack(words, axis=1).reshape(-1)[:n]
    return flat < np.uint32(drop_threshold(p))


def dropout_apply(y: np.ndarray, j: int, call: int, seed: int, p: float) -> np.ndarray:
    """keep ? y * s : 0 on a contiguous array of y's dtype"""
    keep = dropout_keep(y.size, j, call, seed, p).reshape(y.shape)
    return np.where(keep, y * y.dtype.type(drop_scale(p)), y.dtype.type(0))


# ---------------------------------------------------------------------------------------------- the gather
def stretched_sizes(T, F, a, q):
    return int(math.floor(T * float(a))), int(math.floor(F * float(q)))


def axis_positions(n_out: int, n_in: int, dtype):
    """align-corners positions of ``n_out`` points over ``n_in``: (i0, i1, w) with the position and the weight formed in fp64; the fp32 yardstick rounds the weight
    once to fp32 as the device does, the fp64 truth keeps it"""
    pos = np.arange(n_out, dtype=np.float64) * float(n_in - 1) / float(n_out - 1)
    i0 = np.minimum(np.floor(pos).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), (pos - i0).astype(dtype)


def lerp(u, v, w, dtype):
    """fmaf(w, v - u, u) in ``dtype``: the difference rounded, then one rounding of the fused multiply-add (a float32 product is exact in double)"""
    if dtype == np.float64:
        return w.astype(np.float64) * (v - u) + u
    d = (v - u).astype(np.float32)
    return (w.astype(np.float64) * d.astype(np.float64) + u.astype(np.float64)).astype(np.float32)


def window(S, Tf: int, T: int, t0: int, dtype):
    """frames t0 .. t0 + T - 1 of S [K][frames][F][C], zeros from Tf on"""
    W = np.zeros((S.shape[0], T) + S.shape[2:], dtype)
    n = max(0, min(T, Tf - t0))
    W[:, :n] = S[:, t0:t0 + n]
    return W


def gather(S, Tf: int, T: int, t0: int, a: float, q: float, dtype=np.float64):
    """one unit: S [K][frames][F][C] (K = 1 + I sources) -> [K][T][F][C]; the time axis first, then frequency"""
    W = window(S, Tf, T, t0, dtype)
    K, _, F, C = W.shape
    Tp, Fp = stretched_sizes(T, F, a, q)
    assert Tp >= 2 and Fp >= 2
    i0, i1, wt = axis_positions(Tp, T, dtype)
    R = lerp(W[:, i0], W[:, i1], wt[None, :, None, None], dtype)
    out = np.zeros((K, T, F, C), dtype)
    if Tp >= T:
        off = (Tp - T) // 2
        out[:] = R[:, off:off + T]
    else:
        off = (T - Tp) // 2
        out[:, off:off + Tp] = R
    j0, j1, wf = axis_positions(Fp, F, dtype)
    nf = min(F, Fp)
    res = np.zeros((K, T, F, C), dtype)
    res[:, :, :nf] = lerp(out[:, :, j0[:nf]], out[:, :, j1[:nf]], wf[None, None, :nf, None], dtype)
    return res


def batch(tracks, draws, T: int, dtype=np.float64):
    """tracks: [(S [K][frames][F][C], Tf)], draws: [(track, t0, a, q)] -> (mix [B][T][F][C], target [I][B][T][F][C])"""
    units = [gather(tracks[k][0], tracks[k][1], T, t0, a, q, dtype) for k, t0, a, q in draws]
    allk = np.stack(units, axis=1)
    return allk[0], allk[1:]


# ---------------------------------------------------------------------------------------------- the U-Net with dropout
def unet_train_dropout(mix, P, name: str, inst: int, n_instr: int, bn_eps: float, p: float, seed: int, call: int, frozen: bool = False, stats=None, variant=None):
    """separator_train_np.unet_train with the drop after the norm of decoder levels 1 .. 3.  The mask of y_j [B][I][pos][C] is cut at instrument ``inst``."""
    x, pres = mix, []
    for l in range(1, LEVELS + 1):
        pre = conv_down(x, P[f"{name}.conv{l}.weight"], P[f"{name}.conv{l}.bias"])
        x = sp.elu(norm(pre, P, f"{name}.bn{l}", bn_eps, frozen, stats))
        pres.append(pre)
    up = None
    for j in range(1, LEVELS + 1):
        skip = pres[LEVELS - j]
        xin = skip if up is None else torch.cat([skip, up], dim=-1)
        v = conv_up(xin, P[f"{name}.deconv{j}.weight"], P[f"{name}.deconv{j}.bias"])
        act = sp.elu(v)
        m = None
        if p > 0 and j <= DROP_LEVELS:
            B, H, Wd, Cc = act.shape
            keep = dropout_keep(B * n_instr * H * Wd * Cc, j, call, seed, p).reshape(B, n_instr, H, Wd, Cc)[:, inst]
            m = torch.from_numpy(np.where(keep, drop_scale(p), np.float32(0))).to(act.dtype)
        if m is not None and variant == "mask_before_norm":
            act = act * m
        out = norm(act, P, f"{name}.bn{LEVELS + j}", bn_eps, frozen, stats)
        if m is not None and variant == "no_backward_mask":
            out = out + (out * m - out).detach()
        elif m is not None and variant != "mask_before_norm":
            out = out * m
        up = out
    return head(up, P[f"{name}.head.weight"], P[f"{name}.head.bias"])


def forward(mix, P, cfg, p: float, seed: int, call: int, frozen: bool = False, stats=None, variant=None):
    """mix [B][T][F][C] -> logits [I][B][T][F][C]"""
    I = len(cfg.instruments)
    return torch.stack([unet_train_dropout(mix, P, name, i, I, cfg.bn_eps, p, seed, call, frozen, stats, variant) for i, name in enumerate(cfg.instruments)])


def loss_and_grads(mix, target, state, cfg, dtype, p: float, seed: int, call: int, frozen: bool = False, variant=None):
    """separator_train_np.loss_and_grads with dropout -> (loss, {key: gradient}, {norm key: (batch mean, batch var)})"""
    P = st.params(state, dtype)
    stats = {}
    L = loss_fn(forward(mix.to(dtype), P, cfg, p, seed, call, frozen, stats, variant), mix.to(dtype), target.to(dtype))
    keys = [k for k in P if P[k].requires_grad]
    gs = torch.autograd.grad(L, [P[k] for k in keys], allow_unused=True)
    return L.detach(), {k: (g if g is not None else torch.zeros_like(P[k])) for k, g in zip(keys, gs)}, stats


def train_steps(batches, state, cfg, dtype, lr: float, p: float, seed: int, betas=(0.9, 0.999), eps: float = 1e-8):
    """one Adam step per (mix, target) of ``batches`` with dropout at call counters 0, 1, .. -> the final state as tensors of ``dtype``"""
    cur = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype) for k, v in state.items()}
    mom = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in cur.items() if k.endswith(st.TRAINABLE)}
    for s, (mix, target) in enumerate(batches, start=1):
        P = {k: (t.clone().requires_grad_(True) if k in mom else t) for k, t in cur.items()}
        stats = {}
        L = loss_fn(forward(mix.to(dtype), P, cfg, p, seed, s - 1, False, stats), mix.to(dtype), target.to(dtype))
        keys = list(mom)
        gs = torch.autograd.grad(L, [P[k] for k in keys], allow_unused=True)
        for k, g in zip(keys, gs):
            g = g if g is not None else torch.zeros_like(cur[k])
            cur[k], m, v = st.adam_step(cur[k], g, mom[k][0], mom[k][1], s, lr, betas, eps)
            mom[k] = (m, v)
        for key, (mean, var) in stats.items():
            cur[f"{key}.mean"] = st.running_update(cur[f"{key}.mean"], mean)
            cur[f"{key}.var"] = st.running_update(cur[f"{key}.var"], var)
    return cur


def frozen_loss(mix, target, cur, cfg, dtype) -> float:
    """trainer.loss(): the running statistics, no dropout"""
    P = {k: t.to(dtype) for k, t in cur.items()}
    with torch.no_grad():
        return float(loss_fn(st.forward(mix.to(dtype), P, cfg, frozen=True), mix.to(dtype), target.to(dtype)))


# ---------------------------------------------------------------------------------------------- the learning scenario of the tests
def two_band_stems(N: int, seed: int, channels: int = 2, sr: int = 44100):
    """two sources in disjoint bands (bins of n_fft = 1024 below 24 and from 40 up, so that a shift of a semitone keeps them apart): sums of amplitude-modulated
    partials -> ([C][N], [C][N]) float32"""
    r = np.random.default_rng(seed)
    t = np.arange(N) / sr
    out = []
    for lo, hi in ((150.0, 950.0), (1800.0, 2500.0)):
        x = np.zeros((channels, N))
        for _ in range(6):
            f, rate, ph = r.uniform(lo, hi), r.uniform(1.0, 6.0), r.uniform(0, 2 * np.pi, channels)
            amp = r.uniform(0.05, 0.2) * (0.55 + 0.45 * np.sin(2 * np.pi * rate * t + r.uniform(0, 2 * np.pi)))
            x += amp * np.sin(2 * np.pi * f * t[None, :] + ph[:, None])
        out.append(np.ascontiguousarray(x, np.float32))
    return out[0], out[1]
