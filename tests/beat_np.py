"""A plain-numpy restatement of Demixed_DilatedTransformerModel.forward for ONE song (tests only), written from the model's description: conv front end, dilated
5-tap attention with its head / offset table and head 7's key quirk, instrument attention after layers 3-5, beat and tempo heads.  fp64 throughout.

forward(sd, feat[instr][T][128], nlayers=9) -> dict(logits [T][ntoken], tempo [300], front [instr][T][D], layer0 [instr][T][D])
"""
from __future__ import annotations

import math

import numpy as np

OFFSETS = [[-2, -1, 0, 1, 2]] * 4 + [[-4, -3, -2, -1, 0], [-3, -2, -1, 0, 1], [-1, 0, 1, 2, 3], [0, 1, 2, 3, 4]]


def _ln(x, g, b, eps=1e-5):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def _erf(x):
    try:
        from scipy.special import erf
        return erf(x)
    except ImportError:
        import torch
        return torch.erf(torch.from_numpy(x)).numpy()


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def _conv_time(x, w, b, pad_t):
    """x [Cin][T][W], w [Cout][Cin][kt][kw], zero padding pad_t in time -> [Cout][T][W - kw + 1]"""
    cin, T, W = x.shape
    co, _, kt, kw = w.shape
    xp = np.zeros((cin, T + 2 * pad_t, W))
    xp[:, pad_t:pad_t + T] = x
    Wo = W - kw + 1
    out = np.zeros((co, T, Wo)) + b[:, None, None]
    for a in range(kt):
        for c in range(kw):
            patch = xp[:, a:a + T, c:c + Wo]                                  # [Cin][T][Wo]
            out += np.einsum("oi,itw->otw", w[:, :, a, c], patch)
    return out


def _pool3(x):
    n = x.shape[-1] // 3
    return x[..., :3 * n].reshape(*x.shape[:-1], n, 3).max(-1)


def front_end(sd, feat):
    """[instr][T][128] -> tokens [instr][T][D]"""
    out = []
    for i in range(feat.shape[0]):
        x = feat[i][None].astype(np.float64)
        x = np.maximum(_pool3(_conv_time(x, sd["conv1.weight"].astype(np.float64), sd["conv1.bias"].astype(np.float64), 2)), 0)
        x = np.maximum(_pool3(_conv_time(x, sd["conv2.weight"].astype(np.float64), sd["conv2.bias"].astype(np.float64), 0)), 0)
        x = np.maximum(_pool3(_conv_time(x, sd["conv3.weight"].astype(np.float64), sd["conv3.bias"].astype(np.float64), 1)), 0)
        out.append(x[:, :, 0].T)                                                 # [T][D]
    return np.stack(out)


def dilated_attention(p, x, layer):
    """x [instr][T][D] (already LayerNorm'ed) -> attention output [instr][T][D]"""
    I, T, D = x.shape
    nh, hd, s = 8, D // 8, 2 ** layer
    q = x @ p["self_attn.query.weight"].T + p["self_attn.query.bias"]
    k = x @ p["self_attn.key.weight"].T + p["self_attn.key.bias"]
    v = x @ p["self_attn.value.weight"].T + p["self_attn.value.bias"]
    Er = p["self_attn.Er"]                                                       # [nh][hd][5]
    out = np.zeros_like(x)
    t = np.arange(T)
    for h in range(nh):
        kh = 6 if h == 7 else h
        qh = q[..., h * hd:(h + 1) * hd]
        logits, vals, valid = [], [], []
        for j, o in enumerate(OFFSETS[h]):
            tt = t + o * s
            ok = (tt >= 0) & (tt < T)
            ttc = np.clip(tt, 0, T - 1)
            kj = k[:, ttc, kh * hd:(kh + 1) * hd]
            logits.append(((qh * kj).sum(-1) + qh @ Er[h][:, j]) / math.sqrt(hd))
            vals.append(v[:, ttc, h * hd:(h + 1) * hd])
            valid.append(np.broadcast_to(ok, (I, T)))
        lg = np.stack(logits, -1)
        ok = np.stack(valid, -1)
        lg = np.where(ok, lg, -np.inf)
        e = np.exp(lg - lg.max(-1, keepdims=True))
        pr = e / e.sum(-1, keepdims=True)
        out[..., h * hd:(h + 1) * hd] = np.einsum("itj,itjd->itd", pr, np.stack(vals, 2))
    return out


def instr_layer(p, x):
    """torch TransformerEncoderLayer(norm_first, ReLU) over the instr axis of x [instr][T][D]"""
    I, T, D = x.shape
    nh, hd = 8, D // 8
    y = _ln(x, p["norm1.weight"], p["norm1.bias"])
    qkv = y @ p["self_attn.in_proj_weight"].T + p["self_attn.in_proj_bias"]
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    a = np.zeros_like(x)
    for h in range(nh):
        sl = slice(h * hd, (h + 1) * hd)
        lg = np.einsum("itd,jtd->tij", q[..., sl], k[..., sl]) / math.sqrt(hd)
        e = np.exp(lg - lg.max(-1, keepdims=True))
        pr = e / e.sum(-1, keepdims=True)
        a[..., sl] = np.einsum("tij,jtd->itd", pr, v[..., sl])
    x = x + a @ p["self_attn.out_proj.weight"].T + p["self_attn.out_proj.bias"]
    y = _ln(x, p["norm2.weight"], p["norm2.bias"])
    return x + np.maximum(y @ p["linear1.weight"].T + p["linear1.bias"], 0) @ p["linear2.weight"].T + p["linear2.bias"]


def forward(sd, feat, nlayers: int = 9):
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x = front_end(sd, feat)
    res = {"front": x.copy()}
    tacc = 0.0
    for l in range(nlayers):
        p = {k[len(f"Transformer_layers.time_attention_{l}."):]: v for k, v in sd.items() if k.startswith(f"Transformer_layers.time_attention_{l}.")}
        skip = dilated_attention(p, _ln(x, p["norm1.weight"], p["norm1.bias"]), l)
        x = x + skip
        y = _ln(x, p["norm2.weight"], p["norm2.bias"])
        x = x + _gelu(y @ p["linear1.weight"].T + p["linear1.bias"]) @ p["linear2.weight"].T + p["linear2.bias"]
        tacc = tacc + skip.mean(0)
        if l == 0:
            res["layer0"] = x.copy()
        if 3 <= l <= 5:
            pi = {k[len(f"Transformer_layers.instr_attention_{l}."):]: v for k, v in sd.items() if k.startswith(f"Transformer_layers.instr_attention_{l}.")}
            x = instr_layer(pi, x)
    h = np.maximum(x, 0).mean(0)
    res["logits"] = h @ sd["out_linear.weight"].T + sd["out_linear.bias"]
    res["tempo"] = np.maximum(tacc, 0).mean(0) @ sd["out_linear_t.weight"].T + sd["out_linear_t.bias"]
    return res
