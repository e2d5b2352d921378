"""One numpy function per launch of the Beat-Transformer engine (csrc/beat.hip: run_chunk), for ONE song, in the device's layout: rows are (instr, t), r = i T + t;
frames are t.  tests/beat_np.py's forward is their composition; tests/test_gpu_beat_stages.py feeds each of them the device's own tap of the stage before.

Every function takes ``dtype``: np.float64 is the reference, np.float32 the same formula evaluated in fp32 numpy (the yardstick E32 of the attention stages, as
tests/dtw_np.py's cost_matrix(dtype=np.float32) is for the DTW cost test).  LayerNorm's float32 form is torch's fp32 F.layer_norm, the yardstick of
tests/test_gpu_gemm3_epilogues.py::test_ln_rows_f32.  ``mutant`` arguments are the deliberately wrong variants tests/test_beat_stage_ref_cpu.py uses to show that the
bounds of the GPU test would catch them.

The k_gemm3 stages are described by ``gemm_wb`` (the [N][K] weight and bias the engine packs) and ``EPILOGUE``; ``gemm_stage`` evaluates one, ``gemm_mag`` gives
sum |x w| + |b| (+ |resid|), the per-cell magnitude of tests/test_gpu_gemm3.py's 1e-6 rule.
"""
from __future__ import annotations

import math

import numpy as np

OFFSETS = [[-2, -1, 0, 1, 2]] * 4 + [[-4, -3, -2, -1, 0], [-3, -2, -1, 0, 1], [-1, 0, 1, 2, 3], [0, 1, 2, 3, 4]]
SEG = 128                     # BEAT_SEG: frames per tempo partial sum
C2_COLS = 31                  # conv2 columns whose 12-wide patch lies inside the row (the GEMM runs over all 42; k_beat_patch3 reads 0 .. 23)
EPILOGUE = dict(c2="bias", c3="bias", qkv="bias", hid="gelu", x_ffn="resid", iqkv="bias", ix_attn="resid", ihid="relu", ix_ffn="resid")
TIME_STAGES = ("ln1", "qkv", "skip", "x_attn", "tacc", "ln2", "hid", "x_ffn")
INSTR_STAGES = ("iln1", "iqkv", "iao", "ix_attn", "iln2", "ihid", "ix_ffn")


def _erf(x):
    try:
        from scipy.special import erf
        return erf(x)
    except ImportError:
        import torch
        return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def time_params(sd, l):
    pre = f"Transformer_layers.time_attention_{l}."
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def instr_params(sd, l):
    pre = f"Transformer_layers.instr_attention_{l}."
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def has_instr_layer(l, nlayers):
    return 3 <= l <= 5 and l < nlayers


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln(x, g, b, dtype=np.float64, eps=1e-5):
    if dtype == np.float32:
        import torch
        t = torch.nn.functional.layer_norm(torch.from_numpy(np.ascontiguousarray(x, np.float32)), (x.shape[-1],), torch.from_numpy(np.ascontiguousarray(g, np.float32)),
                                           torch.from_numpy(np.ascontiguousarray(b, np.float32)), eps)
        return t.numpy()
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


# ------------------------------------------------------------------------------------------------ k_gemm3 stages
def gemm_wb(sd, stage, l=None):
    """the [N][K] weight and [N] bias of a k_gemm3 stage as etd_beat_create lays them out (float64)"""
    f = lambda a: np.asarray(a, np.float64)
    if stage == "c2":           # [co][ci][0][kw] -> [co][kw 32 + ci]
        return f(sd["conv2.weight"])[:, :, 0, :].transpose(0, 2, 1).reshape(64, 384), f(sd["conv2.bias"])
    if stage == "c3":           # [co][ci][kt][kw] -> [co][kt 384 + kw 64 + ci]
        w = f(sd["conv3.weight"])
        return w.transpose(0, 2, 3, 1).reshape(w.shape[0], 1152), f(sd["conv3.bias"])
    if stage == "qkv":
        p = time_params(sd, l)
        return (np.concatenate([f(p[f"self_attn.{n}.weight"]) for n in ("query", "key", "value")]),
                np.concatenate([f(p[f"self_attn.{n}.bias"]) for n in ("query", "key", "value")]))
    p = instr_params(sd, l) if stage.startswith("i") else time_params(sd, l)
    name = {"hid": "linear1", "x_ffn": "linear2", "ihid": "linear1", "ix_ffn": "linear2", "ix_attn": "self_attn.out_proj"}.get(stage)
    if stage == "iqkv":
        return f(p["self_attn.in_proj_weight"]), f(p["self_attn.in_proj_bias"])
    return f(p[name + ".weight"]), f(p[name + ".bias"])


def gemm_stage(sd, stage, l, x, resid=None, dtype=np.float64):
    """epilogue(x W^T + b) of a k_gemm3 stage; RESID: (x W^T + b) + resid"""
    W, b = gemm_wb(sd, stage, l)
    u = np.asarray(x, dtype) @ W.astype(dtype).T + b.astype(dtype)
    epi = EPILOGUE[stage]
    if epi == "gelu":
        return (0.5 * u * (1.0 + _erf(u / dtype(math.sqrt(2.0))))).astype(dtype)
    if epi == "relu":
        return np.maximum(u, 0)
    if epi == "resid":
        return u + np.asarray(resid, dtype)
    return u


def gemm_mag(sd, stage, l, x, resid=None):
    """sum_k |x_k w_k| + |b| (+ |resid|) per output cell, float64: what tests/test_gpu_gemm3_epilogues.py calls `full`"""
    W, b = gemm_wb(sd, stage, l)
    m = np.abs(np.asarray(x, np.float64)) @ np.abs(W).T + np.abs(b)
    return m + np.abs(np.asarray(resid, np.float64)) if resid is not None else m


# ------------------------------------------------------------------------------------------------ conv front end
def _shift_rows(a, d, I, T, pad):
    """rows r = i T + t of a [I T][...] array moved so that out[r] = a[row of (i, t + d)]; outside the stem: 0, or (mutant 'neighbour') whatever row r + d of the
    buffer holds -- the next / previous stem's, cyclically"""
    out = np.roll(a, -d, axis=0)
    if pad == "zero":
        t = np.arange(I * T) % T + d
        out[(t < 0) | (t >= T)] = 0
    return out


def conv1(sd, feat, dtype=np.float64, pad="zero", mag=False):
    """k_beat_conv1: feat [I][T][128] -> c1 [I T][42][32] = relu(max_{u<3} conv(x)[t][3 p + u]); time padding (2, 0).  mag: also max_u (|b| + sum |w x|)"""
    I, T, _ = feat.shape
    x = np.asarray(feat, dtype).reshape(I * T, 128)
    w, b = np.asarray(sd["conv1.weight"], dtype)[:, 0], np.asarray(sd["conv1.bias"], dtype)        # [32][5][3]
    acc = np.zeros((I * T, 126, 32), dtype) + b
    m = np.zeros((I * T, 126, 32), np.float64) + np.abs(np.asarray(b, np.float64)) if mag else None
    for kt in range(5):
        xs = _shift_rows(x, kt - 2, I, T, pad)
        for kw in range(3):
            acc = acc + xs[:, kw:kw + 126, None] * w[None, None, :, kt, kw]
            if mag:
                m += np.abs(xs[:, kw:kw + 126, None].astype(np.float64) * w[None, None, :, kt, kw].astype(np.float64))
    out = np.maximum(acc.reshape(I * T, 42, 3, 32).max(2), 0)
    return (out, m.reshape(I * T, 42, 3, 32).max(2)) if mag else out


def conv2_patches(c1):
    """c1 [R][42][32] -> the 384-float GEMM rows of columns 0 .. 30: [R 31][384] (row (r, col) = the floats from (r 42 + col) 32 on)"""
    R = c1.shape[0]
    flat = np.ascontiguousarray(c1).reshape(R, 42 * 32)
    return np.stack([flat[:, c * 32:c * 32 + 384] for c in range(C2_COLS)], 1).reshape(R * C2_COLS, 384)


def conv2(sd, c1, dtype=np.float64):
    """conv2 + bias on columns 0 .. 30 of every row: [R][31][64] (the device's buffer is [R][42][64]; its columns 31 .. 41 read past the row and nothing reads them)"""
    return gemm_stage(sd, "c2", None, conv2_patches(c1), dtype=dtype).reshape(c1.shape[0], C2_COLS, 64)


def patch3(c2, I, T, pad="zero"):
    """k_beat_patch3 (a pure selection): c2 [R][>= 24][64] -> x3 [R 3][1152], x3[r 3 + c][kt 384 + kw 64 + ci] = relu(max_{u<3} c2[r + kt - 1][3 (c + kw) + u][ci]),
    0 where t + kt - 1 is outside the song (conv3's time padding 1)"""
    R = I * T
    pooled = np.maximum(np.asarray(c2)[:, :24].reshape(R, 8, 3, 64).max(2), 0)                    # [R][8][64]
    out = np.zeros((R, 3, 3, 6, 64), pooled.dtype)
    for kt in range(3):
        ps = _shift_rows(pooled, kt - 1, I, T, pad)
        for c in range(3):
            out[:, c, kt] = ps[:, c:c + 6]
    return out.reshape(R * 3, 1152)


def conv3(sd, x3, dtype=np.float64):
    return gemm_stage(sd, "c3", None, x3, dtype=dtype)


def pool3(c3):
    """k_beat_pool3 (a pure selection): c3 [R 3][256] -> tokens [R][256]"""
    return np.maximum(np.asarray(c3).reshape(-1, 3, c3.shape[-1]).max(1), 0)


# ------------------------------------------------------------------------------------------------ attention kernels
def dattn(p, qkv, I, T, layer, dtype=np.float64, mutant=None):
    """k_beat_dattn: qkv [I T][768] (q | k | v) -> skip [I T][256]; x_attn = x + skip is the caller's.  mutant: 'er0' (Er zeroed), 'h7own' (head 7 reads its own
    keys), 'rot' (the offset rows of heads 4 .. 7 rotated by one), 'mask0' (a tap outside the song takes logit 0 and value 0 and stays in the softmax)"""
    D = qkv.shape[1] // 3
    nh, hd, s = 8, D // 8, 2 ** layer
    a = np.asarray(qkv, dtype).reshape(I, T, 3 * D)
    q, k, v = a[..., :D], a[..., D:2 * D], a[..., 2 * D:]
    Er = np.asarray(p["self_attn.Er"], dtype)                                      # [nh][hd][5]
    if mutant == "er0":
        Er = np.zeros_like(Er)
    offs = list(OFFSETS)
    if mutant == "rot":
        offs = OFFSETS[:4] + [OFFSETS[5], OFFSETS[6], OFFSETS[7], OFFSETS[4]]
    out = np.zeros((I, T, D), dtype)
    t = np.arange(T)
    scale = dtype(math.sqrt(hd))
    for h in range(nh):
        kh = 6 if (h == 7 and mutant != "h7own") else h
        qh = q[..., h * hd:(h + 1) * hd]
        logits, vals, valid = [], [], []
        for j, o in enumerate(offs[h]):
            tt = t + o * s
            ok = (tt >= 0) & (tt < T)
            ttc = np.clip(tt, 0, T - 1)
            kj = k[:, ttc, kh * hd:(kh + 1) * hd]
            vj = v[:, ttc, h * hd:(h + 1) * hd]
            if mutant == "mask0":
                kj, vj = kj * ok[None, :, None], vj * ok[None, :, None]
            logits.append(((qh * kj).sum(-1) + qh @ Er[h][:, j]) / scale)
            vals.append(vj)
            valid.append(np.broadcast_to(ok, (I, T)))
        lg, ok = np.stack(logits, -1), np.stack(valid, -1)
        if mutant == "mask0":
            lg = np.where(ok, lg, dtype(0))
        else:
            lg = np.where(ok, lg, dtype(-np.inf))
        e = np.exp(lg - lg.max(-1, keepdims=True))
        pr = e / e.sum(-1, keepdims=True)
        out[..., h * hd:(h + 1) * hd] = np.einsum("itj,itjd->itd", pr, np.stack(vals, 2))
    return out.reshape(I * T, D)


def iattn(iqkv, I, T, dtype=np.float64):
    """k_beat_iattn: in_proj output [I T][768] -> 8-head attention over the I rows of each frame [I T][256]"""
    D = iqkv.shape[1] // 3
    nh, hd = 8, D // 8
    a = np.asarray(iqkv, dtype).reshape(I, T, 3 * D)
    q, k, v = a[..., :D], a[..., D:2 * D], a[..., 2 * D:]
    out = np.zeros((I, T, D), dtype)
    for h in range(nh):
        sl = slice(h * hd, (h + 1) * hd)
        lg = np.einsum("itd,jtd->tij", q[..., sl], k[..., sl]) / dtype(math.sqrt(hd))
        e = np.exp(lg - lg.max(-1, keepdims=True))
        pr = e / e.sum(-1, keepdims=True)
        out[..., sl] = np.einsum("tij,jtd->itd", pr, v[..., sl])
    return out.reshape(I * T, D)


# ------------------------------------------------------------------------------------------------ fixed-order fp32 sums
def skipacc(skip, tacc_prev, I, T, dtype=np.float64, mutant=None, mag=False):
    """k_beat_skipacc: tacc[t] = (tacc_prev[t] +) (sum_i skip[i T + t]) / I  (tacc_prev None: the first layer).  mutant 'instr-1': the mean over I - 1 stems.
    mag: also sum |terms| = sum_i |skip| / I + |tacc_prev|"""
    s = np.asarray(skip, dtype).reshape(I, T, -1)
    n = I - 1 if mutant == "instr-1" else I
    m = s[:n].sum(0) / dtype(n)
    out = m if tacc_prev is None else np.asarray(tacc_prev, dtype) + m
    if mag:
        g = np.abs(np.asarray(skip, np.float64)).reshape(I, T, -1).sum(0) / I
        return out, g if tacc_prev is None else g + np.abs(np.asarray(tacc_prev, np.float64))
    return out


def head(sd, x, I, T, dtype=np.float64, mag=False):
    """k_beat_head: logits[t][k] = b[k] + W[k] . mean_i relu(x[i T + t]).  mag: also |b| + |W| . mean_i relu(x)"""
    W, b = np.asarray(sd["out_linear.weight"], dtype), np.asarray(sd["out_linear.bias"], dtype)
    h = np.maximum(np.asarray(x, dtype), 0).reshape(I, T, -1).sum(0) / dtype(I)
    out = h @ W.T + b
    if mag:
        return out, np.abs(h.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))
    return out


def tempo_part(tacc, T, dtype=np.float64, seg=SEG):
    """k_beat_tempo_part: part[g] = sum over frames [g seg, g seg + seg) of relu(tacc[t]) -> [ceil(T / seg)][256] (relu >= 0: the sum is its own sum |terms|).
    seg = 127 is the mutant"""
    r = np.maximum(np.asarray(tacc, dtype), 0)
    return np.stack([r[g:g + seg].sum(0) for g in range(0, T, seg)])


def tempo(sd, part, T, dtype=np.float64, mag=False):
    """k_beat_tempo: out[j] = bt[j] + Wt[j] . ((sum_g part[g]) / T).  mag: also |bt| + |Wt| . m"""
    W, b = np.asarray(sd["out_linear_t.weight"], dtype), np.asarray(sd["out_linear_t.bias"], dtype)
    m = np.asarray(part, dtype).sum(0) / dtype(T)
    out = m @ W.T + b
    if mag:
        return out, np.abs(m.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))
    return out


# ------------------------------------------------------------------------------------------------ the chain
def chain(sd, feat, nlayers=9, dtype=np.float64):
    """every stage of one song from its features, each from the stage before: dict with c1, c2 ([R][31][64]), x3, c3, front, per time layer l `ln1.l` .. `x_ffn.l`
    (TIME_STAGES), per instrument layer `iln1.l` .. `ix_ffn.l` (INSTR_STAGES), part, logits, tempo"""
    I, T, _ = feat.shape
    r = {}
    r["c1"] = conv1(sd, feat, dtype)
    r["c2"] = conv2(sd, r["c1"], dtype)
    r["x3"] = patch3(r["c2"], I, T)
    r["c3"] = conv3(sd, r["x3"], dtype)
    x = r["front"] = pool3(r["c3"])
    tacc = None
    for l in range(nlayers):
        p = time_params(sd, l)
        r[f"ln1.{l}"] = ln(x, p["norm1.weight"], p["norm1.bias"], dtype)
        r[f"qkv.{l}"] = gemm_stage(sd, "qkv", l, r[f"ln1.{l}"], dtype=dtype)
        r[f"skip.{l}"] = dattn(p, r[f"qkv.{l}"], I, T, l, dtype)
        x = r[f"x_attn.{l}"] = x + r[f"skip.{l}"]
        tacc = r[f"tacc.{l}"] = skipacc(r[f"skip.{l}"], tacc, I, T, dtype)
        r[f"ln2.{l}"] = ln(x, p["norm2.weight"], p["norm2.bias"], dtype)
        r[f"hid.{l}"] = gemm_stage(sd, "hid", l, r[f"ln2.{l}"], dtype=dtype)
        x = r[f"x_ffn.{l}"] = gemm_stage(sd, "x_ffn", l, r[f"hid.{l}"], resid=x, dtype=dtype)
        if has_instr_layer(l, nlayers):
            q = instr_params(sd, l)
            r[f"iln1.{l}"] = ln(x, q["norm1.weight"], q["norm1.bias"], dtype)
            r[f"iqkv.{l}"] = gemm_stage(sd, "iqkv", l, r[f"iln1.{l}"], dtype=dtype)
            r[f"iao.{l}"] = iattn(r[f"iqkv.{l}"], I, T, dtype)
            x = r[f"ix_attn.{l}"] = gemm_stage(sd, "ix_attn", l, r[f"iao.{l}"], resid=x, dtype=dtype)
            r[f"iln2.{l}"] = ln(x, q["norm2.weight"], q["norm2.bias"], dtype)
            r[f"ihid.{l}"] = gemm_stage(sd, "ihid", l, r[f"iln2.{l}"], dtype=dtype)
            x = r[f"ix_ffn.{l}"] = gemm_stage(sd, "ix_ffn", l, r[f"ihid.{l}"], resid=x, dtype=dtype)
    r["logits"] = head(sd, x, I, T, dtype)
    r["part"] = tempo_part(tacc, T, dtype)
    r["tempo"] = tempo(sd, r["part"], T, dtype)
    return r


def chain_call(sd, feats, nlayers, dtype):
    """``chain`` over the songs of a call, concatenated in the call's global row / frame / segment order (tempo: [songs][300]); plus `feat`"""
    per = [chain(sd, f, nlayers, dtype) for f in feats]
    out = {k: (np.stack([p[k] for p in per]) if k == "tempo" else np.concatenate([p[k] for p in per])) for k in per[0]}
    out["feat"] = feats
    return out


def song_slices(Ts, I):
    """(row slice, frame slice, T) of every song of a call in its global row / frame order"""
    r0 = f0 = 0
    for T in Ts:
        yield slice(r0, r0 + I * T), slice(f0, f0 + T), T
        r0, f0 = r0 + I * T, f0 + T
