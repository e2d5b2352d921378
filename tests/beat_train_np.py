"""Torch restatement of what etude_amd.BeatTrainer computes (csrc/beat_train.hip), written against tests/beat_stage_ref.py's stage formulas: the
Beat-Transformer forward in eval arithmetic (no dropout), this project's beat / tempo loss, autograd for the gradients, and the clipped AdamW trajectory of
tests/train_np.py.  Runs in fp64 (the reference of the GPU tests) or fp32 (their yardstick) on the CPU.

    loss = sum_c (1 / n_c) sum_{scored (f, c)} (1 + (pos_weight_c - 1) y) bce_with_logits(z, y)  +  tempo_weight * mean_{songs with a target} -sum_k p_k log_softmax(t)_k

A batch is a dict: ``feats`` (list of [I][T][128]), ``beat`` (list of [T][ntoken], -1 = not scored), ``tempo`` (list of [300] or None; or None).
``mutant`` names one of the deliberately wrong variants tests/test_beat_train_cpu.py uses to show that the GPU test's bound would catch them:
'der0' (Er gets no gradient), 'h7own' (head 7 reads its own keys), 'skip_instr-1' (the skip mean's gradient divided by instr - 1), 'fold_kw' (conv2's input gradient
misses kw = 5), 'tempo_T-1' (the tempo mean over T - 1 frames).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from beat_stage_ref import OFFSETS, has_instr_layer
from train_np import clip_and_adamw

EPS32 = 2.0 ** -24


def to_torch(state: Dict[str, np.ndarray], dtype=torch.float64, requires_grad: bool = True) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad)) for k, v in state.items())


def _grad_scale(x: torch.Tensor, s: float) -> torch.Tensor:
    """x in the forward pass, s times its gradient in the backward pass"""
    return x.detach() + (x - x.detach()) * s


def _pool3(x: torch.Tensor, diag: Optional[dict], name: str) -> torch.Tensor:
    """max over groups of 3 along the last axis (floor), then ReLU: F.max_pool2d routes the gradient to the first maximal column, relu has gradient 0 at 0"""
    n = x.shape[-1] // 3
    if diag is not None:
        top = x[..., :3 * n].reshape(*x.shape[:-1], n, 3).detach().sort(-1).values
        diag.setdefault("pool_gap", []).append(float((top[..., 2] - top[..., 1]).min()))
        diag.setdefault("relu_gap", []).append(float(top[..., 2].abs().min()))
        diag.setdefault("pool_in", []).append(x[..., :3 * n].reshape(*x.shape[:-1], n, 3).detach().clone())
    return torch.relu(F.max_pool2d(x, (1, 3), (1, 3)))


def front_end(p: Dict[str, torch.Tensor], feat: torch.Tensor, mutant: Optional[str] = None, diag: Optional[dict] = None, used_only: bool = False) -> torch.Tensor:
    """[I][T][128] -> tokens [I][T][256]"""
    I, T, _ = feat.shape
    x = F.conv2d(feat[:, None], p["conv1.weight"], p["conv1.bias"], padding=(2, 0))                      # [I][32][T][126]
    c1 = _pool3(x, diag, "pool1")                                                                          # [I][32][T][42]
    w2 = p["conv2.weight"]
    c2 = p["conv2.bias"][None, :, None, None]
    for kw in range(12):                                                                                   # conv2 (1, 12) as its 12 taps
        tap = c1[..., kw:kw + 31]
        if mutant == "fold_kw" and kw == 5:
            tap = tap.detach()
        c2 = c2 + torch.einsum("ictw,oc->iotw", tap, w2[:, :, 0, kw])
    if used_only:
        c2 = c2[..., :24]                                                                                  # (the columns the model reads; diag only)
    c2p = _pool3(c2, diag, "pool2")                                                                        # [I][64][T][10 or 8]
    x = F.conv2d(c2p, p["conv3.weight"], p["conv3.bias"], padding=(1, 0))                                  # [I][256][T][5 or 3]
    x = _pool3(x[..., :3], diag, "pool3")                                                                  # [I][256][T][1]
    return x[..., 0].transpose(1, 2)


def dattn_from_qkv(qkv: torch.Tensor, Er: torch.Tensor, layer: int, mutant: Optional[str] = None, diag: Optional[dict] = None) -> torch.Tensor:
    """k_bt_dattn: qkv [I][T][768] (q | k | v), Er [8][32][5] -> skip [I][T][256]; taps outside the song are masked by index"""
    I, T, D3 = qkv.shape
    D = D3 // 3
    hd, s = D // 8, 2 ** layer
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    if mutant == "der0":
        Er = Er.detach()
    t = torch.arange(T)
    outs = []
    for h in range(8):
        kh = 6 if (h == 7 and mutant != "h7own") else h
        qh = q[..., h * hd:(h + 1) * hd]
        lg, vals, oks = [], [], []
        for j, o in enumerate(OFFSETS[h]):
            tt = t + o * s
            ok = (tt >= 0) & (tt < T)
            ttc = tt.clamp(0, T - 1)
            kj, vj = k[:, ttc, kh * hd:(kh + 1) * hd], v[:, ttc, h * hd:(h + 1) * hd]
            qk = (qh * kj).sum(-1)
            if diag is not None and bool(ok.any()):
                diag.setdefault("qk_min", []).append(float(qk.detach()[:, ok].abs().min()))
            lg.append((qk + qh @ Er[h][:, j]) / math.sqrt(hd))
            vals.append(vj)
            oks.append(ok)
        lg, ok = torch.stack(lg, -1), torch.stack(oks, -1)[None].expand(I, T, 5)
        pr = torch.softmax(lg.masked_fill(~ok, float("-inf")), -1)
        outs.append((pr[..., None] * torch.stack(vals, 2)).sum(2))
    return torch.cat(outs, -1)


def dilated_attention(p: Dict[str, torch.Tensor], pre: str, x: torch.Tensor, layer: int, mutant: Optional[str] = None, diag: Optional[dict] = None) -> torch.Tensor:
    """x [I][T][256] (already normalised) -> skip [I][T][256]"""
    qkv = torch.cat([F.linear(x, p[pre + f"self_attn.{n}.weight"], p[pre + f"self_attn.{n}.bias"]) for n in ("query", "key", "value")], -1)
    return dattn_from_qkv(qkv, p[pre + "self_attn.Er"], layer, mutant, diag)


def iattn_from_qkv(a: torch.Tensor) -> torch.Tensor:
    """k_bt_iattn: in_proj output [I][T][768] -> 8-head attention over the I rows of every frame [I][T][256]"""
    I, T, D3 = a.shape
    D = D3 // 3
    hd = D // 8
    q, k, v = (a[..., i * D:(i + 1) * D].reshape(I, T, 8, hd) for i in range(3))
    lg = torch.einsum("ithd,jthd->thij", q, k) / math.sqrt(hd)
    return torch.einsum("thij,jthd->ithd", torch.softmax(lg, -1), v).reshape(I, T, D)


def instrument_attention(p: Dict[str, torch.Tensor], pre: str, x: torch.Tensor) -> torch.Tensor:
    """x [I][T][256] (normalised) -> the out_proj input [I][T][256]"""
    return iattn_from_qkv(F.linear(x, p[pre + "self_attn.in_proj_weight"], p[pre + "self_attn.in_proj_bias"]))


def forward(p: Dict[str, torch.Tensor], feat: torch.Tensor, nlayers: int, mutant: Optional[str] = None, diag: Optional[dict] = None):
    """one song's features [I][T][128] -> (logits [T][ntoken], tempo [300])"""
    I, T, _ = feat.shape
    x = front_end(p, feat, mutant, diag)
    ln = lambda x, pre, n: F.layer_norm(x, (256,), p[pre + n + ".weight"], p[pre + n + ".bias"], 1e-5)      # noqa: E731
    tacc = None
    for l in range(nlayers):
        pre = f"Transformer_layers.time_attention_{l}."
        skip = dilated_attention(p, pre, ln(x, pre, "norm1"), l, mutant, diag)
        x = x + skip
        m = skip.sum(0) / I
        if mutant == "skip_instr-1":
            m = _grad_scale(m, I / (I - 1.0))
        tacc = m if tacc is None else tacc + m
        x = x + F.linear(F.gelu(F.linear(ln(x, pre, "norm2"), p[pre + "linear1.weight"], p[pre + "linear1.bias"])), p[pre + "linear2.weight"], p[pre + "linear2.bias"])
        if has_instr_layer(l, nlayers):
            pre = f"Transformer_layers.instr_attention_{l}."
            ao = instrument_attention(p, pre, ln(x, pre, "norm1"))
            x = x + F.linear(ao, p[pre + "self_attn.out_proj.weight"], p[pre + "self_attn.out_proj.bias"])
            x = x + F.linear(torch.relu(F.linear(ln(x, pre, "norm2"), p[pre + "linear1.weight"], p[pre + "linear1.bias"])), p[pre + "linear2.weight"], p[pre + "linear2.bias"])
    logits = F.linear(torch.relu(x).sum(0) / I, p["out_linear.weight"], p["out_linear.bias"])
    tm = torch.relu(tacc).sum(0) / (T - 1 if mutant == "tempo_T-1" else T)
    return logits, F.linear(tm, p["out_linear_t.weight"], p["out_linear_t.bias"])


def loss_of(p: Dict[str, torch.Tensor], nlayers: int, batch: dict, pos_weight=None, tempo_weight: float = 1.0, mutant: Optional[str] = None, diag: Optional[dict] = None):
    """(loss, scored beat cells, skipped): the loss of the module docstring over the batch; nan and skipped when nothing is scored"""
    dt = next(iter(p.values())).dtype
    outs = [forward(p, torch.as_tensor(np.asarray(f), dtype=dt), nlayers, mutant, diag) for f in batch["feats"]]
    z = torch.cat([o[0] for o in outs])
    y = torch.cat([torch.as_tensor(np.asarray(b), dtype=dt) for b in batch["beat"]])
    nt = z.shape[1]
    pw = torch.ones(nt, dtype=dt) if pos_weight is None else torch.as_tensor(np.asarray(pos_weight), dtype=dt)
    scored = y >= 0
    ys = torch.where(scored, y, torch.zeros_like(y))
    cell = (1 + (pw - 1) * ys) * F.binary_cross_entropy_with_logits(z, ys, reduction="none")
    n_c = scored.sum(0)
    loss = z.sum() * 0
    for c in range(nt):
        if int(n_c[c]):
            loss = loss + cell[:, c][scored[:, c]].sum() / int(n_c[c])
    tempo = batch.get("tempo") or [None] * len(outs)
    rows = [-(torch.as_tensor(np.asarray(t), dtype=dt) * torch.log_softmax(o[1], -1)).sum() for o, t in zip(outs, tempo) if t is not None]
    if rows:
        loss = loss + tempo_weight * torch.stack(rows).sum() / len(rows)
    skipped = int(n_c.sum()) == 0 and not rows
    return (loss * float("nan") if skipped else loss), int(n_c.sum()), skipped


def loss_and_grads(state: Dict[str, np.ndarray], nlayers: int, batch: dict, dtype=torch.float64, loss_scale: float = 1.0, pos_weight=None, tempo_weight: float = 1.0,
                   mutant: Optional[str] = None):
    """(loss_scale * loss, {key: loss_scale * d loss / d key}) as numpy arrays of ``dtype``; a parameter the loss does not reach gets zeros"""
    p = to_torch(state, dtype)
    loss, _, skipped = loss_of(p, nlayers, batch, pos_weight, tempo_weight, mutant)
    if skipped:
        return float("nan"), OrderedDict((k, np.zeros_like(v.detach().numpy())) for k, v in p.items())
    (loss * loss_scale).backward()
    return float(loss.detach()) * loss_scale, OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()) for k, v in p.items())


def diagnostics(state: Dict[str, np.ndarray], nlayers: int, feats: Sequence) -> dict:
    """the smallest margins of the choices a gradient depends on: max-pool top-2 gaps, pooled maxima against the ReLU's 0, |q . k| of in-range taps"""
    p = to_torch(state, torch.float64, requires_grad=False)
    diag: dict = {}
    with torch.no_grad():
        for f in feats:
            forward(p, torch.as_tensor(np.asarray(f), dtype=torch.float64), nlayers, None, diag)
    return {k: min(v) for k, v in diag.items() if k != "pool_in"}


def pool_margins(state: Dict[str, np.ndarray], feat) -> List[dict]:
    """For each of the three max-pools of the front end, over the cells the model reads: the smallest top-2 gap and the smallest |maximum| (the ReLU's kink) of
    the fp64 restatement, and the largest |fp32 - fp64| of the pool's input in fp32 torch.  A choice whose margin is below that error is not decidable in fp32."""
    vals = {}
    for dt in (torch.float64, torch.float32):
        diag: dict = {}
        p = to_torch(state, dt, requires_grad=False)
        with torch.no_grad():
            front_end(p, torch.as_tensor(np.asarray(feat), dtype=dt), None, diag, used_only=True)
        vals[dt] = diag["pool_in"]
    out = []
    for a, c in zip(vals[torch.float64], vals[torch.float32]):
        top = a.sort(-1).values
        out.append(dict(gap=float((top[..., 2] - top[..., 1]).min()), kink=float(top[..., 2].abs().min()), err32=float((a - c.double()).abs().max())))
    return out


def trajectory(state: Dict[str, np.ndarray], nlayers: int, batches: Sequence[dict], n_steps: int, dtype=torch.float64, max_norm: float = 0.5, lr: float = 1e-3,
               betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, pos_weight=None, tempo_weight: float = 1.0):
    """``n_steps`` optimizer steps, each over ``batches`` (accumulated with loss_scale 1 / len(batches)) through train_np.clip_and_adamw;
    returns (the unscaled losses of every batch of every step, the final parameters)"""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    params = OrderedDict((k, np.array(v, npdt)) for k, v in state.items())
    m = OrderedDict((k, np.zeros_like(v)) for k, v in params.items())
    v = OrderedDict((k, np.zeros_like(w)) for k, w in params.items())
    out: List[List[float]] = []
    nb = len(batches)
    for s in range(n_steps):
        acc = OrderedDict((k, np.zeros_like(w)) for k, w in params.items())
        losses = []
        for b in batches:
            loss, g = loss_and_grads(params, nlayers, b, dtype, 1.0 / nb, pos_weight, tempo_weight)
            losses.append(loss * nb)
            for k in acc:
                acc[k] += g[k].astype(npdt)
        clip_and_adamw(params, acc, m, v, s + 1, max_norm, lr, betas, eps, weight_decay)
        out.append(losses)
    return out, params


def rel_err(g: np.ndarray, g64: np.ndarray) -> float:
    """max |g - g64| / max |g64| (0 / 0 = 0; anything else over 0 = inf)"""
    den = float(np.abs(g64).max()) if g64.size else 0.0
    num = float(np.abs(np.asarray(g, np.float64) - g64).max()) if g64.size else 0.0
    return 0.0 if num == 0.0 else (math.inf if den == 0.0 else num / den)


def make_batch(seed: int, Ts: Sequence[int], instr: int = 5, ntoken: int = 2, no_tempo=(), unscored=(), p_unscored: float = 0.1, period: int = 0) -> dict:
    """a synthetic ragged batch: synth.beat_features per song, sparse beat targets with about 10 % unscored cells, a smooth tempo distribution; ``no_tempo`` /
    ``unscored``: indices of songs without a tempo target / with every beat cell unscored; ``period`` > 0: features periodic in time"""
    from etude_amd import synth
    rng = np.random.default_rng(seed)
    feats, beat, tempo = [], [], []
    for s, T in enumerate(Ts):
        if period:      # the first `period` frames repeated: the front end then has few distinct cells (see tests/test_gpu_beat_train.py, l9_T1030)
            one = synth.beat_features(seed * 1000 + s, period, instr=instr)
            feats.append(np.ascontiguousarray(np.tile(one, (1, (T + period - 1) // period, 1))[:, :T]))
        else:
            feats.append(synth.beat_features(seed * 1000 + s, T, instr=instr))
        y = (rng.random((T, ntoken)) < 0.2).astype(np.float32)
        y = np.where(rng.random((T, ntoken)) < 0.3, np.float32(0.5) * y + np.float32(0.25), y).astype(np.float32)      # some soft labels
        y[rng.random((T, ntoken)) < p_unscored] = -1.0
        if s in unscored:
            y[:] = -1.0
        beat.append(y)
        if s in no_tempo:
            tempo.append(None)
        else:
            c = rng.uniform(40, 260)
            d = np.exp(-0.5 * ((np.arange(300) - c) / 6.0) ** 2)
            d = (d / d.sum()).astype(np.float32)
            d[int(c)] += np.float32(1.0 - float(d.astype(np.float64).sum()))      # the fp32 row sums to 1 within rounding
            tempo.append(d)
    return dict(feats=feats, beat=beat, tempo=tempo)
