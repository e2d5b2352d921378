"""Separator training, restated with torch-CPU ops in a dtype of the caller's choice: fp64 autograd is the truth, fp32 autograd the yardstick a device
gradient is measured against.  The shared pieces (ELU, the tap-by-tap convolutions' geometry, LEVELS) are separator_np's; the convolutions here are the same sums
over a batch [B][T][F][C].

``variant`` switches ONE deliberate mistake on, for the tests that show each would be seen: "one_unit" (statistics over unit 0 only), "unbiased" (variance / (n - 1)),
"no_skip_grad" (the skip connection passes no gradient), "no_coupling" (the softmax's denominator passes no gradient), "norm_by_B" (the loss divided by B only)."""
from __future__ import annotations

import numpy as np
import torch

import separator_np as sp

LEVELS = sp.LEVELS
MOMENTUM = 0.99
TRAINABLE = (".weight", ".bias", ".gamma", ".beta")


def params(state, dtype, requires_grad: bool = True):
    """the state as torch tensors of ``dtype``; the trainable ones are leaves that require a gradient"""
    out = {}
    for k, v in state.items():
        t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype).clone()
        if requires_grad and k.endswith(TRAINABLE):
            t.requires_grad_(True)
        out[k] = t
    return out


# ---------------------------------------------------------------------------------------------- the convolutions over a batch
def conv_down(x, w, b):
    """separator_np.conv_down on [B][T][F][Ci]"""
    B, T, F, Ci = x.shape
    xp = torch.zeros((B, T + 3, F + 3, Ci), dtype=x.dtype)
    xp[:, 1:T + 1, 1:F + 1] = x
    out = torch.zeros((B, T // 2, F // 2, w.shape[3]), dtype=x.dtype)
    for kt in range(5):
        for kf in range(5):
            out = out + xp[:, kt:kt + T:2, kf:kf + F:2] @ w[kt, kf]
    return out + b


def conv_up(x, w, b):
    """separator_np.conv_up on [B][T][F][Ci]"""
    B, T, F, Ci = x.shape
    full = torch.zeros((B, 2 * T + 3, 2 * F + 3, w.shape[2]), dtype=x.dtype)
    for kt in range(5):
        for kf in range(5):
            full[:, kt:kt + 2 * T:2, kf:kf + 2 * F:2] += x @ w[kt, kf].T
    return full[:, 1:1 + 2 * T, 1:1 + 2 * F] + b


def head(x, w, b):
    """separator_np.head on [B][T][F][1]"""
    B, T, F, Ci = x.shape
    xp = torch.zeros((B, T + 6, F + 6, Ci), dtype=x.dtype)
    xp[:, 3:T + 3, 3:F + 3] = x
    out = torch.zeros((B, T, F, w.shape[3]), dtype=x.dtype)
    for kt in range(4):
        for kf in range(4):
            out = out + xp[:, 2 * kt:2 * kt + T, 2 * kf:2 * kf + F] @ w[kt, kf]
    return out + b


# ---------------------------------------------------------------------------------------------- the norm in training mode
def batch_stats(x, variant=None):
    """per channel over all units and positions: the mean and the biased variance"""
    xs = x[:1] if variant == "one_unit" else x
    red = tuple(range(x.dim() - 1))
    mean = xs.mean(red)
    var = ((xs - mean) ** 2).mean(red)
    if variant == "unbiased":
        n = xs.numel() // xs.shape[-1]
        var = var * (n / max(n - 1, 1))
    return mean, var


def norm(x, P, key: str, bn_eps: float, frozen: bool, stats, variant=None):
    """gamma (x - mean) / sqrt(var + eps) + beta on the batch's statistics (frozen: the running ones); ``stats[key]`` collects (mean, var) of the batch"""
    if frozen:
        mean, var = P[f"{key}.mean"], P[f"{key}.var"]
    else:
        mean, var = batch_stats(x, variant)
        if stats is not None:
            stats[key] = (mean.detach(), var.detach())
    eps = torch.tensor(np.float32(bn_eps)).to(x.dtype)
    return P[f"{key}.gamma"] * ((x - mean) / torch.sqrt(var + eps)) + P[f"{key}.beta"]


def unet_train(mix, P, name: str, bn_eps: float, frozen: bool = False, stats=None, variant=None, taps=None):
    """mix [B][T][F][C] -> logits [B][T][F][C] of instrument ``name``.  ``taps`` collects every layer's tensors."""
    x, pres = mix, []
    for l in range(1, LEVELS + 1):
        pre = conv_down(x, P[f"{name}.conv{l}.weight"], P[f"{name}.conv{l}.bias"])
        act = sp.elu(norm(pre, P, f"{name}.bn{l}", bn_eps, frozen, stats, variant))      # (conv_6's is read by nothing; its statistics still move)
        if taps is not None:
            taps[f"conv{l}"] = (x, pre, act)
        pres.append(pre)
        x = act
    up = None
    for j in range(1, LEVELS + 1):
        skip = pres[LEVELS - j]
        if variant == "no_skip_grad":
            skip = skip.detach()
        xin = skip if up is None else torch.cat([skip, up], dim=-1)
        v = conv_up(xin, P[f"{name}.deconv{j}.weight"], P[f"{name}.deconv{j}.bias"])
        out = norm(sp.elu(v), P, f"{name}.bn{LEVELS + j}", bn_eps, frozen, stats, variant)
        if taps is not None:
            taps[f"deconv{j}"] = (skip, up, v, out)
        up = out
    logits = head(up, P[f"{name}.head.weight"], P[f"{name}.head.bias"])
    if taps is not None:
        taps["head"] = (up, logits)
    return logits


def forward(mix, P, cfg, frozen: bool = False, stats=None, variant=None):
    """mix [B][T][F][C] -> logits [I][B][T][F][C]"""
    return torch.stack([unet_train(mix, P, name, cfg.bn_eps, frozen, stats, variant) for name in cfg.instruments])


def loss_fn(logits, mix, target, variant=None):
    """logits, target [I][B][T][F][C], mix [B][T][F][C] -> (1 / (I B T F C)) sum |softmax_i(logits) mix - target_i|"""
    if variant == "no_coupling":
        e = torch.exp(logits - logits.max(0, keepdim=True).values.detach())
        s = e / e.sum(0, keepdim=True).detach()
    else:
        s = torch.softmax(logits, dim=0)
    tot = (s * mix[None] - target).abs().sum()
    return tot / (mix.shape[0] if variant == "norm_by_B" else logits.numel())


def loss_and_grads(mix, target, state, cfg, dtype, frozen: bool = False, variant=None):
    """-> (loss, {trainable key: gradient; zeros where the loss does not depend on the tensor}, {norm key: (batch mean, batch var)})"""
    P = params(state, dtype)
    stats = {}
    L = loss_fn(forward(mix.to(dtype), P, cfg, frozen, stats, variant), mix.to(dtype), target.to(dtype), variant)
    keys = [k for k in P if P[k].requires_grad]
    gs = torch.autograd.grad(L, [P[k] for k in keys], allow_unused=True)
    return L.detach(), {k: (g if g is not None else torch.zeros_like(P[k])) for k, g in zip(keys, gs)}, stats


# ---------------------------------------------------------------------------------------------- the optimizer and the running statistics
def running_update(r, batch):
    """r <- m r + (1 - m) batch in the tensors' dtype; 1 - m is the double difference rounded once"""
    m, om = torch.tensor(MOMENTUM).to(r.dtype), torch.tensor(1.0 - MOMENTUM).to(r.dtype)
    return m * r + om * batch.to(r.dtype)


def adam_step(p, g, m, v, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """torch.optim.Adam's single-tensor step (no weight decay, no amsgrad) at 1-based ``step``, in the tensors' dtype -> (p, m, v), with the roundings of torch's CPU
    kernels (lerp and addcmul end in one fused multiply-add, addcdiv scales the numerator first).  The bias corrections and 1 - beta are formed in double and rounded
    once."""
    dt = p.dtype
    c = lambda x: torch.tensor(x, dtype=torch.float64).to(dt)      # noqa: E731
    b1, b2 = betas
    fma = lambda x, y, z: (x.to(torch.float64) * y.to(torch.float64) + z.to(torch.float64)).to(dt)      # noqa: E731  (one rounding: a float32 product is exact in double)
    m = fma(c(1.0 - b1), g - m, m)                       # exp_avg.lerp_(grad, 1 - beta1)
    v = fma(c(1.0 - b2) * g, g, v * c(b2))               # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = torch.sqrt(v) / c(bc2 ** 0.5) + c(eps)
    p = p + (c(-(lr / bc1)) * m) / denom                 # p.addcdiv_(exp_avg, denom, value = -step_size)
    return p, m, v


def train_steps(mix, target, state, cfg, dtype, steps: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """``steps`` Adam steps on one batch -> (the loss before each step, the final state as float arrays of ``dtype``)"""
    cur = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype) for k, v in state.items()}
    mom = {k: (torch.zeros_like(t), torch.zeros_like(t)) for k, t in cur.items() if k.endswith(TRAINABLE)}
    losses = []
    for s in range(1, steps + 1):
        P = {k: (t.clone().requires_grad_(True) if k in mom else t) for k, t in cur.items()}
        stats = {}
        L = loss_fn(forward(mix.to(dtype), P, cfg, False, stats), mix.to(dtype), target.to(dtype))
        keys = list(mom)
        gs = torch.autograd.grad(L, [P[k] for k in keys], allow_unused=True)
        losses.append(float(L.detach()))
        for k, g in zip(keys, gs):
            g = g if g is not None else torch.zeros_like(cur[k])
            cur[k], m, v = adam_step(cur[k], g, mom[k][0], mom[k][1], s, lr, betas, eps)
            mom[k] = (m, v)
        for key, (mean, var) in stats.items():
            cur[f"{key}.mean"] = running_update(cur[f"{key}.mean"], mean)
            cur[f"{key}.var"] = running_update(cur[f"{key}.var"], var)
    return losses, cur
