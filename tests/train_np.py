"""Restatement of the decoder's training step in plain torch on the CPU.  TEST INFRASTRUCTURE ONLY.

The loss is ``oracle.neox.embed`` + ``transformer`` + ``lm_head`` + ``F.cross_entropy`` under autograd (neither ``embed`` nor ``transformer`` is wrapped in no_grad;
only ``forward_logits`` is), in the dtype of the state handed in: float64 is the reference every bound is taken against, float32 is the reference's own arithmetic
and the yardstick.  Clipping (``clip_grad_norm_``), AdamW (``torch.optim.AdamW``'s single-tensor path) and the cosine schedule are written out by hand.
A right-padded batch is evaluated one sequence at a time over its valid positions: under the causal mask a valid position never reads a padded one, and padded
positions carry no label, so this is the batched forward of the reference (tests/golden/make_golden_train.py runs the reference itself on the padded batch).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from etude_amd.decoder import EtudeDecoderConfig, expected_state_keys
from etude_amd.train import state_shapes
from oracle import neox

FROZEN = "transformer.embed_in.weight"      # in the state dict, never read (the model is fed inputs_embeds): no gradient, AdamW leaves it alone


def tiny_config(**over) -> EtudeDecoderConfig:
    d = dict(vocab_size=157, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, max_position_embeddings=256, num_classes=3,
             num_attribute_bins=3, attribute_emb_dim=64, pad_token_id=0, pad_class_id=0, attribute_pad_id=0)
    d.update(over)
    return EtudeDecoderConfig(**d)


def second_config() -> EtudeDecoderConfig:
    return tiny_config(hidden_size=512, num_attention_heads=8, num_hidden_layers=1, intermediate_size=640)


def dims_of(cfg: EtudeDecoderConfig) -> neox.NeoxDims:
    return neox.NeoxDims(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                         intermediate_size=cfg.intermediate_size, max_position_embeddings=cfg.max_position_embeddings, attribute_emb_dim=cfg.attribute_emb_dim,
                         rotary_pct=cfg.rotary_pct, rope_theta=cfg.rope_theta, layer_norm_eps=cfg.layer_norm_eps)


def seeded_state(cfg: EtudeDecoderConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """fp32 weights in which no parameter is trivial: N(0, 0.05) matrices and tables (zero padding rows), N(0, 0.02) biases, LayerNorm gains 1 + N(0, 0.1)."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for k, shape in state_shapes(cfg).items():
        if ("layernorm" in k or "layer_norm" in k) and k.endswith(".weight"):
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            w = 0.02 * rng.standard_normal(shape)
        else:
            w = 0.05 * rng.standard_normal(shape)
            if k in ("word_embeddings.weight", FROZEN):
                w[cfg.pad_token_id] = 0
            elif k == "class_embeddings.weight":
                w[cfg.pad_class_id] = 0
            elif k.endswith("_embeddings.weight"):
                w[cfg.attribute_pad_id] = 0
        out[k] = w.astype(np.float32)
    return out


def ragged_batch(cfg: EtudeDecoderConfig, lens: Sequence[int], seed: int = 0, ignore_all: Sequence[int] = (), prefix_frac: float = 0.3) -> Dict[str, np.ndarray]:
    """A right-padded batch with the keys of ``EtudeDataset.collate_fn``.  Labels are -100 on a prefix of every sequence (and on the whole of the sequences in
    ``ignore_all``); ids, classes and bins are drawn from the whole table, so pad ids and pad bins appear inside valid positions."""
    rng = np.random.default_rng(seed)
    B, T = len(lens), max(lens)
    b = {"input_ids": np.full((B, T), cfg.pad_token_id, np.int64), "attention_mask": np.zeros((B, T), np.int64), "class_ids": np.full((B, T), cfg.pad_class_id, np.int64),
         "labels": np.full((B, T), -100, np.int64)}
    for k in ("polyphony_bin_ids", "rhythm_intensity_bin_ids", "sustain_bin_ids", "pitch_overlap_bin_ids"):
        b[k] = np.full((B, T), cfg.attribute_pad_id, np.int64)
    for i, n in enumerate(lens):
        b["input_ids"][i, :n] = rng.integers(0, cfg.vocab_size, n)
        b["attention_mask"][i, :n] = 1
        b["class_ids"][i, :n] = rng.integers(0, cfg.num_classes, n)
        for k in ("polyphony_bin_ids", "rhythm_intensity_bin_ids", "sustain_bin_ids", "pitch_overlap_bin_ids"):
            b[k][i, :n] = rng.integers(0, cfg.num_attribute_bins, n)
        if i not in ignore_all:
            p = min(n - 1, int(prefix_frac * n)) if n > 1 else 0
            b["labels"][i, p:n] = rng.integers(0, cfg.vocab_size, n - p)
    return b


def to_torch(state: Dict[str, np.ndarray], dtype, requires_grad: bool = True) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(requires_grad)) for k, v in state.items())


def loss_of(sd: Dict[str, torch.Tensor], cfg: EtudeDecoderConfig, batch: Dict[str, np.ndarray]) -> torch.Tensor:
    """EtudeDecoder.forward(..., labels=...).loss (etude_decoder.py:148-206) of a right-padded batch"""
    d = dims_of(cfg)
    lens = np.asarray(batch["attention_mask"]).sum(axis=1)
    logits, labels = [], []
    for i, n in enumerate(lens):
        n = int(n)
        if n == 0:
            continue
        t = lambda k: torch.as_tensor(np.asarray(batch[k])[i, :n])[None]      # noqa: E731
        attrs = {"pitch_overlap": t("pitch_overlap_bin_ids"), "polyphony": t("polyphony_bin_ids"), "note_sustain": t("sustain_bin_ids"),
                 "rhythm_intensity": t("rhythm_intensity_bin_ids")}
        h, _ = neox.transformer(sd, neox.embed(sd, t("input_ids"), t("class_ids"), attrs), d)
        logits.append(F.linear(h, sd["lm_head.weight"])[0])
        labels.append(torch.as_tensor(np.asarray(batch["labels"])[i, :n]))
    return F.cross_entropy(torch.cat(logits), torch.cat(labels))


def padding_rows(cfg: EtudeDecoderConfig) -> Dict[str, int]:
    """nn.Embedding(padding_idx=...) of the six tables (etude_decoder.py:98-112): that row's gradient is zero.  ``oracle.neox.embed`` indexes plain tensors, so the
    restatement zeroes those rows itself."""
    out = {"word_embeddings.weight": cfg.pad_token_id, "class_embeddings.weight": cfg.pad_class_id}
    for a in ("pitch_overlap", "polyphony", "note_sustain", "rhythm_intensity"):
        out[a + "_embeddings.weight"] = cfg.attribute_pad_id
    return out


def loss_and_grads(state: Dict[str, np.ndarray], cfg: EtudeDecoderConfig, batch, dtype=torch.float64, scale: float = 1.0) -> Tuple[float, "OrderedDict[str, np.ndarray]"]:
    """(loss, scale * d loss / d p for every key; zeros for the frozen table), autograd in ``dtype``"""
    sd = to_torch(state, dtype)
    loss = loss_of(sd, cfg, batch)
    keys = [k for k in sd if k != FROZEN]
    gs = torch.autograd.grad(loss * scale, [sd[k] for k in keys])
    out = OrderedDict((k, np.zeros(tuple(v.shape), np.float64 if dtype == torch.float64 else np.float32)) for k, v in sd.items())
    for k, g in zip(keys, gs):
        out[k] = g.numpy().copy()
    for k, row in padding_rows(cfg).items():
        out[k][row] = 0
    return float(loss.detach()), out


def cosine_schedule_with_warmup(step: int, warmup: int, total: int, num_cycles: float = 0.5) -> float:
    """transformers.get_cosine_schedule_with_warmup's lr_lambda"""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    progress = float(step - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))


def grad_norm(grads: Dict[str, np.ndarray]) -> float:
    """the L2 norm clip_grad_norm_ computes, in float64"""
    return math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for k, g in grads.items() if k != FROZEN))


def clip_and_adamw(params: Dict[str, np.ndarray], grads: Dict[str, np.ndarray], m: Dict[str, np.ndarray], v: Dict[str, np.ndarray], step: int, max_norm: float,
                   lr: float, betas=(0.9, 0.98), eps: float = 1e-8, weight_decay: float = 0.01) -> float:
    """clip_grad_norm_ then torch.optim.AdamW (single-tensor path), in place on numpy arrays of one dtype; ``step`` is the count AFTER this step (1 for the first).
    Returns the norm before clipping."""
    norm = grad_norm(grads)
    dt = next(iter(params.values())).dtype.type
    coef = dt(min(1.0, max_norm / (norm + 1e-6))) if max_norm > 0 else dt(1.0)
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    step_size, bc2_sqrt = dt(lr / bc1), dt(math.sqrt(bc2))
    for k in params:
        if k == FROZEN:
            continue
        g = grads[k].astype(dt) * coef
        grads[k][...] = g
        params[k] *= dt(1.0 - lr * weight_decay)
        m[k] += (g - m[k]) * dt(1.0 - betas[0])
        v[k] *= dt(betas[1])
        v[k] += dt(1.0 - betas[1]) * g * g
        params[k] -= step_size * (m[k] / (np.sqrt(v[k]) / bc2_sqrt + dt(eps)))
    return norm


def torch_clip_and_adamw(params: Dict[str, np.ndarray], grads: Dict[str, np.ndarray], n_steps_before: int, m, v, max_norm, lr, betas=(0.9, 0.98), eps=1e-8,
                         weight_decay=0.01, dtype=torch.float32) -> "OrderedDict[str, np.ndarray]":
    """one clip_grad_norm_ + torch.optim.AdamW step of torch itself in ``dtype`` (moments and step count given); returns the new parameters"""
    keys = [k for k in params if k != FROZEN]
    ps = [torch.tensor(params[k], dtype=dtype, requires_grad=True) for k in keys]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    for p, k in zip(ps, keys):
        p.grad = torch.tensor(grads[k], dtype=dtype)
        opt.state[p] = {"step": torch.tensor(float(n_steps_before)), "exp_avg": torch.tensor(m[k], dtype=dtype), "exp_avg_sq": torch.tensor(v[k], dtype=dtype)}
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
    opt.step()
    out = OrderedDict((k, np.array(params[k])) for k in params)
    for p, k in zip(ps, keys):
        out[k] = p.detach().numpy()
    return out


def trajectory(state: Dict[str, np.ndarray], cfg, batches: Sequence[dict], n_steps: int, dtype=torch.float64, max_norm: float = 1.0, lr: float = 2e-4,
               betas=(0.9, 0.98), eps: float = 1e-8, weight_decay: float = 0.01, lr_fn=None, use_torch_optimizer: bool = False) -> List[List[float]]:
    """``n_steps`` optimizer steps, each over ``batches`` (gradient accumulation with 1 / len(batches)); returns the losses of every batch of every step.
    ``use_torch_optimizer``: torch.optim.AdamW and clip_grad_norm_ themselves instead of the hand-written step."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    params = OrderedDict((k, np.array(v, npdt)) for k, v in state.items())
    m = OrderedDict((k, np.zeros_like(p)) for k, p in params.items())
    v = OrderedDict((k, np.zeros_like(p)) for k, p in params.items())
    out = []
    tps = opt = None
    if use_torch_optimizer:
        tps = to_torch(params, dtype)
        opt = torch.optim.AdamW([tps[k] for k in tps if k != FROZEN], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for s in range(n_steps):
        cur = lr * (lr_fn(s) if lr_fn else 1.0)
        losses = []
        if use_torch_optimizer:
            for g in opt.param_groups:
                g["lr"] = cur
            opt.zero_grad()
            for b in batches:
                loss = loss_of(tps, cfg, b)
                (loss / len(batches)).backward()
                losses.append(float(loss.detach()))
            for k, row in padding_rows(cfg).items():
                tps[k].grad[row] = 0
            torch.nn.utils.clip_grad_norm_([tps[k] for k in tps if k != FROZEN], max_norm)
            opt.step()
        else:
            acc = OrderedDict((k, np.zeros_like(p)) for k, p in params.items())
            for b in batches:
                loss, g = loss_and_grads(params, cfg, b, dtype, 1.0 / len(batches))
                losses.append(loss)
                for k in acc:
                    acc[k] += g[k]
            clip_and_adamw(params, acc, m, v, s + 1, max_norm, cur, betas, eps, weight_decay)
        out.append(losses)
    return out
