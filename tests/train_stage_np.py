"""Stage references of the decoder trainer (csrc/dec_train.hip): each row and elementwise kernel as torch on the CPU states it, in the dtype of the tensors handed
in (float64: the reference; float32: the yardstick).  TEST INFRASTRUCTURE ONLY.

Nothing here is a formula derived by hand: forwards are ``F.layer_norm``, ``F.gelu``, ``F.cross_entropy(reduction="none")``, ``F.embedding`` and ``oracle/neox.py``'s
own rotary function (an fp32 angle, then cos / sin, as the engine's table is made), backwards are ``torch.autograd.grad`` of those forwards.  ``chain`` strings the
stages into the whole loss and gradient; tests/test_train_cpu.py holds it to ``train_np.loss_and_grads`` so that no stage reference drifts away from the model.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Sequence

import numpy as np
import torch
import torch.nn.functional as F

import train_np as tn
from oracle import neox

ATTRS = ("pitch_overlap", "polyphony", "note_sustain", "rhythm_intensity")      # the concat order of the four attribute embeddings (and of attrs4)


def T(a, dt) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a)).to(dt)


# ------------------------------------------------------------------ LayerNorm
def ln_fwd(x, g, b, eps):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def ln_stats(x, eps):
    """(mean [M], rstd [M]) as torch's own layer norm saves them"""
    one = torch.ones(x.shape[-1], dtype=x.dtype)
    _, mean, rstd = torch.native_layer_norm(x, (x.shape[-1],), one, one, eps)
    return mean.reshape(-1), rstd.reshape(-1)


def ln_bwd(x, g, b, eps, dy):
    """(dx, d gain, d bias): autograd of F.layer_norm at dy"""
    x, g, b = (t.detach().clone().requires_grad_(True) for t in (x, g, b))
    return torch.autograd.grad(ln_fwd(x, g, b, eps), (x, g, b), dy)


# ------------------------------------------------------------------ GELU
def gelu_fwd(x):
    return F.gelu(x)


def gelu_bwd(x, dy):
    x = x.detach().clone().requires_grad_(True)
    return torch.autograd.grad(F.gelu(x), x, dy)[0]


# ------------------------------------------------------------------ RoPE
def _rope_fwd(qkv, pos, nh, dims):
    M = qkv.shape[0]
    x = qkv.view(M, nh, 3, 64)
    rot = [neox._rope(x[:, :, j].transpose(0, 1)[None], pos, dims)[0].transpose(0, 1) for j in (0, 1)]      # [1, nh, M, 64] in, [M, nh, 64] out
    return torch.stack(rot + [x[:, :, 2]], dim=2).reshape(M, nh * 192)


def rope(qkv, pos, nh, dims, sign=1):
    """qkv [M][nh][q | k | v][64] with q and k rotated at pos [M]; sign -1: the backward pass of that rotation (autograd), which is its inverse"""
    pos = torch.as_tensor(np.asarray(pos), dtype=torch.int64)
    if sign == 1:
        return _rope_fwd(qkv, pos, nh, dims)
    x = torch.zeros_like(qkv).requires_grad_(True)
    return torch.autograd.grad(_rope_fwd(x, pos, nh, dims), x, qkv)[0]


# ------------------------------------------------------------------ attention (tests/test_gpu_train.py holds the kernels to the same statement)
def attn_fwd(qkv, lens, nh):
    outs, r0 = [], 0
    for n in lens:
        x = qkv[r0:r0 + n].view(n, nh, 3, 64)
        q, k, v = x[:, :, 0].transpose(0, 1), x[:, :, 1].transpose(0, 1), x[:, :, 2].transpose(0, 1)
        w = (q @ k.transpose(1, 2)) * 0.125
        w = w.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1)[None], float("-inf"))
        outs.append((torch.softmax(w, -1) @ v).transpose(0, 1).reshape(n, nh * 64))
        r0 += n
    return torch.cat(outs)


def attn_bwd(qkv, lens, nh, dO):
    qkv = qkv.detach().clone().requires_grad_(True)
    return torch.autograd.grad(attn_fwd(qkv, lens, nh), qkv, dO)[0]


# ------------------------------------------------------------------ embeddings
def embed_gather(tables4, attrs4):
    """A4 [M][4 E]: the four attribute rows side by side"""
    return torch.cat([F.embedding(torch.as_tensor(np.asarray(attrs4[k]), dtype=torch.int64), tables4[k]) for k in range(4)], dim=-1)


def embed_sum(word, cemb, ids, cls, h_in):
    i, c = torch.as_tensor(np.asarray(ids), dtype=torch.int64), torch.as_tensor(np.asarray(cls), dtype=torch.int64)
    return (F.embedding(i, word) + F.embedding(c, cemb)) + h_in


def embed_grad(src, col0, width, idx, n_rows, pad, grad0=None):
    """grad0 + the gradient of an nn.Embedding(n_rows, width, padding_idx=pad) looked up at idx, at the upstream gradient src[:, col0 : col0 + width]"""
    w = torch.zeros(n_rows, width, dtype=src.dtype, requires_grad=True)
    out = F.embedding(torch.as_tensor(np.asarray(idx), dtype=torch.int64), w, padding_idx=int(pad))
    g = torch.autograd.grad(out, w, src[:, col0:col0 + width])[0]
    return g if grad0 is None else grad0 + g


# ------------------------------------------------------------------ cross-entropy
def ce(logits, labels, scale):
    """(row_loss [M], 0 where the label is -100; d (scale * sum of row losses) / d logits)"""
    x = logits.detach().clone().requires_grad_(True)
    rl = F.cross_entropy(x, torch.as_tensor(np.asarray(labels), dtype=torch.int64), reduction="none", ignore_index=-100)
    return rl.detach(), torch.autograd.grad(rl.sum() * scale, x)[0]


# ------------------------------------------------------------------ column reductions
def colred(dy, g0, x=None, eps=None, g1=None):
    """mode 0: g0 + the column sums of dy (a bias gradient).  With x: (g0 + LayerNorm's bias gradient, g1 + its gain gradient) at dy"""
    if x is None:
        return g0 + dy.sum(0)
    one, zero = torch.ones(x.shape[-1], dtype=x.dtype), torch.zeros(x.shape[-1], dtype=x.dtype)
    _, dg, db = ln_bwd(x, one, zero, eps, dy)
    return g0 + db, g1 + dg


# ------------------------------------------------------------------ the stages chained: the whole loss and gradient
def chain(state: Dict[str, np.ndarray], cfg, batch, dtype=torch.float64):
    """(loss, gradients) of a right-padded batch through the stage references above, in the order etd_dtrain_forward_backward runs its kernels"""
    sd = {k: T(v, dtype) for k, v in state.items()}
    dims = tn.dims_of(cfg)
    H, E, nh, L, eps = cfg.hidden_size, cfg.attribute_emb_dim, cfg.num_attention_heads, cfg.num_hidden_layers, cfg.layer_norm_eps
    mask = np.asarray(batch["attention_mask"]).astype(bool)
    lens = [int(n) for n in mask.sum(1) if n > 0]
    ids, cls, labels = (np.asarray(batch[k])[mask] for k in ("input_ids", "class_ids", "labels"))
    attrs4 = [np.asarray(batch[k])[mask] for k in ("pitch_overlap_bin_ids", "polyphony_bin_ids", "sustain_bin_ids", "rhythm_intensity_bin_ids")]
    pos = np.concatenate([np.arange(n) for n in lens])
    scored = int((labels != -100).sum())
    lin = lambda x, w, b=None: F.linear(x, sd[w], sd[b] if b else None)      # noqa: E731
    # ---- forward
    A4 = embed_gather([sd[a + "_embeddings.weight"] for a in ATTRS], attrs4)
    hs = [embed_sum(sd["word_embeddings.weight"], sd["class_embeddings.weight"], ids, cls, lin(A4, "attribute_projection.weight", "attribute_projection.bias"))]
    saved = []
    for l in range(L):
        p, h = f"transformer.layers.{l}.", hs[-1]
        x1 = ln_fwd(h, sd[p + "input_layernorm.weight"], sd[p + "input_layernorm.bias"], eps)
        x2 = ln_fwd(h, sd[p + "post_attention_layernorm.weight"], sd[p + "post_attention_layernorm.bias"], eps)
        qkv = rope(lin(x1, p + "attention.query_key_value.weight", p + "attention.query_key_value.bias"), pos, nh, dims)
        att = attn_fwd(qkv, lens, nh)
        a = lin(att, p + "attention.dense.weight", p + "attention.dense.bias")
        pre = lin(x2, p + "mlp.dense_h_to_4h.weight", p + "mlp.dense_h_to_4h.bias")
        m = lin(gelu_fwd(pre), p + "mlp.dense_4h_to_h.weight", p + "mlp.dense_4h_to_h.bias")
        saved.append(dict(x1=x1, x2=x2, qkv=qkv, att=att, pre=pre))
        hs.append((m + a) + h)
    lnf_w, lnf_b = sd["transformer.final_layer_norm.weight"], sd["transformer.final_layer_norm.bias"]
    hf = ln_fwd(hs[-1], lnf_w, lnf_b, eps)
    row_loss, dlogits = ce(lin(hf, "lm_head.weight"), labels, 1.0 / scored)
    loss = float(row_loss.sum()) / scored
    # ---- backward
    G = OrderedDict((k, torch.zeros_like(v)) for k, v in sd.items())
    zero = torch.zeros(H, dtype=dtype)
    G["lm_head.weight"] = dlogits.T @ hf
    dxn = dlogits @ sd["lm_head.weight"]
    G["transformer.final_layer_norm.bias"], G["transformer.final_layer_norm.weight"] = colred(dxn, zero, hs[-1], eps, zero)
    dh = ln_bwd(hs[-1], lnf_w, lnf_b, eps, dxn)[0]
    for l in range(L - 1, -1, -1):
        p, h, s = f"transformer.layers.{l}.", hs[l], saved[l]
        ln1 = (sd[p + "input_layernorm.weight"], sd[p + "input_layernorm.bias"])
        ln2 = (sd[p + "post_attention_layernorm.weight"], sd[p + "post_attention_layernorm.bias"])
        G[p + "mlp.dense_4h_to_h.weight"] = dh.T @ gelu_fwd(s["pre"])
        G[p + "mlp.dense_4h_to_h.bias"] = colred(dh, zero)
        dpre = gelu_bwd(s["pre"], dh @ sd[p + "mlp.dense_4h_to_h.weight"])
        G[p + "mlp.dense_h_to_4h.weight"] = dpre.T @ s["x2"]
        G[p + "mlp.dense_h_to_4h.bias"] = colred(dpre, torch.zeros(dpre.shape[1], dtype=dtype))
        dx2 = dpre @ sd[p + "mlp.dense_h_to_4h.weight"]
        G[p + "post_attention_layernorm.bias"], G[p + "post_attention_layernorm.weight"] = colred(dx2, zero, h, eps, zero)
        G[p + "attention.dense.weight"] = dh.T @ s["att"]
        G[p + "attention.dense.bias"] = colred(dh, zero)
        datt = dh @ sd[p + "attention.dense.weight"]
        dh = dh + ln_bwd(h, *ln2, eps, dx2)[0]
        dqkv = rope(attn_bwd(s["qkv"], lens, nh, datt), pos, nh, dims, sign=-1)
        G[p + "attention.query_key_value.weight"] = dqkv.T @ s["x1"]
        G[p + "attention.query_key_value.bias"] = colred(dqkv, torch.zeros(3 * H, dtype=dtype))
        dx1 = dqkv @ sd[p + "attention.query_key_value.weight"]
        G[p + "input_layernorm.bias"], G[p + "input_layernorm.weight"] = colred(dx1, zero, h, eps, zero)
        dh = dh + ln_bwd(h, *ln1, eps, dx1)[0]
    G["attribute_projection.weight"] = dh.T @ A4
    G["attribute_projection.bias"] = colred(dh, zero)
    dA4 = dh @ sd["attribute_projection.weight"]
    G["word_embeddings.weight"] = embed_grad(dh, 0, H, ids, cfg.vocab_size, cfg.pad_token_id)
    G["class_embeddings.weight"] = embed_grad(dh, 0, H, cls, cfg.num_classes, cfg.pad_class_id)
    for k, a in enumerate(ATTRS):
        G[a + "_embeddings.weight"] = embed_grad(dA4, k * E, E, attrs4[k], cfg.num_attribute_bins, cfg.attribute_pad_id)
    return loss, OrderedDict((k, g.numpy()) for k, g in G.items())
