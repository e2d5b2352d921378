"""Stage-wise reference of the EtudeDecoder (GPT-NeoX layers) with the 16-bit decoder's rounding sites (CPU, torch; test helper).

Every function computes ONE stage of oracle/neox.py's forward from the activations of the stage before it, in the dtype of its input (float64 for a
reference).  Given the device's own tap of stage k (etd_debug_decoder_stage_taps: byte for byte what the device fed stage k + 1) and the cache rows read
back, the float64 stage is a reference for stage k + 1 ALONE.  tests/test_gpu_decoder_stages.py holds the 16-bit sequences of etude_amd/csrc/api_dec.hip
(fused decode step, skinny sequence, batched prefill, last-rows tail) to that; tests/test_dec_stage_ref_cpu.py pins this file to the oracle.

`sites` switches on roundings to `dtype` (the decoder's operand type) where the kernels of csrc/dec_kernels.hip / dec_prefill.hip / dec_fused.hip store or
pack a 16-bit value; with all of them on a stage function emulates the device stage up to fp32 accumulation order and the device's exp2 / erf:

    W     every Linear weight as uploaded (biases, LayerNorm parameters and the embedding tables stay fp32 on the device)
    LN    LayerNorm rows X1b / X2b (k_ln_rows, k_resid_ln_rows, k_dmlp_fused, k_dstep_head) and the final LayerNorm rows in front of lm_head
    KV    K / V rows as appended to the cache        Qb    the batched prefill's RoPE'd queries (the step and the skinny sequence keep Q in fp32)
    G     GELU(up)                                   P     softmax numerators of k_pattn's PV product (the denominator sums them unrounded; k_dattn keeps fp32)
    O     normalised attention output, the operand of attention.dense

Rows are [M, hidden]; queries / attention outputs are head-major ([head * 64 + d], the device's Q / Xcat layout); K / V rows are [M, heads, 64].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

ALL_SITES = frozenset("W LN KV Qb G P O".split())
STEP_SITES = ALL_SITES - {"Qb", "P"}         # k_dstep_qkv_up + k_dattn / k_dstep_attn_down: fp32 queries, fp32 numerators
TGT_CLASS_ID = 2


class _Rounder:
    def __init__(self, sites, dtype):
        self.sites = frozenset(sites or ())
        if self.sites and dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("rounding sites need dtype torch.float16 or torch.bfloat16")
        self.dtype = dtype

    def __call__(self, name, v):
        return v.to(self.dtype).to(v.dtype) if name in self.sites else v


def _p(l):
    return f"transformer.layers.{l}."


def _w(sd, r, name, like):
    return r("W", sd[name].to(like.dtype))


@torch.no_grad()
def embed(sd, ids, cls, attrs4):
    """oracle/neox.py: embed.  ids / cls [M], attrs4 [4, M] in the library's order (pitch_overlap, polyphony, note_sustain, rhythm_intensity) -> [M, H]"""
    names = ("pitch_overlap", "polyphony", "note_sustain", "rhythm_intensity")
    a = torch.cat([sd[f"{n}_embeddings.weight"][attrs4[i]] for i, n in enumerate(names)], dim=-1)
    proj = F.linear(a, sd["attribute_projection.weight"], sd["attribute_projection.bias"])
    return sd["word_embeddings.weight"][ids] + sd["class_embeddings.weight"][cls] + proj


@torch.no_grad()
def layer_norms(sd, l, h, eps, sites=(), dtype=None):
    """stage `ln`: the residual stream entering layer l -> (X1b, X2b)"""
    r = _Rounder(sites, dtype)
    return tuple(r("LN", F.layer_norm(h, (h.shape[-1],), sd[_p(l) + n + ".weight"].to(h.dtype), sd[_p(l) + n + ".bias"].to(h.dtype), eps))
                 for n in ("input_layernorm", "post_attention_layernorm"))


def rope_tables(pos, rd=16, theta=10000.0):
    """cos / sin [M, rd / 2] as HF (and oracle/neox.py: _rope, and etd_decoder_create) build them: in fp32"""
    inv = 1.0 / (theta ** (torch.arange(0, rd, 2, dtype=torch.float32) / rd))
    fr = torch.as_tensor(pos).float()[:, None] * inv[None, :]
    return fr.cos(), fr.sin()


@torch.no_grad()
def qkv(sd, l, x1, pos, n_heads, sites=(), dtype=None, q_site=None):
    """stage `qkv`: X1b [M, H] and the rows' positions -> (Q [M, H] head-major, K [M, heads, 64], V [M, heads, 64]), RoPE (rotate-half, 16 of 64 dims) on Q and K.
    q_site "Qb": the batched prefill's 16-bit queries."""
    r = _Rounder(sites, dtype)
    M = x1.shape[0]
    y = F.linear(x1, _w(sd, r, _p(l) + "attention.query_key_value.weight", x1), sd[_p(l) + "attention.query_key_value.bias"].to(x1.dtype))
    y = y.reshape(M, n_heads, 3, 64)              # GPT-NeoX's [head][q | k | v][64] rows
    cos, sin = (t.to(x1.dtype)[:, None, :] for t in rope_tables(pos))

    def rot(v):
        a, b = v[..., :8], v[..., 8:16]
        return torch.cat([a * cos - b * sin, b * cos + a * sin, v[..., 16:]], dim=-1)
    q, k, v = rot(y[:, :, 0]), rot(y[:, :, 1]), y[:, :, 2]
    q = q.reshape(M, n_heads * 64)
    return (r(q_site, q) if q_site else q), r("KV", k), r("KV", v)


@torch.no_grad()
def gelu_up(sd, l, x2, sites=(), dtype=None):
    """stage `up`: X2b -> GELU(dense_h_to_4h), erf form (the first `intermediate` columns of Xcat)"""
    r = _Rounder(sites, dtype)
    return r("G", F.gelu(F.linear(x2, _w(sd, r, _p(l) + "mlp.dense_h_to_4h.weight", x2), sd[_p(l) + "mlp.dense_h_to_4h.bias"].to(x2.dtype))))


def key_range(pos, max_ctx):
    """keys a row at position `pos` sees on the device: 0 .. min(pos, max_ctx - 1)"""
    return min(int(pos), int(max_ctx) - 1) + 1


@torch.no_grad()
def attention(q, K, V, n_keys, sites=(), dtype=None, p_site=None):
    """stage `attn`: q [M, H] head-major; K / V [M, heads, >= n_keys[m], 64] = each row's cache rows as the device holds them (or [heads, keys, 64] shared by all rows); row m sees keys 0 .. n_keys[m] - 1
    at scale 1/8 -> normalised output [M, H], rounded at site O.  p_site "P": the numerators are rounded for the PV product (k_pattn)."""
    r = _Rounder(sites, dtype)
    shared = K.dim() == 3                         # one stream's rows against one cache [heads, keys, 64]
    M, nh, nk = q.shape[0], K.shape[-3], K.shape[-2]
    qh = q.reshape(M, nh, 64)
    s = torch.einsum("mhd,hnd->mhn" if shared else "mhd,mhnd->mhn", qh, K) / 8.0
    dead = torch.arange(nk)[None, None, :] >= torch.as_tensor(n_keys)[:, None, None]
    s = s.masked_fill(dead, float("-inf"))
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    den = p.sum(-1, keepdim=True)
    if p_site:
        p = r(p_site, p)
    o = torch.einsum("mhn,hnd->mhd" if shared else "mhn,mhnd->mhd", p, V) / den
    return r("O", o.reshape(M, nh * 64))


def cat_weight(sd, l, like):
    """[dense_4h_to_h | attention.dense] along K, and b2 + bd (etd_decoder_create sums the two in fp32: 2^-24 relative, far below every 16-bit site)"""
    W = torch.cat([sd[_p(l) + "mlp.dense_4h_to_h.weight"], sd[_p(l) + "attention.dense.weight"]], dim=1).to(like.dtype)
    b = sd[_p(l) + "mlp.dense_4h_to_h.bias"].to(like.dtype) + sd[_p(l) + "attention.dense.bias"].to(like.dtype)
    return W, b


@torch.no_grad()
def dense_slabs(sd, l, o, n_heads, sites=(), dtype=None):
    """fused step: head h's share of attention.dense, Wd[:, 64 h .. + 64] o_h -> [heads, M, H]"""
    r = _Rounder(sites, dtype)
    Wd = _w(sd, r, _p(l) + "attention.dense.weight", o)
    return torch.stack([F.linear(o[:, 64 * h:64 * h + 64], Wd[:, 64 * h:64 * h + 64]) for h in range(n_heads)])


@torch.no_grad()
def down_slabs(sd, l, xcat, n_slabs, sites=(), dtype=None):
    """split-K slabs of the (down | dense) projection: slab z = Wcat[:, 512 z .. + 512] xcat[:, 512 z .. + 512] -> [n_slabs, M, H]"""
    r = _Rounder(sites, dtype)
    W = r("W", cat_weight(sd, l, xcat)[0])
    return torch.stack([F.linear(xcat[:, 512 * z:512 * z + 512], W[:, 512 * z:512 * z + 512]) for z in range(n_slabs)])


def resid(sd, l, slabs, hin):
    """hout = sum of the slabs + (b2 + bd) + hin (k_resid_ln_rows: fp32, no 16-bit site)"""
    return slabs.sum(0) + cat_weight(sd, l, hin)[1] + hin


@torch.no_grad()
def mlp_resid(sd, l, x2, attn, hin, sites=(), dtype=None):
    """stage `mlp` in one go (k_dmlp_fused): X2b, the attention block and hin -> hout"""
    r = _Rounder(sites, dtype)
    W, b = cat_weight(sd, l, hin)
    return F.linear(torch.cat([gelu_up(sd, l, x2, sites, dtype), attn], dim=1), r("W", W), b) + hin


@torch.no_grad()
def head_logits(sd, h, eps, sites=(), dtype=None):
    """stage `head`: the last layer's hout -> logits"""
    r = _Rounder(sites, dtype)
    x = r("LN", F.layer_norm(h, (h.shape[-1],), sd["transformer.final_layer_norm.weight"].to(h.dtype), sd["transformer.final_layer_norm.bias"].to(h.dtype), eps))
    return F.linear(x, _w(sd, r, "lm_head.weight", h))


def next_embed(sd, tok, tgt_attrs4):
    """the head kernel's next-step embedding: token `tok` [M] with the target class and the rows' target attributes [4, M]"""
    return embed(sd, tok, torch.full_like(tok, TGT_CLASS_ID), tgt_attrs4)


# ---- the stages chained: what the CPU test pins to the oracle, and tools/diag_rounding_budget.py prints the budget of
@torch.no_grad()
def layer(sd, l, h, pos, K_past, V_past, d, sites=(), dtype=None, prefill=False):
    """One layer over the rows of ONE stream at positions `pos` (consecutive), against its cache so far K_past / V_past [heads, n_past, 64] (or None).
    prefill: the batched prefill's sites (Qb, P).  -> (hout, K, V) with K / V [heads, n_past + M, 64]"""
    kw = dict(sites=sites, dtype=dtype)
    nh = d.num_attention_heads
    x1, x2 = layer_norms(sd, l, h, d.layer_norm_eps, **kw)
    q, k, v = qkv(sd, l, x1, pos, nh, q_site="Qb" if prefill else None, **kw)
    K, V = k.transpose(0, 1), v.transpose(0, 1)
    if K_past is not None:
        K, V = torch.cat([K_past, K], 1), torch.cat([V_past, V], 1)
    o = attention(q, K, V, [int(p) + 1 for p in pos], p_site="P" if prefill else None, **kw)
    xcat = torch.cat([gelu_up(sd, l, x2, **kw), o], dim=1)
    return resid(sd, l, down_slabs(sd, l, xcat, xcat.shape[1] // 512, **kw), h), K, V


@torch.no_grad()
def forward(sd, d, ids, cls, attrs4, cache=None, sites=(), dtype=None, prefill=False):
    """logits [M, V] of one stream's rows (appended behind `cache`, a per-layer list of (K, V), or a fresh stream) and the new cache"""
    past = 0 if cache is None else cache[0][0].shape[1]
    h = embed(sd, ids, cls, attrs4)
    pos = torch.arange(len(ids)) + past
    new = []
    for l in range(d.num_hidden_layers):
        h, K, V = layer(sd, l, h, pos, None if cache is None else cache[l][0], None if cache is None else cache[l][1], d, sites, dtype, prefill)
        new.append((K, V))
    return head_logits(sd, h, d.layer_norm_eps, sites, dtype), new


# ---- shared by the CPU and the GPU test: synthetic prompts and the near-tie rule of the head stage
def prompts(seed, lengths):
    """[(ids, cls, attrs4 [4, T])] int32 numpy, one per length"""
    rng = np.random.default_rng(seed)
    return [(rng.integers(6, 154, T).astype(np.int32), rng.integers(1, 3, T).astype(np.int32), rng.integers(0, 3, (4, T)).astype(np.int32)) for T in lengths]


def near_tie_share(ref_logits, bound):
    """share of rows whose float64 top-2 gap is within 2 x bound (exempt from the argmax check), and the mask of the clear rows"""
    top2 = ref_logits.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * bound
    return 1.0 - float(clear.double().mean()), clear


def ratios(got, ref, emu):
    """(E_max, E_rms, max |got - ref| / E_max, rms (got - ref) / E_rms)"""
    e, g = (emu - ref).double(), (got - ref).double()
    e_max, e_rms = float(e.abs().max()), float(e.pow(2).mean().sqrt())
    return e_max, e_rms, float(g.abs().max()) / e_max, float(g.pow(2).mean().sqrt()) / e_rms


P2_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 192, 513)
S1_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129)
MAX_X, RMS_X, TIE_CAP = 3.0, 2.0, 0.05
PROMPT_SEED = 23


def case_lengths(name):
    """prompt lengths of the GPU test's cases (tests/test_gpu_decoder_stages.py)"""
    rng = np.random.default_rng(PROMPT_SEED)
    if name == "S1":
        return list(S1_LENGTHS) + rng.integers(10, 200, 33 - len(S1_LENGTHS)).tolist()
    if name == "S2":
        return rng.integers(300, 381, 54).tolist()
    if name == "S3":
        return rng.integers(20, 91, 300).tolist()
    return {"S4": [5, 40, 64, 65, 100, 129], "S5": [1], "P1": [1, 65, 130], "P2": list(P2_LENGTHS), "P3": [513] * 96}[name]


def case_limits(name):
    """bar-token limits per stream: S4's streams 1 and 4 emit their second and last token in the first step, so the tapped second step finds them finished"""
    return [8, 2, 8, 8, 2, 8] if name == "S4" else [8] * len(case_lengths(name))


CASE_WEIGHTS = {"S1": ("bench",), "S2": ("ctx",), "S3": ("bench",), "S4": ("bench",), "P1": ("bench",), "P2": ("bench", "ctx")}      # the cases with a head stage
TGT_ATTRS = (2, 1, 1, 1)
WEIGHT_SEED = 1


def state_dict(weights):
    from etude_amd import synth
    sd = synth.decoder_state_dict_ctx(WEIGHT_SEED) if weights == "ctx" else synth.decoder_state_dict(WEIGHT_SEED, {})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
