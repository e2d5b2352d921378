"""Stage-wise reference of the hFT-Transformer with the 16-bit extractor's rounding sites (CPU, torch; test helper).

Every function computes ONE stage of oracle/hft.py's model_forward from the activations of the stage(s) before it, in the dtype of
its input (float64 for a reference, float32 to pin the helper to the oracle: tests/test_hft_stage_ref_cpu.py).  Given the device's
own tap of stage k (byte for byte what the device fed stage k + 1), the float64 stage is a reference for stage k + 1 ALONE: no
rounding of an earlier stage is in it.  tests/test_gpu_extractor_stages.py holds every kernel sequence of the 16-bit mode to that.

`sites` switches on roundings to `dtype` (the extractor's operand type, torch.float16 or torch.bfloat16) where the kernels of
etude_amd/csrc/ext_kernels.hip / ext_fused.hip round; with all of them on, a stage function is an emulation of the device stage that
differs from it by fp32 accumulation order and the device's exp2 only.  The distance between the emulation and the reference is the
stage's own rounding budget -- known without running the device.

    W    weights as uploaded: every Linear weight, the folded conv+embedding map, the 16-bit position tables (biases, LayerNorm
         parameters and pos_embedding_time stay fp32 on the device)
    X    the stage input, operand AND residual (a no-op on a tap, which is 16-bit already)
    Q K V  projected queries / keys / values           P    softmax numerators exp(s - max) (the denominator sums them unrounded)
    O    normalised attention output (operand of fc_o) X1   LayerNorm output after the (self-)attention block
    Qc Kc Vc Pc Oc   the same five sites of a frequency-decoder layer's cross-attention; X2: its LayerNorm output
    H    hidden activations relu(fc_1)                 Y    the stage output

Layouts are the oracle's: frequency-major stages [B * n_frame, n_bin or n_note, hid], time-major stages [B * n_note, n_frame, hid].
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

ENC_SITES = frozenset("W X Q K V P O X1 H Y".split())
DEC_SITES = ENC_SITES | frozenset("Qc Kc Vc Pc Oc X2".split())
ALL_SITES = DEC_SITES
LOG2E = 1.4426950408889634

# (n_frame, n_note, windows, checkpoint) of tests/test_gpu_extractor_stages.py; "cal" = synth.extractor_state_dict_cal, "bench" = synth.extractor_state_dict.
# One checkpoint seed and one feature seed for all of them (tests/test_hft_stage_ref_cpu.py checks what the GPU test needs of these seeds).
CKPT_SEED, FEAT_SEED = 7, 11
CASES = ((32, 88, 1, "cal"), (64, 88, 2, "cal"), (96, 88, 1, "cal"), (64, 128, 1, "cal"), (32, 12, 1, "cal"), (64, 88, 2, "bench"))


def case_inputs(nf, nn, nwin, ckpt):
    """(state dict of fp32 torch tensors, HftDims, features [nwin, 256, nf + 64] fp32 numpy) of one case."""
    from etude_amd import synth
    from oracle import hft
    make = synth.extractor_state_dict_cal if ckpt == "cal" else synth.extractor_state_dict
    sd = {k: torch.from_numpy(v) for k, v in make(CKPT_SEED, dict(n_frame=nf, n_note=nn)).items()}
    return sd, hft.HftDims(n_frame=nf, n_note=nn), synth.window_features(FEAT_SEED, nwin, 256, nf + 64)


class _Rounder:
    def __init__(self, sites, dtype):
        self.sites = frozenset(sites or ())
        if self.sites and dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("rounding sites need dtype torch.float16 or torch.bfloat16")
        self.dtype = dtype

    def __call__(self, name, v):
        return v.to(self.dtype).to(v.dtype) if name in self.sites else v


def _lin(sd, r, pfx, x, wsite="W"):
    return F.linear(x, r(wsite, sd[pfx + ".weight"].to(x.dtype)), sd[pfx + ".bias"].to(x.dtype))


def _ln(sd, pfx, x):
    return F.layer_norm(x, (x.shape[-1],), sd[pfx + ".weight"].to(x.dtype), sd[pfx + ".bias"].to(x.dtype), 1e-5)


def _attention(sd, r, pfx, q_in, kv_in, n_heads, tags, fold_log2e=False, q_exact=False):
    """MHA (oracle/hft.py: mha) with the sites `tags` = (Q, K, V, P, O).  fold_log2e: the queries carry 1/sqrt(head_dim) AND log2(e) before they are rounded
    and the numerators are exp2 (k_enc_layer); otherwise the raw queries are rounded and the scale rides in the exponent (k_attn, k_attn_frag).  q_exact: the
    queries are a constant of the checkpoint, projected with unrounded weights at load and then rounded (the frequency decoder's layer zero)."""
    tq, tk, tv, tp, to = tags
    hid = kv_in.shape[-1]
    hd = hid // n_heads
    split = lambda v: v.reshape(v.shape[0], -1, n_heads, hd).permute(0, 2, 1, 3)      # noqa: E731
    q = _lin(sd, r, pfx + ".fc_q", q_in, wsite=None if q_exact else "W")
    K = r(tk, split(_lin(sd, r, pfx + ".fc_k", kv_in)))
    V = r(tv, split(_lin(sd, r, pfx + ".fc_v", kv_in)))
    if fold_log2e:
        Q = r(tq, split(q) * (LOG2E / math.sqrt(hd)))
        s = torch.matmul(Q, K.transpose(-1, -2))
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
    else:
        Q = r(tq, split(q))
        s = torch.matmul(Q, K.transpose(-1, -2)) / math.sqrt(hd)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
    den = p.sum(-1, keepdim=True)                      # the kernels sum the fp32 numerators, then round them for the PV product
    o = r(to, torch.matmul(r(tp, p), V) / den)
    o = o.permute(0, 2, 1, 3).reshape(o.shape[0], -1, hid)
    return _lin(sd, r, pfx + ".fc_o", o)


def _ffn_ln(sd, r, pfx, x1):
    ff = pfx + ".positionwise_feedforward"
    h = r("H", torch.relu(_lin(sd, r, ff + ".fc_1", x1)))
    return r("Y", _ln(sd, pfx + ".layer_norm", x1 + _lin(sd, r, ff + ".fc_2", h)))


@torch.no_grad()
def embed(sd, spec_in, d, sites=(), dtype=None):
    """oracle/hft.py: encoder_forward up to the "embed" tap, as the ONE [hid][65] map the conv and the Linear fold into (there is nothing non-linear between
    them), applied to features centred on -8 like k_embed does.  spec_in [B, n_bin, n_frame + 2 n_margin] -> [B * n_frame, n_bin, hid]."""
    r = _Rounder(sites, dtype)
    dt = spec_in.dtype
    cw = sd["encoder.conv.weight"].double().reshape(d.cnn_channel, d.cnn_kernel)
    cb = sd["encoder.conv.bias"].double()
    npos = d.n_proc - (d.cnn_kernel - 1)
    tw = sd["encoder.tok_embedding_freq.weight"].double().reshape(d.hid_dim, d.cnn_channel, npos)
    fold = torch.zeros((d.hid_dim, d.n_proc), dtype=torch.float64)
    for k in range(d.cnn_kernel):
        fold[:, k:k + npos] += (tw * cw[None, :, k, None]).sum(1)
    bias = sd["encoder.tok_embedding_freq.bias"].double() + (tw.sum(2) * cb[None]).sum(1)
    center = -8.0
    Wf = r("W", fold.to(dt))
    b = (bias + center * Wf.double().sum(1)).to(dt)                      # x = (x - center) + center, against the weights the product really uses
    B = spec_in.shape[0]
    u = spec_in.unfold(2, d.n_proc, 1).permute(0, 2, 1, 3).reshape(B * d.n_frame, d.n_bin, d.n_proc)
    y = F.linear(r("X", u - center), Wf, b)
    return r("Y", y * math.sqrt(d.hid_dim) + r("W", sd["encoder.pos_embedding_freq.weight"].to(dt))[None])


@torch.no_grad()
def encoder_layer(sd, pfx, x, n_heads=4, sites=(), dtype=None, fold_log2e=False):
    """oracle/hft.py: encoder_layer (one shared LayerNorm) -- the encoder's layers_freq (k_enc_layer: fold_log2e=True) and the decoder's layers_time."""
    r = _Rounder(sites, dtype)
    x = r("X", x)
    a = _attention(sd, r, pfx + ".self_attention", x, x, n_heads, ("Q", "K", "V", "P", "O"), fold_log2e)
    x1 = r("X1", _ln(sd, pfx + ".layer_norm", x + a))
    return _ffn_ln(sd, r, pfx, x1)


@torch.no_grad()
def decoder_layer_zero(sd, pfx, enc, pos, n_heads=4, sites=(), dtype=None):
    """oracle/hft.py: decoder_layer_zero.  enc [N, n_bin, hid] (the encoder output), pos = decoder.pos_embedding_freq.weight [n_note, hid]: the target of
    every frame, so its queries are a constant."""
    r = _Rounder(sites, dtype)
    enc = r("X", enc)
    pos = pos.to(enc.dtype)[None]
    a = _attention(sd, r, pfx + ".encoder_attention", pos, enc, n_heads, ("Qc", "Kc", "Vc", "Pc", "Oc"), q_exact=True)
    x2 = r("X2", _ln(sd, pfx + ".layer_norm", r("W", pos) + a))
    return _ffn_ln(sd, r, pfx, x2)


@torch.no_grad()
def decoder_layer(sd, pfx, enc, trg, n_heads=4, sites=(), dtype=None):
    """oracle/hft.py: decoder_layer.  enc [N, n_bin, hid], trg [N, n_note, hid] (the previous frequency-decoder layer's output)."""
    r = _Rounder(sites, dtype)
    enc, trg = r("X", enc), r("X", trg)
    a = _attention(sd, r, pfx + ".self_attention", trg, trg, n_heads, ("Q", "K", "V", "P", "O"))
    x1 = r("X1", _ln(sd, pfx + ".layer_norm", trg + a))
    a = _attention(sd, r, pfx + ".encoder_attention", x1, enc, n_heads, ("Qc", "Kc", "Vc", "Pc", "Oc"))
    x2 = r("X2", _ln(sd, pfx + ".layer_norm", x1 + a))
    return _ffn_ln(sd, r, pfx, x2)


@torch.no_grad()
def time_in(sd, x, d, sites=(), dtype=None):
    """oracle/hft.py: decoder_forward's "time_in": [B * n_frame, n_note, hid] -> [B * n_note, n_frame, hid], x * 16 + pos_embedding_time (ONE rounding)."""
    r = _Rounder(sites, dtype)
    t = x.reshape(-1, d.n_frame, d.n_note, d.hid_dim).permute(0, 2, 1, 3).reshape(-1, d.n_frame, d.hid_dim)
    return r("Y", t * math.sqrt(d.hid_dim) + sd["decoder.pos_embedding_time.weight"].to(x.dtype)[None])


def _heads(sd, r, sfx, x):
    on, off, mpe = (torch.sigmoid(_lin(sd, r, f"decoder.fc_{n}_{sfx}", x))[..., 0] for n in ("onset", "offset", "mpe"))
    return on, off, mpe, _lin(sd, r, f"decoder.fc_velocity_{sfx}", x)


@torch.no_grad()
def heads_freq(sd, x, d, sites=(), dtype=None):
    """The A outputs from the last frequency-decoder layer [B * n_frame, n_note, hid]: onset / offset / mpe probabilities [B * n_frame, n_note] and the
    velocity logits [B * n_frame, n_note, n_velocity].  (The probabilities and logits are fp32 on the device: the only site is W.)"""
    return _heads(sd, _Rounder(sites, dtype), "freq", x)


@torch.no_grad()
def heads_time(sd, t, d, sites=(), dtype=None):
    """The B outputs from the last time layer [B * n_note, n_frame, hid], in the layout of the A outputs."""
    on, off, mpe, vel = _heads(sd, _Rounder(sites, dtype), "time", t)
    fm = lambda v: v.reshape(-1, d.n_note, d.n_frame).transpose(1, 2).reshape(-1, d.n_note)      # noqa: E731
    vel = vel.reshape(-1, d.n_note, d.n_frame, d.n_velocity).transpose(1, 2).reshape(-1, d.n_note, d.n_velocity)
    return fm(on), fm(off), fm(mpe), vel


TAP_NAMES = ("embed", "enc0", "enc1", "enc2", "dec0", "dec1", "dec2", "time_in", "time0", "time1", "time2")   # etd_extractor_debug_tap's stage numbers


def tap_stage(s, sd, d, prev, enc=None, spec=None, sites=(), dtype=None):
    """Stage s (a debug-tap number, 0-10) from `prev`, the output of stage s - 1 (spec for stage 0; the frequency decoder also takes `enc`, the output of stage 3)."""
    kw = dict(sites=sites, dtype=dtype)
    if s == 0:
        return embed(sd, spec, d, **kw)
    if s <= 3:
        return encoder_layer(sd, f"encoder.layers_freq.{s - 1}", prev, d.n_heads, fold_log2e=True, **kw)
    if s == 4:
        return decoder_layer_zero(sd, "decoder.layer_zero_freq", enc, sd["decoder.pos_embedding_freq.weight"], d.n_heads, **kw)
    if s <= 6:
        return decoder_layer(sd, f"decoder.layers_freq.{s - 5}", enc, prev, d.n_heads, **kw)
    if s == 7:
        return time_in(sd, prev, d, **kw)
    return encoder_layer(sd, f"decoder.layers_time.{s - 8}", prev, d.n_heads, **kw)
