#!/usr/bin/env python3
"""Which bf16 rounding of the extractor's EncoderLayer owns its error?  (CPU, torch fp32 + emulated bf16 roundings; no GPU, no library.)

The bf16 extractor sits 1.2-1.3 % rms off the fp32 reference after EVERY encoder layer (profiles/r02_error_budget.txt); the layer's LayerNorms renormalise, so
the figure does not grow from layer to layer -- it is made inside one layer.  This script runs encoder layer 0 of the oracle (oracle/hft.py, amt_apc.py:244-259)
on real embedded frames of a synthetic window and rounds to bf16 exactly where csrc/ext_fused.hip's k_enc_layer does -- one site at a time, then cumulatively:

    W      weights                                   X     the layer input (operand AND residual)
    Q, K   projected queries (pre-scaled) / keys     V     projected values
    P      softmax numerators exp(s - max)           O     normalised attention output (operand of fc_o)
    X1     LayerNorm output (operand of the feed-forward block AND its residual)
    H      hidden activations relu(fc_1)             Y     the layer output

Prints rms(err) / rms(ref) and max|err| of the layer output per site.  usage: python tools/diag_rounding_budget.py [n_frames=16]

`python tools/diag_rounding_budget.py stages [n_frames=8]` prints instead what every layer costs in IEEE half from its exact 16-bit input, against float64.
The rounding sites are those of tests/hft_stage_ref.py: this script and the GPU stage tests share one emulation.

`python tools/diag_rounding_budget.py decoder-stages [tokens=65]` does the same for the 16-bit decoder, per layer and stage, with the sites of
tests/dec_stage_ref.py (the budget tests/test_gpu_decoder_stages.py holds the device to), for both synthetic weight sets."""
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from etude_amd import synth  # noqa: E402
from oracle import hft  # noqa: E402
from tests.hft_stage_ref import encoder_layer  # noqa: E402


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def layer(sd, pfx, x, sites, n_heads=4):
    """the layer with bf16 roundings at `sites`: tests/hft_stage_ref.py, the emulation the GPU stage tests take their bounds from"""
    return encoder_layer(sd, pfx, x, n_heads, sites=sites, dtype=torch.bfloat16)


def stage_table(nfr):
    """Every layer from its EXACT 16-bit input (the oracle's own tap rounded to IEEE half), float64, all sites on: what one stage costs when nothing
    accumulates -- the budget tests/test_gpu_extractor_stages.py holds the device to."""
    from tests.hft_stage_ref import CKPT_SEED, FEAT_SEED, ENC_SITES
    print(f"n_frame {nfr}, checkpoint seed {CKPT_SEED}, window_features({FEAT_SEED}, ...), IEEE-half sites {' '.join(sorted(ENC_SITES))}")
    print("layer (from its exact 16-bit input)   bench ckpt max / rms      cal ckpt max / rms        max |output|")
    d = hft.HftDims(n_frame=nfr)
    x = torch.from_numpy(synth.window_features(FEAT_SEED, 1, 256, nfr + 2 * d.n_margin))
    rows = {}
    for make in (synth.extractor_state_dict, synth.extractor_state_dict_cal):
        sd = {k: torch.from_numpy(v) for k, v in make(CKPT_SEED, dict(n_frame=nfr)).items()}
        taps = {}
        hft.model_forward(sd, x, d, taps)
        sd64 = {k: v.double() for k, v in sd.items()}
        for pfx, src, fold in (("encoder.layers_freq.0", "embed", True), ("encoder.layers_freq.1", "enc0", True), ("encoder.layers_freq.2", "enc1", True),
                               ("decoder.layers_time.0", "time_in", False), ("decoder.layers_time.1", "time0", False)):
            xin = taps[src].half().double()
            ref = encoder_layer(sd64, pfx, xin, d.n_heads, fold_log2e=fold)
            emu = encoder_layer(sd64, pfx, xin, d.n_heads, sites=ENC_SITES, dtype=torch.float16, fold_log2e=fold)
            e = emu - ref
            rows.setdefault(pfx, []).append((float(e.abs().max()), float(e.pow(2).mean().sqrt()), float(ref.abs().max())))
    for pfx, ((bm, br, bt), (cm, cr, ct)) in rows.items():
        print(f"{pfx:36s}  {bm:.1e} / {br:.1e}         {cm:.1e} / {cr:.1e}         {min(bt, ct):.1f} - {max(bt, ct):.1f}")


def decoder_stage_table(T):
    """Every decoder stage from its exact input (the float64 chain's own activations, rounded where the device hands the stage a 16-bit tensor), all sites of
    the batched prefill on: E_max / E_rms per layer."""
    from tests import dec_stage_ref as sr
    from tests._util import neox_dims
    d = neox_dims({})
    ids, cls, a4 = (torch.from_numpy(np.ascontiguousarray(v).astype(np.int64)) for v in sr.prompts(sr.PROMPT_SEED, [T])[0])
    kw = dict(sites=sr.ALL_SITES, dtype=torch.float16)
    half = lambda v: v.half().double()      # noqa: E731
    e = lambda emu, ref: f"{float((emu - ref).abs().max()):.1e} / {float((emu - ref).pow(2).mean().sqrt()):.1e}"      # noqa: E731
    for weights in ("bench", "ctx"):
        sd = {k: v.double() for k, v in sr.state_dict(weights).items()}
        print(f"{weights} weights, one prompt of {T} tokens, IEEE-half sites {' '.join(sorted(sr.ALL_SITES))}: E_max / E_rms per stage from its exact input")
        print("prefill sites (Qb, P; k_pattn, k_dmlp_fused) | step sites (fp32 Q, k_dattn / k_dstep_attn_down, split-K slabs)")
        print("layer  ln                   qkv Q                K append             V append             attn                 mlp hout           | "
              "step Q               up GELU              step attn            dense slabs          down slabs")
        h, pos = sr.embed(sd, ids, cls, a4), torch.arange(T)
        for l in range(d.num_hidden_layers):
            x1, x2 = sr.layer_norms(sd, l, h, d.layer_norm_eps)
            ln = e(torch.cat(sr.layer_norms(sd, l, h, d.layer_norm_eps, **kw), 1), torch.cat([x1, x2], 1))
            x1, x2 = half(x1), half(x2)
            q, k, v = sr.qkv(sd, l, x1, pos, d.num_attention_heads)
            qe, ke, ve = sr.qkv(sd, l, x1, pos, d.num_attention_heads, q_site="Qb", **kw)
            q32 = q
            q, K, V = half(q), half(k).transpose(0, 1), half(v).transpose(0, 1)
            nk = list(range(1, T + 1))
            o = sr.attention(q, K, V, nk)
            oe = sr.attention(q, K, V, nk, p_site="P", **kw)
            o16 = half(o)
            hout = sr.mlp_resid(sd, l, x2, o16, h)
            # the step's / skinny sequence's stages (STEP_SITES) from the same exact inputs: fp32 queries, GELU(up), attention with fp32 numerators, the per-head
            # dense slabs and the split-K slabs of the (down | dense) projection
            skw = dict(sites=sr.STEP_SITES, dtype=torch.float16)
            nh = d.num_attention_heads
            g = sr.gelu_up(sd, l, x2)
            os_ = sr.attention(q32, K, V, nk)
            xcat = torch.cat([half(g), half(os_)], 1)
            step = (e(sr.qkv(sd, l, x1, pos, nh, **skw)[0], q32), e(sr.gelu_up(sd, l, x2, **skw), g), e(sr.attention(q32, K, V, nk, **skw), os_),
                    e(sr.dense_slabs(sd, l, sr.attention(q32, K, V, nk, **skw), nh, **skw), sr.dense_slabs(sd, l, os_, nh)),
                    e(sr.down_slabs(sd, l, xcat, 5, **skw), sr.down_slabs(sd, l, xcat, 5)))
            print(f"{l:5d}  {ln:19s}  {e(qe, q):19s}  {e(ke, k):19s}  {e(ve, v):19s}  {e(oe, o):19s}  {e(sr.mlp_resid(sd, l, x2, o16, h, **kw), hout):19s}| " +
                  "  ".join(f"{x:19s}" for x in step))
            h = hout
        ref = sr.head_logits(sd, h, d.layer_norm_eps)
        print(f"head logits {e(sr.head_logits(sd, h, d.layer_norm_eps, **kw), ref)} (max |logit| {float(ref.abs().max()):.1f})")
        tok = ref.argmax(-1)
        nh_ = sr.next_embed(sd, tok, torch.tensor(sr.TGT_ATTRS)[:, None].expand(4, T))
        print(f"head next ln {e(torch.cat(sr.layer_norms(sd, 0, nh_, d.layer_norm_eps, **kw), 1), torch.cat(sr.layer_norms(sd, 0, nh_, d.layer_norm_eps), 1))}"
              " (slab sum + bias + residual and the next embedding have no 16-bit site: E = 0, held to n 2^-24 sum |terms|)")


def main():
    torch.set_num_threads(8)
    if len(sys.argv) > 1 and sys.argv[1] == "decoder-stages":
        with torch.no_grad():
            decoder_stage_table(int(sys.argv[2]) if len(sys.argv) > 2 else 65)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "stages":
        with torch.no_grad():
            stage_table(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
        return
    nfr = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    sd = {k: torch.from_numpy(v) for k, v in synth.extractor_state_dict(0).items()}
    d = hft.HftDims()
    x = torch.from_numpy(synth.window_features(5, 1))
    taps = {}
    with torch.no_grad():
        # the embedded frames (amt_apc.py:74-99) of the first nfr frames of the window
        sub = x[:, :, : nfr + 2 * d.n_margin]
        d2 = hft.HftDims(n_frame=nfr)
        hft.encoder_forward(sd, sub, d2, taps)
        emb = taps["embed"]                                  # [nfr, 256, 256]
        pfx = "encoder.layers_freq.0"
        ref = layer(sd, pfx, emb, set())
        assert torch.allclose(ref, taps["enc0"], atol=2e-4), float((ref - taps["enc0"]).abs().max())
        rms = lambda e: float(e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())      # noqa: E731
        sites = ["W", "X", "Q", "K", "V", "P", "O", "X1", "H", "Y"]
        print(f"encoder layer 0 on {nfr} frames x 256 bins; output rms {float(ref.pow(2).mean().sqrt()):.3f}")
        print("site            rms err / rms ref    max |err|")
        for sname in sites:
            y = layer(sd, pfx, emb, {sname})
            print(f"only {sname:3s}        {rms(y - ref):.4e}          {float((y - ref).abs().max()):.3e}")
        cum = set()
        for sname in sites:
            cum.add(sname)
            y = layer(sd, pfx, emb, cum)
            print(f"+ {sname:3s} (cum.)     {rms(y - ref):.4e}          {float((y - ref).abs().max()):.3e}")
        for drop in (["Q", "K"], ["P"], ["X", "X1"], ["Q", "K", "P"], ["W"]):
            y = layer(sd, pfx, emb, set(sites) - set(drop))
            print(f"all but {'+'.join(drop):8s} {rms(y - ref):.4e}          {float((y - ref).abs().max()):.3e}")
        # the same for layer 1, whose input is a LayerNorm output (unit scale): exact (fp32) input, all roundings on
        pf1 = "encoder.layers_freq.1"
        ref1 = layer(sd, pf1, taps["enc0"], set())
        y1 = layer(sd, pf1, taps["enc0"], set(sites))
        Q1 = F.linear(taps["enc0"], sd[pf1 + ".self_attention.fc_q.weight"], sd[pf1 + ".self_attention.fc_q.bias"]).view(nfr, -1, 4, 64).permute(0, 2, 1, 3) / 8.0
        K1 = F.linear(taps["enc0"], sd[pf1 + ".self_attention.fc_k.weight"], sd[pf1 + ".self_attention.fc_k.bias"]).view(nfr, -1, 4, 64).permute(0, 2, 1, 3)
        print(f"layer 1 from its EXACT input, every rounding on: rms {float((y1 - ref1).pow(2).mean().sqrt() / ref1.pow(2).mean().sqrt()):.4e}, max {float((y1 - ref1).abs().max()):.3e}"
              f" (its scores: std {float(torch.matmul(Q1, K1.permute(0, 1, 3, 2)).std()):.2f})")
        # statistics that explain the Q / K figure: the spread of the scores a rounding error is exponentiated through
        sa = pfx + ".self_attention"
        Q = F.linear(emb, sd[sa + ".fc_q.weight"], sd[sa + ".fc_q.bias"]).view(nfr, -1, 4, 64).permute(0, 2, 1, 3) / 8.0
        K = F.linear(emb, sd[sa + ".fc_k.weight"], sd[sa + ".fc_k.bias"]).view(nfr, -1, 4, 64).permute(0, 2, 1, 3)
        s = torch.matmul(Q, K.permute(0, 1, 3, 2))
        sb = torch.matmul(bf(Q), bf(K).permute(0, 1, 3, 2))
        print(f"scores: std {float(s.std()):.2f}, |max| {float(s.abs().max()):.1f}; bf16 Q, K move a score by rms {float((sb - s).pow(2).mean().sqrt()):.4f} (max {float((sb - s).abs().max()):.3f})"
              " -> that much RELATIVE error in every softmax numerator")


if __name__ == "__main__":
    main()
