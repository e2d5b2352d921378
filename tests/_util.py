"""Shared helpers for the tests (dims of the golden configs, state-dict conversion)."""
import numpy as np
import torch

from etude_amd import synth

TINY_EXT = dict(n_margin=4, n_frame=16, n_bin=32, cnn_channel=4, cnn_kernel=5, hid_dim=32, pf_dim=64,
                n_heads=4, n_layers_enc=3, n_layers_dec=3, n_note=12, n_velocity=8)
TINY_DEC = dict(vocab_size=154, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                max_position_embeddings=128, attribute_emb_dim=16)
TINY_DEC_KW = dict(gain=2.0, p_eos=0.15)


# ---- stated tolerances of the extractor's 16-bit serving mode against the fp32 reference (north_star: "extractor onset/frame logits within a stated fp tolerance").
# Operands are IEEE half since round 5 (rounds 1-4, bf16 operands: 8e-2 max / 6e-3 mean on probabilities, 0.3 on velocity logits); measured values are printed by
# close_to() (pytest -s) and recorded in profiles/r05_ext_f16.txt.  The exact-parity mode (precision "fp32") is held to 2e-4 in its own tests.
# Measured with IEEE-half operands over every seed and shape the GPU suite uses: probabilities <= 1.94e-2 max (3-min clip: 1.19e-2) / <= 4.1e-4 mean, velocity logits 1.8e-2.
# Those are END-TO-END figures: every stage's rounding accumulated.  Stage by stage, each from the device's own tap of the stage before it, the 16-bit mode is
# held to its own rounding budget instead (tests/test_gpu_extractor_stages.py: max |got - float64| <= 3 E_max, rms <= 2 E_rms, E = the float64 stage with the
# kernels' rounding sites emulated).  Largest ratios measured on MI355X over its six cases, 11 taps + A / B probabilities + velocity logits each:
# 1.13 E_max (n_frame 32, 88 notes: tap 6 dec2; E_max 5.3e-3 at |x| <= 7.7) and 1.01 E_rms (n_frame 64, 128 notes: tap 8 time0); every other stage 0.87-1.08
# E_max and 1.00 E_rms, time_in 0 ulp off the rounded formula in every cell, velocity argmax agreement >= 0.9993 with <= 1.04 % of the cells exempt as near-ties.
EXT_P_TOL, EXT_P_MEAN, EXT_L_TOL = 3e-2, 1e-3, 0.06
# The 16-bit decoder is held the same way (tests/test_gpu_decoder_stages.py, tests/dec_stage_ref.py): every stage of the fused step, the skinny sequence, the batched
# prefill and its last-rows tail -- LayerNorm rows, QKV + RoPE, the appended K / V rows, GELU(up), attention (per-head dense slabs in the fused step), the split-K down
# slabs, the fused prefill MLP, the logits -- from the device's own tap of the stage before it (etd_debug_decoder_stage_taps) and the cache rows read back:
# max |got - float64| <= 3 E_max, rms <= 2 E_rms, E = the float64 stage with the kernels' 16-bit sites on.  Stages without a 16-bit site (slab sum + bias + residual,
# the next embedding) are held per cell to n 2^-24 sum |terms|, gathers and layer hand-overs bit for bit; the emitted token is the argmax of the tapped logits and the
# float64 argmax off near-ties (top-2 gap <= 2 x 3 E_max; share capped at 5 %).  The end-to-end logit bounds of tests/test_gpu_decoder_parity.py (1e-2; 0.12 on the
# context weights) stay what they are: the sum over eight layers of these budgets (tools/diag_rounding_budget.py decoder-stages: per stage E_max 3e-4 .. 2e-3 on the
# benchmark weights, up to 8e-3 on the context weights' queries).
# Measured on the CPU (tests/test_dec_stage_ref_cpu.py): float64 chain vs oracle 8e-15 / 8e-14 on the benchmark / context weights; all sites on: 3.9e-3 of the
# stated 1e-2; near-tie share 0 .. 1.3 % of the 5 % cap.  Worst device ratio per case (stage, layer, E_max): none recorded; the GPU file prints every stage's.
EXT_P_TOL_PAD = 3e-2          # HFT_Transformer wrapper, frames whose receptive field contains its -80 padding rows (bf16 operands needed 1e-1 there)


def close_to(got, ref, tol, mean_tol=None, what=""):
    """assert max |got - ref| < tol (and mean < mean_tol), printing what was measured"""
    e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    mx, mn = float(e.max()), float(e.mean())
    print(f"[measured] {what}: max {mx:.3e} (tol {tol:.1e})" + (f", mean {mn:.3e} (tol {mean_tol:.1e})" if mean_tol else ""))
    assert mx < tol, (what, mx, tol)
    if mean_tol is not None:
        assert mn < mean_tol, (what, mn, mean_tol)


def torch_sd(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def hft_dims(over):
    from oracle.hft import HftDims
    return HftDims(**synth.extractor_dims(**over))


def neox_dims(over):
    from oracle.neox import NeoxDims
    d = synth.decoder_dims(**over)
    return NeoxDims(vocab_size=d["vocab_size"], hidden_size=d["hidden_size"], num_hidden_layers=d["num_hidden_layers"],
                    num_attention_heads=d["num_attention_heads"], intermediate_size=d["intermediate_size"],
                    max_position_embeddings=d["max_position_embeddings"], attribute_emb_dim=d["attribute_emb_dim"],
                    context_num_past_xy_pairs=d["context_num_past_xy_pairs"])


def split_generated(ids, bos):
    """Flat generated id list -> per-bar lists (each starts with Bar_BOS)."""
    bars, cur = [], None
    for t in ids:
        if t == bos:
            if cur is not None:
                bars.append(cur)
            cur = [t]
        else:
            cur.append(t)
    if cur is not None:
        bars.append(cur)
    return bars


# ---- device buffers between guard floats (the stage files' rule: nothing is written outside an output, every float inside is written)
GUARD = 64
NAN_BITS = 0x7FC0DEAD


class Guarded:
    """n floats on the device between two guards.  Guards and inside hold NAN_BITS until a kernel writes them; ``fill`` (a scalar) or ``data`` (n fp32 values, for a
    buffer a kernel updates in place) initialises the inside."""

    def __init__(self, n, fill=None, data=None):
        import ctypes as C
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
        if fill is not None:
            self.buf[GUARD:GUARD + self.n] = fill
        if data is not None:
            d = torch.as_tensor(data).detach().to(torch.float32).contiguous().reshape(-1)
            assert d.numel() == self.n, (d.numel(), self.n)
            self.buf[GUARD:GUARD + self.n] = d.view(torch.int32).cuda()
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def floats(self):
        """the inside, on the host, as fp32"""
        torch.cuda.synchronize()
        return self.buf[GUARD:GUARD + self.n].cpu().view(torch.float32)

    def check(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == NAN_BITS).all(), f"{what}: written below the buffer"
        assert (b[GUARD + self.n:] == NAN_BITS).all(), f"{what}: written beyond the buffer"
        assert not (b[GUARD:GUARD + self.n] == NAN_BITS).any(), f"{what}: a float inside was never written"
