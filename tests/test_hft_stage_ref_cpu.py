"""tests/hft_stage_ref.py pinned to the oracle (CPU): with no rounding site and fp32 inputs, chaining its stage functions IS oracle/hft.py's model_forward.

The GPU stage tests (tests/test_gpu_extractor_stages.py) take their reference and their rounding budget from that helper alone; this file is what makes
the helper the oracle's arithmetic rather than a second opinion, and checks on the CPU what the GPU tests assume of their seeds."""
import numpy as np
import pytest
import torch

from oracle import hft
from tests import hft_stage_ref as sr

# What "fp32 round-off" is comes from the oracle itself: its fp32 run against its own float64 run (same code, double weights and input), per tap.  The
# benchmark checkpoint's first encoder layer is a hard argmax (scores with sigma ~ 3 700) that amplifies a last-bit difference of its input a thousandfold,
# so no fixed figure fits both checkpoints; the oracle's own fp32 error does.  The fp32 chain is another summation order of the same arithmetic (the
# folded embedding; exp(s - max) / sum for torch.softmax): an independent round-off of the same size, whose maximum over 10^6 cells stays within 3 x.
F32_OWN = 3.0
# In float64 the chain must BE the oracle: eps = 2.2e-16 on 512-term dot products through that thousandfold amplification is 1e-10 of the largest value.
F64_REL = 1e-10


def _errs(got, ref64, own32, what):
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err, own, top = float((got.double() - ref64).abs().max()), float((own32.double() - ref64).abs().max()), float(ref64.abs().max())
    print(f"[measured] {what} ({str(got.dtype)[6:]}): max |stage chain - float64 oracle| = {err:.2e}; fp32 oracle's own {own:.2e}; max |oracle| {top:.2e}")
    if got.dtype == torch.float64:
        assert err <= F64_REL * max(top, 1.0), (what, err, top)
    else:
        assert err <= F32_OWN * own, (what, err, own)


@pytest.mark.parametrize("ckpt", ["cal", "bench"])
def test_stage_chain_without_sites_is_the_oracle(ckpt):
    nf = 32
    sd, d, x = sr.case_inputs(nf, 88, 1, ckpt)
    spec = torch.from_numpy(x)
    t32, t64 = {}, {}
    o32 = hft.model_forward(sd, spec, d, t32)
    o64 = hft.model_forward({k: v.double() for k, v in sd.items()}, spec.double(), d, t64)
    names = ("onset", "offset", "mpe", "velocity")
    for dt in (torch.float32, torch.float64):
        prev = enc = None
        for s, name in enumerate(sr.TAP_NAMES):
            prev = sr.tap_stage(s, sd, d, prev, enc=enc, spec=spec.to(dt))
            assert prev.dtype == dt
            if s == 3:
                enc = prev
            if s == 6:
                a_heads = sr.heads_freq(sd, prev, d)
            _errs(prev, t64[name], t32[name], f"{ckpt} tap {s} {name}")
        b_heads = sr.heads_time(sd, prev, d)
        for i in range(4):
            _errs(a_heads[i], o64[i].reshape(a_heads[i].shape), o32[i].reshape(a_heads[i].shape), f"{ckpt} {names[i]} A")
            _errs(b_heads[i], o64[5 + i].reshape(b_heads[i].shape), o32[5 + i].reshape(b_heads[i].shape), f"{ckpt} {names[i]} B")


def test_sites_round_where_they_say_and_nowhere_else():
    """every site moves its stage by about one rounding of the operand type and no site is a no-op; a stage output with Y on is representable in that type"""
    sd8, d8, x = sr.case_inputs(8, 88, 1, "cal")
    taps = {}
    hft.model_forward(sd8, torch.from_numpy(x), d8, taps)
    enc = taps["enc2"].half().double()
    trg = taps["dec0"].half().double()
    for dtype, ulp in ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)):
        ref = sr.decoder_layer(sd8, "decoder.layers_freq.0", enc, trg)
        top = float(ref.abs().max())
        for site in sorted(sr.DEC_SITES - {"X"}):                     # (X is the identity on a 16-bit tap)
            y = sr.decoder_layer(sd8, "decoder.layers_freq.0", enc, trg, sites={site}, dtype=dtype)
            e = float((y - ref).abs().max())
            assert 0 < e < 64 * ulp * top, (site, dtype, e)
        y = sr.decoder_layer(sd8, "decoder.layers_freq.0", enc, trg, sites=sr.DEC_SITES, dtype=dtype)
        assert torch.equal(y, y.to(dtype).double())
    assert torch.equal(sr.decoder_layer(sd8, "decoder.layers_freq.0", enc, trg, sites={"X"}, dtype=torch.float16), ref)
    with pytest.raises(ValueError):
        sr.decoder_layer(sd8, "decoder.layers_freq.0", enc, trg, sites={"Y"})


@pytest.mark.parametrize("nf,nn,nwin,ckpt", [c for c in sr.CASES if c[0] == 32 or c[3] == "bench"], ids=lambda v: str(v))
def test_velocity_near_ties_stay_under_the_cap_for_the_chosen_seeds(nf, nn, nwin, ckpt):
    """The GPU test compares the emitted velocity argmax with the float64 argmax wherever the float64 top-2 gap exceeds 2 E_max of the logits (E_max: what
    rounding the head weights moves them by), and lets at most 2 % of the cells be exempt.  That the REFERENCE alone stays under the cap for the seeds in
    use is a property of the checkpoint and the features, checked here on the oracle's own activations rounded to half (the smallest cases and the
    benchmark checkpoint's; the head weights and the unit-scale LayerNorm outputs they read are drawn the same way in the others)."""
    sd, d, x = sr.case_inputs(nf, nn, nwin, ckpt)
    taps = {}
    hft.model_forward(sd, torch.from_numpy(x), d, taps)
    for name, tap, fn in (("A", "dec2", sr.heads_freq), ("B", "time2", sr.heads_time)):
        t = taps[tap].half().double()
        ref = fn(sd, t, d)[3]
        emu = fn(sd, t, d, sites={"W"}, dtype=torch.float16)[3]
        e_max = float((emu - ref).abs().max())
        top2 = ref.topk(2, -1).values
        exempt = float(((top2[..., 0] - top2[..., 1]) <= 2 * e_max).double().mean())
        print(f"[measured] {nf}/{nn}/{nwin} {ckpt} velocity {name}: E_max {e_max:.2e}, cells within 2 E_max of a tie {exempt:.4f}")
        assert exempt <= 0.02
        assert np.isfinite(ref.numpy()).all()
