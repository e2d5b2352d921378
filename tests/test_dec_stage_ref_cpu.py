"""tests/dec_stage_ref.py pinned to the oracle (CPU): chained in float64 without rounding sites the stages ARE oracle.neox.forward_logits (1e-10), in the
prefill form and in the step form (prefix prefilled, one row appended against the cache); with every site on the chain sits inside the 16-bit mode's stated
1e-2 on the benchmark weights; and the near-tie cap of the GPU test's head stage holds for every case with the emulation standing in for the device."""
import functools

import numpy as np
import pytest
import torch

from tests import dec_stage_ref as sr
from tests._util import neox_dims


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int64))


def _oracle(sd, d, p):
    from oracle import neox
    a4 = _t(p[2])
    lg, _ = neox.forward_logits(sd, d, _t(p[0])[None], _t(p[1])[None], {"pitch_overlap": a4[0][None], "polyphony": a4[1][None], "note_sustain": a4[2][None],
                                                                       "rhythm_intensity": a4[3][None]})
    return lg[0]


@functools.lru_cache(maxsize=None)
def _p2(weights):
    sd = {k: v.double() for k, v in sr.state_dict(weights).items()}
    d = neox_dims({})
    ps = sr.prompts(sr.PROMPT_SEED, sr.P2_LENGTHS)
    return sd, d, ps, [_oracle(sd, d, p) for p in ps]


@pytest.mark.parametrize("weights", ["bench", "ctx"])
def test_float64_chain_is_the_oracle(weights):
    sd, d, ps, ref = _p2(weights)
    worst_p = worst_s = 0.0
    for p, want in zip(ps, ref):
        ids, cls, a4 = _t(p[0]), _t(p[1]), _t(p[2])
        got, _ = sr.forward(sd, d, ids, cls, a4)
        worst_p = max(worst_p, float((got - want).abs().max()))
        T = len(ids)
        cache = sr.forward(sd, d, ids[:-1], cls[:-1], a4[:, :-1])[1] if T > 1 else None
        step, _ = sr.forward(sd, d, ids[-1:], cls[-1:], a4[:, -1:], cache=cache)
        worst_s = max(worst_s, float((step[0] - want[-1]).abs().max()))
    print(f"[measured] {weights}: float64 chain vs oracle, prefill form {worst_p:.2e}, step form {worst_s:.2e}")
    assert worst_p <= 1e-10 and worst_s <= 1e-10


def test_emulated_chain_is_inside_the_stated_16_bit_tolerance():
    sd, d, ps, ref = _p2("bench")
    worst = 0.0
    for p, want in zip(ps, ref):
        got, _ = sr.forward(sd, d, _t(p[0]), _t(p[1]), _t(p[2]), sites=sr.ALL_SITES, dtype=torch.float16, prefill=True)
        worst = max(worst, float((got - want).abs().max()))
    print(f"[measured] bench: all sites on (IEEE half), prefill form, max logit error {worst:.3e}")
    assert worst <= 1e-2


def test_key_range_is_the_devices():
    assert [sr.key_range(p, 640) for p in (0, 5, 639, 640, 900)] == [1, 6, 640, 640, 640]


def _emulated_last_hidden(weights, lengths, steps):
    """the emulation (fp32 arithmetic, every site on) standing in for the device: prefill of the case's prompts, then `steps` greedy steps -> the last layer's
    hout of the rows the final logits come from, [n, H] float64"""
    sd = sr.state_dict(weights)
    d = neox_dims({})
    kw = dict(dtype=torch.float16)
    tg = _t(np.asarray(sr.TGT_ATTRS))[:, None]
    rows = []
    for p in sr.prompts(sr.PROMPT_SEED, lengths):
        ids, cls, a4 = _t(p[0]), _t(p[1]), _t(p[2])
        cache, h = None, sr.embed(sd, ids, cls, a4)
        for s in range(steps + 1):
            pos = torch.arange(h.shape[0]) + (0 if cache is None else cache[0][0].shape[1])
            new = []
            for l in range(d.num_hidden_layers):
                h, K, V = sr.layer(sd, l, h, pos, None if cache is None else cache[l][0], None if cache is None else cache[l][1], d,
                                   sr.ALL_SITES if s == 0 else sr.STEP_SITES, prefill=s == 0, **kw)
                new.append((K, V))
            cache, last = new, h[-1:]
            if s < steps:
                tok = sr.head_logits(sd, last, d.layer_norm_eps, sr.STEP_SITES, **kw).argmax(-1)
                h = sr.next_embed(sd, tok, tg)
        rows.append(last[0].double())
    return torch.stack(rows)


@pytest.mark.parametrize("case,weights", [(c, w) for c, ws in sr.CASE_WEIGHTS.items() for w in ws])
def test_near_tie_cap_holds_with_the_emulation_as_the_device(case, weights):
    """the GPU test exempts rows whose float64 top-2 gap is within twice the logit stage's max bound (3 E_max) and caps their share at 5 %: with these seeds the
    emulated device stays under the cap and agrees with the float64 argmax on every other row"""
    hf = _emulated_last_hidden(weights, sr.case_lengths(case), 2 if case.startswith("S") else 0)
    hf = hf[torch.tensor([lim > 2 for lim in sr.case_limits(case)])]      # (S4: the rows still running at the tapped step)
    sd = {k: v.double() for k, v in sr.state_dict(weights).items()}
    eps = neox_dims({}).layer_norm_eps
    ref, emu = sr.head_logits(sd, hf, eps), sr.head_logits(sd, hf, eps, sr.STEP_SITES, torch.float16)
    bound = sr.MAX_X * float((emu - ref).abs().max())
    share, clear = sr.near_tie_share(ref, bound)
    print(f"[measured] {case} {weights}: logit stage max bound {bound:.3e}, rows exempt as near-ties {share:.4f} of {len(hf)}")
    assert share <= sr.TIE_CAP
    assert bool((emu.argmax(-1) == ref.argmax(-1))[clear].all())
