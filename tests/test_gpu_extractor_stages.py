"""Every stage of the 16-bit hFT extractor against float64 ON ITS OWN TAPPED INPUT (teacher forcing).

Debug tap k is byte for byte what the device fed stage k + 1, so the float64 stage computed from it (tests/hft_stage_ref.py, pinned to the oracle by
tests/test_hft_stage_ref_cpu.py) is a reference for stage k + 1 alone: nothing of the stages before it accumulates.  The bound comes from the reference
too, never from the device: the same stage with every rounding site of the kernels switched on (`emu`) sits E_max = max |emu - ref| and E_rms away
from `ref`, about one rounding of the operand type, and the device must sit within

    max |got - ref| <= 3 E_max          rms (got - ref) <= 2 E_rms.

What the emulation does not model (fp32 accumulation order, the device's exp2, a site placed slightly differently) moves a result by at most one more
rounding of that size, and the maximum over ~10^6 cells of two independent one-rounding noises is well inside 3 x; the rms has no tail, so a systematic
fault shows there even where every cell stays under the max bound.  The worst ratios measured on MI355X stand beside EXT_P_TOL in tests/_util.py.

Cases (tests/hft_stage_ref.py: CASES) are the smallest at which each path and tile edge exists:

    n_frame 32, n_note 88, 1 window    time attention on k_attn with ONE half-padded key tile (S % 64 != 0); the smallest legal window
    64 / 88 / 2                        time attention on k_attn_frag; the second window walks the (seq * 4 + head) and window strides of every stage
    96 / 88 / 1                        S % 64 != 0 with one full and one ragged key tile
    64 / 128 / 1                       note self-attention without a padded key (n_note at its limit)
    32 / 12 / 1                        note self-attention that is almost all padding; tiny M in every note-major launch
    64 / 88 / 2, benchmark checkpoint  its first encoder layer is a hard argmax: tap 1 is held to the rms bound only (its max is a tail of flipped winners)
"""
import functools

import numpy as np
import pytest
import torch

from etude_amd.config import ExtractorConfig

from tests import hft_stage_ref as sr

pytestmark = pytest.mark.gpu

MAX_X, RMS_X = 3.0, 2.0
OUT_NAMES = ("onset_A", "offset_A", "mpe_A", "velocity_A", "onset_B", "offset_B", "mpe_B", "velocity_B")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}"


@functools.lru_cache(maxsize=None)
def _device_run(nf, nn, nwin, ckpt, chunk):
    """one transcript_windows call with all 11 taps and the velocity-logit buffer registered -> (taps, the 8 outputs, logits, operand dtype), on the host"""
    from etude_amd.extractor import AMTAPC_Extractor
    sd, d, x = sr.case_inputs(nf, nn, nwin, ckpt)
    cfg = ExtractorConfig()
    cfg.input.num_frame, cfg.midi.num_note = nf, nn
    ex = AMTAPC_Extractor(cfg, {k: v.numpy() for k, v in sd.items()}, "cuda", max_windows=4, chunk_frames=chunk)
    assert ex.precision == "f16"
    dev = ex.device
    rows = [nwin * chunk * 256] * 4 + [nwin * chunk * nn] * 3 + [nwin * nn * nf] * 4          # taps 0-6 hold the first chunk only
    bufs = [torch.zeros((r, 256), dtype=ex.operand_dtype, device=dev) for r in rows]
    vl = torch.zeros((nwin * nf, nn, 128), dtype=torch.float32, device=dev)
    try:
        for s, b in enumerate(bufs):
            ex.debug_tap(s, b)
        ex.debug_velocity_logits(vl)
        outs = ex.transcript_windows(torch.from_numpy(x).to(dev), want_A=True)
        torch.cuda.synchronize()
    finally:
        for s in range(len(bufs)):
            ex.debug_tap(s, None)
        ex.debug_velocity_logits(None)
    res = ([b.cpu() for b in bufs], [o.cpu() for o in outs], vl.cpu(), ex.operand_dtype)
    ex.close()
    return res


def _by_seq(fn, *xs, n=32):
    """fn over blocks of n sequences (the float64 attention of 128 sequences at once would hold gigabytes)"""
    if xs[0].shape[0] <= n:
        return fn(*xs)
    parts = [fn(*(x[i:i + n] for x in xs)) for i in range(0, xs[0].shape[0], n)]
    return tuple(torch.cat(p) for p in zip(*parts)) if isinstance(parts[0], tuple) else torch.cat(parts)


@functools.lru_cache(maxsize=None)
def _stages(nf, nn, nwin, ckpt):
    """[(name, got, ref, emu)] of every stage of one case: the 11 taps, the A and B probabilities, the velocity logits.  ref / emu are float64, computed
    from the DEVICE's taps of the preceding stage(s); nothing here compares yet."""
    taps, outs, vl, dt = _device_run(nf, nn, nwin, ckpt, nf)
    sd, d, x = sr.case_inputs(nf, nn, nwin, ckpt)
    sd = {k: v.double() for k, v in sd.items()}
    shapes = [(nwin * nf, 256, 256)] * 4 + [(nwin * nf, nn, 256)] * 3 + [(nwin * nn, nf, 256)] * 4
    t64 = [t.double().reshape(s) for t, s in zip(taps, shapes)]
    spec = torch.from_numpy(x).double()
    res = []
    for s, name in enumerate(sr.TAP_NAMES):
        both = []
        for kw in (dict(), dict(sites=sr.ALL_SITES, dtype=dt)):
            if s == 0:
                y = sr.tap_stage(0, sd, d, None, spec=spec, **kw)
            elif s == 4:
                y = _by_seq(lambda e: sr.tap_stage(4, sd, d, None, enc=e, **kw), t64[3])
            elif s in (5, 6):
                y = _by_seq(lambda p, e: sr.tap_stage(s, sd, d, p, enc=e, **kw), t64[s - 1], t64[3])
            elif s == 7:
                y = sr.tap_stage(7, sd, d, t64[6], **kw)
            else:
                y = _by_seq(lambda p: sr.tap_stage(s, sd, d, p, **kw), t64[s - 1])
            both.append(y)
        res.append((f"tap {s} {name}", t64[s], both[0], both[1]))
    for sfx, fn, src, o0 in (("A", sr.heads_freq, t64[6], 0), ("B", sr.heads_time, t64[10], 4)):
        ref, emu = fn(sd, src, d), fn(sd, src, d, sites={"W"}, dtype=dt)
        for i, n in enumerate(("onset", "offset", "mpe")):
            res.append((f"{n}_{sfx} probability", outs[o0 + i].double(), ref[i], emu[i]))
        if sfx == "B":
            res.append(("velocity_B logits", vl.double(), ref[3], emu[3]))
        res.append((f"velocity_{sfx} argmax", outs[o0 + 3], ref[3], emu[3]))
    return res


def _rms(e):
    return float(e.pow(2).mean().sqrt())


@pytest.mark.parametrize("case", sr.CASES, ids=_case_id)
def test_every_stage_within_its_own_rounding_budget(dev, case):
    nf, nn, nwin, ckpt = case
    bad = []
    for name, got, ref, emu in _stages(*case):
        if name.endswith("argmax"):
            continue
        assert got.shape == ref.shape == emu.shape, (name, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), name
        e_max, e_rms = float((emu - ref).abs().max()), _rms(emu - ref)
        g_max, g_rms = float((got - ref).abs().max()), _rms(got - ref)
        print(f"[measured] {_case_id(case)} {name}: max |got - ref| = {g_max:.3e} = {g_max / e_max:.2f} E_max, rms = {g_rms:.3e} = {g_rms / e_rms:.2f} E_rms"
              f" (max |ref| {float(ref.abs().max()):.2f})")
        max_only_rms = ckpt == "bench" and name.startswith("tap 1 ")           # hard-argmax attention: a heavy tail of flipped winners, held by its rms
        if g_max > MAX_X * e_max and not max_only_rms:
            bad.append((name, "max", g_max, e_max))
        if g_rms > RMS_X * e_rms:
            bad.append((name, "rms", g_rms, e_rms))
        if "probability" in name:
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0, name
    assert not bad, bad


def _ulp(v, dt):
    """distance from |v| to the next value of dt above it (v holds values of dt)"""
    a = v.abs().to(dt)
    up = (a.view(torch.int16) + 1).view(dt)
    return (up.double() - a.double())


@pytest.mark.parametrize("case", sr.CASES, ids=_case_id)
def test_time_in_is_the_permuted_tap_with_one_rounding(dev, case):
    """tap 7 = round(16 tap 6 + pos_embedding_time) in the time-major order: within ONE unit in the last place of the operand type in every cell (the device
    adds in fp32 before it rounds), which no wrong frame, note or window index survives"""
    nf, nn, nwin, ckpt = case
    dt = _device_run(nf, nn, nwin, ckpt, nf)[3]
    name, got, ref, emu = _stages(*case)[7]
    assert name.startswith("tap 7")
    ulps = (got - emu).abs() / _ulp(emu, dt)
    print(f"[measured] {_case_id(case)} time_in: cells off the rounded formula {float((ulps > 0).double().mean()):.2e}, worst {float(ulps.max()):.2f} ulp")
    assert float(ulps.max()) <= 1.0


@pytest.mark.parametrize("case", sr.CASES, ids=_case_id)
def test_velocity_argmax_is_the_float64_argmax_off_near_ties(dev, case):
    for name, got, ref, emu in _stages(*case):
        if not name.endswith("argmax"):
            continue
        assert got.dtype == torch.int8 and got.shape == ref.shape[:-1]
        e_max = float((emu - ref).abs().max())
        top2 = ref.topk(2, -1).values
        clear = (top2[..., 0] - top2[..., 1]) > 2 * e_max
        exempt = 1.0 - float(clear.double().mean())
        agree = got.long() == ref.argmax(-1)
        print(f"[measured] {_case_id(case)} {name}: agreement {float(agree.double().mean()):.4f}, cells exempt as near-ties {exempt:.4f}")
        assert exempt <= 0.02, (name, exempt)
        assert bool(agree[clear].all()), (name, int((~agree[clear]).sum()))


def test_chunked_encoder_is_the_same_bytes(dev):
    """n_frame 64 in two chunks of 32 frames against one chunk of 64: taps 7-10 and all 8 outputs byte for byte; taps 0-6 hold the first chunk of each
    window, so they are compared over those rows"""
    nf, nn, nwin, ckpt = sr.CASES[1]
    assert (nf, nwin) == (64, 2)
    whole, w_outs, w_vl, _ = _device_run(nf, nn, nwin, ckpt, 64)
    part, p_outs, p_vl, _ = _device_run(nf, nn, nwin, ckpt, 32)
    for s in range(7):
        per = 256 if s < 4 else nn
        a = whole[s].reshape(nwin, 64, per, 256)[:, :32]
        b = part[s].reshape(nwin, 32, per, 256)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"tap {s}"
    for s in range(7, 11):
        assert torch.equal(whole[s].view(torch.int16), part[s].view(torch.int16)), f"tap {s}"
    for n, a, b in zip(OUT_NAMES, w_outs, p_outs):
        assert np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8)), n
    assert np.array_equal(w_vl.numpy().view(np.uint8), p_vl.numpy().view(np.uint8))
