"""The float64 stage reference of the Beat-Transformer engine (tests/beat_stage_ref.py; cases, bounds and checker: tests/beat_stage_check.py) on its own, for every case and architecture of
tests/test_gpu_beat_stages.py / test_gpu_beat_archs.py:
  (a) chaining the stage functions from the features equals beat_np.forward (which the reference goldens pin, tests/test_beat_cpu.py) to 1e-12;
  (b) each of seven deliberately wrong stage variants moves its stage's output by at least 100 x the bound the GPU test applies to that stage there;
  (c) the float32 form of every stage, fed to the GPU test's own checker in the device's place, stays inside every bound.
A mutant is asked for where the case can show it: the Er / head-7 / offset-table mutants at every tapped layer whose dilation leaves a second tap inside some song
(T > 2^l: R2 is the only case for layers 7 and 8), the 127-frame tempo segment where a song is longer than 127 frames (R1, R2, R3; the architecture cases are
T = 3 and 70), the mean over instr - 1 stems where instr > 1, the conv padding where the front end is tapped."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_np  # noqa: E402
import beat_stage_check as K  # noqa: E402
import beat_stage_ref as S  # noqa: E402

CASES = ["R1", "R2", "R3"] + list(K.ARCHS)
FACTOR = 100.0


@functools.lru_cache(maxsize=None)
def _case(name):
    dims, sd, feats, mask, front = K.case(name)
    return dims, sd, feats, mask, front, S.chain_call(sd, feats, dims["nlayers"], np.float64)


@pytest.mark.parametrize("name", CASES)
def test_chain_equals_forward(name):
    dims, sd, feats, _, _, c = _case(name)
    I, r0, f0 = dims["instr"], 0, 0
    for i, f in enumerate(feats):
        T = f.shape[1]
        r = beat_np.forward(sd, f, nlayers=dims["nlayers"])
        for got, ref in ((c["logits"][f0:f0 + T], r["logits"]), (c["tempo"][i], r["tempo"]), (c["front"][r0:r0 + I * T], r["front"].reshape(I * T, -1)),
                         (c["x_ffn.0"][r0:r0 + I * T], r["layer0"].reshape(I * T, -1))):
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12
        r0, f0 = r0 + I * T, f0 + T


@pytest.mark.parametrize("name", CASES)
def test_float32_form_is_inside_every_bound(name):
    dims, sd, feats, mask, front, _ = _case(name)
    rep = K.Report(f"{name} fp32 form")
    seen = K.check_call(rep, sd, dims, [f.shape[1] for f in feats], S.chain_call(sd, feats, dims["nlayers"], np.float32), mask, front)
    assert set(seen) >= K.tapped_stages(dims, mask, front) - {"ln1.0", "x_attn.0", "ln1.7", "x_attn.7", "tacc.7"}        # R2 alone leaves these without a tapped input
    assert name == "R2" or set(seen) == K.tapped_stages(dims, mask, front)
    rep.done()


def _layers(mask, L):
    return [l for l in range(L) if (mask >> l) & 1]


@pytest.mark.parametrize("mutant", ["er0", "h7own", "rot", "mask0"])
@pytest.mark.parametrize("name", CASES)
def test_attention_mutants_break_the_bound(name, mutant):
    dims, sd, feats, mask, _, c = _case(name)
    I, Ts = dims["instr"], [f.shape[1] for f in feats]
    sd64 = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    shown = 0
    for l in _layers(mask, dims["nlayers"]):
        if mutant != "mask0" and max(Ts) <= 2 ** l:
            continue                                                  # only the centre tap is inside any song: a softmax over one tap hides all three
        p = S.time_params(sd64, l)
        run = lambda **kw: np.concatenate([S.dattn(p, c[f"qkv.{l}"][rs], I, T, l, **kw) for rs, _, T in S.song_slices(Ts, I)])
        ref = run()
        bound = K.att_bounds(ref, run(dtype=np.float32))[0]
        moved = float(np.abs(run(mutant=mutant) - ref).max())
        print(f"[measured] {name} {mutant} layer {l}: moves skip by {moved / bound:.1f} x its bound")
        assert moved >= FACTOR * bound, (l, moved, bound)
        shown += 1
    assert shown


@pytest.mark.parametrize("name", [n for n in CASES if n != "R2"])
def test_conv_padding_mutant_breaks_the_bound(name):
    dims, sd, feats, _, front, c = _case(name)
    assert front
    I, Ts = dims["instr"], [f.shape[1] for f in feats]
    worst = 0.0
    for f in feats:
        ref, mag = S.conv1(sd, f, mag=True)
        worst = max(worst, float((np.abs(S.conv1(sd, f, pad="neighbour") - ref) / (K.sum_n("c1") * K.EPS32 * mag)).max()))
    print(f"[measured] {name} conv1 padding from the neighbouring stem: {worst:.1f} x its bound")
    assert worst >= FACTOR
    c2 = c["c2"]
    differ = sum(int((S.patch3(c2[rs], I, T, pad="neighbour") != S.patch3(c2[rs], I, T)).sum()) for rs, _, T in S.song_slices(Ts, I))
    assert differ > 0                                                 # bit for bit: any cell


@pytest.mark.parametrize("name", ["R1", "R2", "R3"])
def test_tempo_segment_mutant_breaks_the_bound(name):
    dims, sd, feats, mask, _, c = _case(name)
    tacc = c[f"tacc.{dims['nlayers'] - 1}"]
    worst = 0.0
    for _, fs, T in S.song_slices([f.shape[1] for f in feats], dims["instr"]):
        if T > 127:
            ref, mut = S.tempo_part(tacc[fs], T), S.tempo_part(tacc[fs], T, seg=127)
            assert ref.shape == mut.shape
            worst = max(worst, float((np.abs(mut - ref) / np.maximum(K.sum_n("part") * K.EPS32 * ref, 1e-300)).max()))
    print(f"[measured] {name} 127-frame tempo segment: {worst:.1f} x its bound")
    assert worst >= FACTOR


@pytest.mark.parametrize("name", [n for n in CASES if n != "instr1"])
def test_skip_mean_mutant_breaks_the_bound(name):
    dims, sd, feats, mask, _, c = _case(name)
    I, Ts = dims["instr"], [f.shape[1] for f in feats]
    for l in _layers(mask, dims["nlayers"]):
        worst = 0.0
        for rs, fs, T in S.song_slices(Ts, I):
            prev = None if l == 0 else c[f"tacc.{l - 1}"][fs]
            ref, mag = S.skipacc(c[f"skip.{l}"][rs], prev, I, T, mag=True)
            worst = max(worst, float((np.abs(S.skipacc(c[f"skip.{l}"][rs], prev, I, T, mutant="instr-1") - ref) / (K.sum_n("tacc", I) * K.EPS32 * mag)).max()))
        print(f"[measured] {name} layer {l} skip averaged over instr - 1 stems: {worst:.1f} x its bound")
        assert worst >= FACTOR, l
