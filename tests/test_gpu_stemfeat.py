"""Stem mel-dB features on the MI355X (csrc/stemfeat.hip, etude_amd.StemFeatures) against the fp64 restatement of DESIGN.md 4d (tests/stemfeat_np.py), their exact
edges and batch invariance, and the route from separated stems through BeatDetector to tempo.json.

Accuracy bound: E = max |engine - fp64 restatement| in dB must satisfy E <= 4 * E32 + 1e-4, E32 being the same maximum for the restatement run in float32
(scipy.fft.rfft on float32 frames and a float32 filterbank product: the arithmetic librosa uses), computed in the same test on the same input.  The factor 4 covers a
different FFT factorisation and the fp32 twiddle table; 1e-4 dB is about 8 ulp of a float32 near 100, for the device's log10f."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import stemfeat_np as sn  # noqa: E402

from etude_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
MAIN_N = 1024 * 40 + 517
BIG_N = 1024 * 600 + 1
_cache = {}


def _stems(N, instr=5, channels=2, seed=11):
    key = (N, instr, channels, seed)
    if key not in _cache:
        x = sn.synthetic_stems(seed, instr=instr, channels=channels, N=N)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def _sf(framing="librosa", **kw):
    from etude_amd.stemfeat import StemFeatures
    key = ("sf", framing, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = StemFeatures(framing=framing, **kw)
    return _cache[key]


def _check(x, framing, **kw):
    """engine against the fp64 restatement, with the float32 restatement's own error as the yardstick"""
    sf = _sf(framing, **kw)
    got = sf.features(torch.from_numpy(np.array(x)).cuda()).cpu().numpy()
    ref = sn.features(x, framing=framing, **kw)
    r32 = sn.features(x, framing=framing, dtype=np.float32, **kw)
    assert got.shape == ref.shape == (x.shape[0], sf.num_frames(x.shape[2]), sf.n_mels)
    assert np.isfinite(got).all()
    E, E32 = float(np.abs(got - ref).max()), float(np.abs(r32 - ref).max())
    print(f"stemfeat {framing} {x.shape} {kw}: E = {E:.3e} dB, E32 = {E32:.3e} dB, bound = {4 * E32 + 1e-4:.3e}, at -80: {(ref <= -80).mean():.2f}")
    assert E <= 4 * E32 + 1e-4, (E, E32)
    assert got.min() >= -80.0 and got.max() <= 0.0
    return got, ref


# (N, instr, channels): every N of the list at both channel counts and both stem counts somewhere
SHAPES = [(1, 1, 1), (1023, 1, 2), (1024, 5, 1), (1025, 1, 1), (2048, 1, 2), (2049, 5, 2), (4097, 1, 1), (4097, 5, 2), (MAIN_N, 5, 2), (MAIN_N, 1, 1),
          (BIG_N, 5, 2)]


@pytest.mark.parametrize("N,instr,channels", SHAPES)
@pytest.mark.parametrize("framing", ["librosa", "spleeter"])
def test_against_restatement(framing, N, instr, channels):
    _check(_stems(N, instr, channels), framing)


@pytest.mark.parametrize("N,instr,channels", [s for s in SHAPES if s[0] >= 2049])
def test_against_restatement_reflect(N, instr, channels):
    _check(_stems(N, instr, channels), "librosa_reflect")


def test_reflect_refuses_short_input():
    with pytest.raises(ValueError, match="librosa_reflect"):
        _sf("librosa_reflect").features(torch.zeros(1, 1, 2048, device="cuda"))


def test_small_transform():
    """n_fft = 256 (an odd log2 of the half length: the radix-2 stage), hop = 64, 32 bands"""
    _check(_stems(64 * 50 + 7, 2, 2), "librosa", n_fft=256, hop=64, n_mels=32)
    _check(_stems(64 * 50 + 7, 2, 2), "librosa_reflect", n_fft=256, hop=64, n_mels=32)


def test_smallest_transform():
    """n_fft = 64: fewer butterflies than threads"""
    _check(_stems(16 * 20 + 3, 1, 1), "spleeter", n_fft=64, hop=16, n_mels=8)


def test_even_log2_transform():
    """log2 of the half length even (6, 8, 10): no radix-2 stage opens the plan, so the pass count and with it the buffer pair that holds the spectrum change parity;
    n_fft = 2048 also has more butterflies per stage than threads"""
    _check(_stems(32 * 40 + 5, 2, 2), "librosa", n_fft=128, hop=32, n_mels=16)
    _check(_stems(32 * 40 + 5, 2, 2), "librosa_reflect", n_fft=128, hop=32, n_mels=16)
    _check(_stems(128 * 30 + 11, 2, 2), "spleeter", n_fft=512, hop=128, n_mels=32)
    _check(_stems(512 * 20 + 3, 2, 2), "librosa", n_fft=2048, hop=512, n_mels=64)


def test_odd_log2_transform_1024():
    """n_fft = 1024 (log2 of the half length = 9), the odd size between 256 and 4096"""
    _check(_stems(256 * 20 + 3, 2, 2), "librosa_reflect", n_fft=1024, hop=256, n_mels=64)


def test_edges_exact():
    x = _stems(MAIN_N)
    for framing in sn.FRAMINGS:
        got = _sf(framing).features(torch.from_numpy(np.array(x)).cuda()).cpu().numpy()
        assert (got[3] == 0.0).all() and not np.signbit(got[3]).any()          # the zero stem
        assert (got[1][12:20] == -80.0).all()                                   # zero frames inside a live stem
        for i in (0, 1, 2, 4):
            assert got[i].max() == 0.0 and got[i].min() >= -80.0
        assert (got == -80.0).mean() > 0.05                                     # the clamp is exercised


def test_invariance_bitwise():
    sf = _sf()
    songs = [_stems(4097, 5, 2, seed=1), _stems(MAIN_N, 5, 2, seed=2), _stems(2049, 5, 2, seed=3)]
    dev = [torch.from_numpy(np.array(s)).cuda() for s in songs]
    alone = [sf.features(d).cpu().numpy() for d in dev]
    packed, Ts = sf.features_many(dev)
    assert Ts == [a.shape[1] for a in alone] and packed.numel() == sum(a.size for a in alone)
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([a.ravel() for a in alone]))
    rev, Tr = sf.features_many(dev[::-1])
    assert Tr == Ts[::-1]
    assert np.array_equal(rev.cpu().numpy(), np.concatenate([a.ravel() for a in alone[::-1]]))
    host, _ = sf.features_many([songs[0], torch.from_numpy(np.array(songs[1])), dev[2]])          # numpy, host tensor, device tensor
    assert np.array_equal(host.cpu().numpy(), packed.cpu().numpy())
    again, _ = sf.features_many(dev)
    assert torch.equal(again, packed)


def test_invariance_bitwise_even_log2():
    """the same at n_fft = 512 (no radix-2 stage): three songs of different lengths, whose last workgroups hold 3, 2 and 4 frames, alone, packed and reversed"""
    sf = _sf("librosa", n_fft=512, hop=128, n_mels=32)
    songs = [_stems(128 * 30 + 11, 2, 2, seed=1), _stems(128 * 57 + 100, 2, 2, seed=2), _stems(128 * 19 + 1, 2, 2, seed=3)]
    dev = [torch.from_numpy(np.array(s)).cuda() for s in songs]
    alone = [sf.features(d).cpu().numpy() for d in dev]
    assert sorted(a.shape[1] % 4 for a in alone) == [0, 2, 3]          # (T = 31, 58, 20: a full last workgroup and two partial ones)
    packed, Ts = sf.features_many(dev)
    assert Ts == [a.shape[1] for a in alone] and packed.numel() == sum(a.size for a in alone)
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([a.ravel() for a in alone]))
    rev, Tr = sf.features_many(dev[::-1])
    assert Tr == Ts[::-1]
    assert np.array_equal(rev.cpu().numpy(), np.concatenate([a.ravel() for a in alone[::-1]]))
    again, _ = sf.features_many(dev)
    assert torch.equal(again, packed)


# ------------------------------------------------------------------ through the detector
@pytest.fixture(scope="module")
def det():
    from etude_amd.beat import BeatDetector
    return BeatDetector(state_dict=synth.beat_state_dict(20240607), tracker="native")


@pytest.fixture(scope="module")
def song_stems():
    return [_stems(1024 * 300 + 77, 5, 2, seed=5), _stems(MAIN_N, 5, 2, seed=6)]


def test_detect_stems_many_equals_detect_many(tmp_path, det, song_stems):
    sf = _sf()
    feats = [sf.features(torch.from_numpy(np.array(s)).cuda()).cpu().numpy() for s in song_stems]
    pa = [tmp_path / "a0.json", tmp_path / "a1.json"]
    pb = [tmp_path / "b0.json", tmp_path / "b1.json"]
    want = det.detect_many(feats, pa)
    got = det.detect_stems_many(song_stems, pb)
    assert got == want
    assert got == det.detect_stems_many([torch.from_numpy(np.array(s)).cuda() for s in song_stems], stem_features=sf)
    for a, b in zip(pa, pb):
        assert a.read_text() == b.read_text()
        assert json.loads(b.read_text()) == want[pa.index(a)]
    acts = det.activations_from_stems_many(song_stems)
    for (b0, d0), (b1, d1) in zip(acts, det.activations_many(feats)):
        assert np.array_equal(b0, b1) and np.array_equal(d0, d1)


def test_structuralize_stems_many_equals_structuralize_many(det, song_stems):
    from etude_amd import structuralize_many, structuralize_stems_many
    sf = _sf()
    feats = [sf.features(torch.from_numpy(np.array(s)).cuda()).cpu().numpy() for s in song_stems]
    assert structuralize_stems_many(det, song_stems) == structuralize_many(det, feats)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_sample_is_refused_before_the_model(det, song_stems, bad):
    want = det.detect_stems_many(song_stems)
    x = np.array(song_stems[1])
    x[2, 1, 20000] = bad
    with pytest.raises(ValueError, match="finite"):
        det.detect_stems_many([song_stems[0], x])
    with pytest.raises(ValueError, match="finite"):
        det.activations_from_stems_many([x])
    assert det.detect_stems_many(song_stems) == want


# ------------------------------------------------------------------ refusals
def test_refusals(det):
    from etude_amd.pipeline import ClipBatchPipeline
    from etude_amd.stemfeat import StemFeatures
    sf = _sf()
    with pytest.raises(ValueError, match=r"\[instr\]\[channels\]\[N\]"):
        sf.features_many([torch.zeros(5, 100, device="cuda")])
    with pytest.raises(ValueError, match="differs"):
        sf.features_many([torch.zeros(5, 2, 100, device="cuda"), torch.zeros(4, 2, 100, device="cuda")])
    with pytest.raises(ValueError, match="differs"):
        sf.features_many([torch.zeros(5, 2, 100, device="cuda"), torch.zeros(5, 1, 100, device="cuda")])
    with pytest.raises(ValueError, match="N >= 1"):
        sf.features_many([torch.zeros(5, 2, 0, device="cuda")])
    with pytest.raises(ValueError, match="power of two"):
        StemFeatures(n_fft=3000)
    with pytest.raises(ValueError, match="instr=5"):
        det.detect_stems_many([torch.zeros(4, 2, 5000, device="cuda")])
    with pytest.raises(ValueError, match="128 mel bands"):
        det.detect_stems_many([torch.zeros(5, 2, 5000, device="cuda")], stem_features=_sf("librosa", n_fft=256, hop=64, n_mels=32))
    with pytest.raises(ValueError, match="one output path"):
        det.detect_stems_many([torch.zeros(5, 2, 5000, device="cuda")], ["a", "b"])
    assert det.detect_stems_many([]) == []
    bare = object.__new__(ClipBatchPipeline)
    with pytest.raises(ValueError, match="not both"):
        bare.extract_stage([None], features=[None], stems=[None])
    # after the refusals the engine still answers
    x = _stems(4097, 5, 2, seed=1)
    assert np.array_equal(sf.features(torch.from_numpy(np.array(x)).cuda()).cpu().numpy(), sf.features(x).cpu().numpy())
