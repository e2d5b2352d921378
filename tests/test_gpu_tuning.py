"""Tuning estimation on the MI355X (csrc/tuning.hip, etude_amd.TuningEstimator) against the fp64 restatement of DESIGN.md 4g (tests/tuning_np.py), every stage on the
device's OWN tapped input; batch invariance, canaries, refusals, the opt-in wiring into the alignment features and the chain from audio to a warping path.

float32 stages (the power P of the first, a middle and the last frame; Y): E = max |device - fp64 restatement| must satisfy E <= 4 * E32 + eps, E32 being the same
maximum for the restatement run in float32 on the same input in the same test and eps 4 float32 ulps of the stage's peak (4f's rule).  Y is checked on the device's own
P only through the frames tapped; its reference is the restatement on the samples.  fp64 stages (Yi, R, sim), each computed by the restatement from the device's own
previous stage: within 1e-9 of the stage's maximum.  The integer: argmax of the device's own sim, and the restatement's integer on every input (all of them decisive,
tests/test_tuning_cpu.py)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import alignfeat_np as an  # noqa: E402
import tuning_np as tn  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
PAD = 4096
_cache = {}


def _est():
    from etude_amd.tuning import TuningEstimator
    if "est" not in _cache:
        _cache["est"] = TuningEstimator()
    return _cache["est"]


def _song(seed, N, cents):
    if (seed, N, cents) not in _cache:
        x = tn.planted_song(seed, N, cents)
        x.setflags(write=False)
        _cache[(seed, N, cents)] = x
    return _cache[(seed, N, cents)]


def _ref(seed, N, cents):
    """the fp64 restatement of a seeded input, computed once"""
    if ("ref", seed, N, cents) not in _cache:
        _cache[("ref", seed, N, cents)] = tn.estimate(_song(seed, N, cents))
    return _cache[("ref", seed, N, cents)]


def _run_tapped(xs, tap=None):
    """one call with buffers of the test's own, canaries around the outputs and the workspace -> per song (tuning, sim, taps); tap = (song, frames) -> also P"""
    est = _est()
    songs = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    Ns, n = [len(x) for x in xs], len(xs)
    nb = est.workspace_bytes(Ns)
    ws = torch.full((nb + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    tun = torch.full((n + 128,), -777, dtype=torch.int32, device="cuda")
    sim = torch.full((n * 100 + 128,), 12345.0, dtype=torch.float64, device="cuda")
    P = None
    if tap is not None:
        P = torch.full((len(tap[1]) * tn.BINS + 128,), 12345.0, dtype=torch.float32, device="cuda")
        est.tap_power(tap[0], tap[1], P[64: 64 + len(tap[1]) * tn.BINS])
    try:
        est.run_raw(songs, tun[64: 64 + n], sim[64: 64 + 100 * n], ws[PAD: PAD + nb])
        torch.cuda.synchronize()
    finally:
        est.tap_power(0, (), None)
    assert bool((ws[:PAD] == 0xA5).all()) and bool((ws[PAD + nb:] == 0xA5).all()), "the workspace canaries were overwritten"
    assert bool((tun[:64] == -777).all()) and bool((tun[64 + n:] == -777).all()), "a tuning canary was overwritten"
    assert bool((sim[:64] == 12345.0).all()) and bool((sim[64 + 100 * n:] == 12345.0).all()), "a sim canary was overwritten"
    if P is not None:
        assert bool((P[:64] == 12345.0).all()) and bool((P[64 + len(tap[1]) * tn.BINS:] == 12345.0).all()), "a power canary was overwritten"
        P = P[64: 64 + len(tap[1]) * tn.BINS].cpu().numpy().reshape(len(tap[1]), tn.BINS)
    host = ws[PAD: PAD + nb].cpu().numpy()
    tun_h, sim_h = tun[64: 64 + n].cpu().numpy(), sim[64: 64 + 100 * n].cpu().numpy().reshape(n, 100)
    res = []
    for s in range(n):
        lay = est.layout(Ns, s)

        def arr(off, count, dtype):
            return host[off: off + count * np.dtype(dtype).itemsize].view(dtype)
        taps = dict(F=lay["F"], G=lay["G"], part=arr(lay["off_part"], lay["G"] * tn.BINS, np.float32).reshape(lay["G"], tn.BINS), Y=arr(lay["off_Y"], tn.BINS, np.float32),
                    Yi=arr(lay["off_Yi"], tn.LOGF, np.float64), R=arr(lay["off_R"], tn.LOGF, np.float64), sim=arr(lay["off_sim"], 100, np.float64))
        res.append((int(tun_h[s]), sim_h[s], taps))
    return res, P


def _bound32(name, got, ref, r32):
    eps = 4 * ULP * float(np.abs(ref).max())
    E, E32 = float(np.abs(got - ref).max()), float(np.abs(r32.astype(np.float64) - ref).max())
    print(f"tuning {name}: E = {E:.3e}, E32 = {E32:.3e}, bound = {4 * E32 + eps:.3e}, E / bound = {E / (4 * E32 + eps):.3f}")
    assert np.isfinite(got).all()
    assert E <= 4 * E32 + eps, (name, E, E32, eps)


def _bound64(name, got, ref):
    peak = float(np.abs(ref).max())
    E = float(np.abs(got - ref).max())
    print(f"tuning {name}: E = {E:.3e}, bound = {1e-9 * peak:.3e} (1e-9 of the stage's maximum {peak:.3e}), E / bound = {E / (1e-9 * peak) if peak else 0.0:.3e}")
    assert np.isfinite(got).all()
    assert E <= 1e-9 * peak, (name, E, peak)


@pytest.mark.parametrize("seed,N,cents", tn.DEVICE_INPUTS)
def test_stages(seed, N, cents):
    x = _song(seed, N, cents)
    F = tn.num_frames(N)
    which = sorted({0, F // 2, F - 1})
    (res,), P = _run_tapped([x], tap=(0, which))
    tuning, sim, tp = res
    assert tp["F"] == F and tp["G"] == -(-F // 8)
    tag = f"N={N}"
    # P of the first, a middle and the last frame: the same windowed samples through the device's FFT, numpy's fp64 FFT and the float32 FFT
    ref = tn.power(tn.frames(x, which))
    r32 = tn.power(tn.frames(x, which, np.float32), np.float32)
    for i, f in enumerate(which):
        _bound32(f"{tag} P frame {f}", P[i], ref[i], r32[i])
    # Y: the sum over time in the contract's groups
    wantY = _ref(seed, N, cents)[1]["Y"]
    _bound32(f"{tag} Y", tp["Y"], wantY, tn.spectrum_sum(x, np.float32))
    y = tp["part"][0].copy()
    for g in range(1, tp["G"]):
        y = y + tp["part"][g]
    assert np.array_equal(y, tp["Y"]), "Y is not the groups' partial sums added in ascending order"
    # the fp64 stages, each on the device's own previous stage
    _bound64(f"{tag} Yi", tp["Yi"], tn.log_frequency(tp["Y"].astype(np.float64)))
    _bound64(f"{tag} R", tp["R"], tn.rectify(tp["Yi"]))
    _bound64(f"{tag} sim", tp["sim"], tn.comb(tp["R"]))
    assert np.array_equal(sim, tp["sim"])
    # the integer
    assert tuning == tn.tuning_of(tp["sim"]) == _ref(seed, N, cents)[0], (tuning, tn.tuning_of(tp["sim"]), _ref(seed, N, cents)[0])
    assert abs((tuning - cents + 50) % 100 - 50) <= 2


def test_silence_and_sinusoid():
    est = _est()
    tun, sim = est.estimate_many([torch.zeros(40000, device="cuda"), tn.sinusoid(40000, 13)], details=True)
    assert tun[0] == -50 and (sim[0] == 0).all()          # the first maximum of a constant
    assert tun[1] == tn.estimate(tn.sinusoid(40000, 13))[0] == 13
    from etude_amd import estimate_tuning
    assert estimate_tuning(tn.sinusoid(40000, 13), 22050) == 13


def test_invariance_bitwise():
    xs = [_song(s, N, d) for s, N, d in tn.DEVICE_INPUTS[:5]]
    alone = [_run_tapped([x])[0][0] for x in xs]
    batch = _run_tapped(xs)[0]
    rev = _run_tapped(xs[::-1])[0][::-1]
    mixed = _run_tapped([xs[4], xs[0], xs[2]])[0]
    for a, b, r in zip(alone, batch, rev):
        for o in (b, r):
            assert a[0] == o[0] and np.array_equal(a[1], o[1]) and np.array_equal(a[2]["Y"], o[2]["Y"]) and np.array_equal(a[2]["sim"], o[2]["sim"])
    for a, o in zip((alone[4], alone[0], alone[2]), mixed):
        assert a[0] == o[0] and np.array_equal(a[1], o[1]) and np.array_equal(a[2]["Y"], o[2]["Y"])
    tun = _est().estimate_many(xs)
    assert list(tun) == [a[0] for a in alone]


def test_refusals():
    from etude_amd import _lib
    est = _est()
    with pytest.raises(ValueError, match="two windows"):
        est.estimate_many([torch.zeros(32767, device="cuda")])
    with pytest.raises(ValueError, match="mono"):
        est.estimate_many([torch.zeros(2, 40000, device="cuda")])
    with pytest.raises(ValueError, match="finite"):
        est.estimate_many([torch.full((40000,), float("nan"), device="cuda")])
    x = torch.zeros(40000, device="cuda")
    short = torch.zeros(32767, device="cuda")
    nb = est.workspace_bytes([40000])
    ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device="cuda")
    tun = torch.full((4,), -777, dtype=torch.int32, device="cuda")
    sim = torch.full((400,), 12345.0, dtype=torch.float64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((ws == 0xA5).all()) and bool((tun == -777).all()) and bool((sim == 12345.0).all())
    with pytest.raises(_lib.EtudeHipError, match=r"rc=-22.*N = 32767"):
        est.run_raw([x, short], tun, sim, torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.EtudeHipError, match=r"rc=-22.*workspace holds"):
        est.run_raw([x], tun, sim, ws[: nb - 256])
    with pytest.raises(_lib.EtudeHipError, match=r"rc=-22.*null output"):
        est.run_raw([x], None, sim, ws)
    with pytest.raises(_lib.EtudeHipError, match=r"rc=-22.*null output"):
        est.run_raw([x], tun, None, ws)
    with pytest.raises(_lib.EtudeHipError, match=r"rc=-22.*songs in one call"):
        est.run_raw([x] * (est.limits["max_songs"] + 1), tun, sim, ws)
    assert untouched(), "a refused call wrote to its buffers"
    # after the refusals the engine still answers
    assert est.estimate(tn.sinusoid(40000, 13)) == 13


def test_features_estimate_wiring():
    from etude_amd.alignfeat import AlignFeatures
    af, est = AlignFeatures(), _est()
    xs = [_song(s, N, d) for s, N, d in tn.DEVICE_INPUTS[:3]]
    tun = est.estimate_many(xs)
    a = af.features_many(xs, "estimate")
    b = af.features_many(xs, [float(t) for t in tun])
    for p, q in zip(a, b):
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])
    zero = af.features_many(xs[:1])[0]          # (the default is still 0 cents: another filterbank than the estimated +1)
    assert tun[0] != 0 and not torch.equal(zero[1], a[0][1])
    with pytest.raises(ValueError, match="estimate"):
        af.features_many(xs, "guess")
    with pytest.raises(ValueError, match="two windows"):
        af.features_many([np.zeros(1000, np.float32)], "estimate")


def test_more_estimates_than_one_handle_holds_banks():
    """70 short sinusoids, each its own number of cents off: the estimates span more than the 64 filterbanks of one handle, the call goes through the bank split"""
    from etude_amd.alignfeat import AlignFeatures
    af, est = AlignFeatures(), _est()
    xs = tn.split_songs()
    tun = est.estimate_many(xs)
    assert list(tun) == [tn.estimate(x)[0] for x in xs]
    assert len(set(tun.tolist())) > af.limits["max_banks"]
    assert len(af._batches([len(x) for x in xs], [float(t) for t in tun])) >= 2
    a = af.features_many(xs, "estimate")
    for i in (0, 63, 64, 69):          # the songs on both sides of the split, each against a call of its own
        one = af.features(xs[i], float(tun[i]))
        assert torch.equal(a[i][0], one[0]) and torch.equal(a[i][1], one[1])


def test_chain_from_detuned_audio(tmp_path):
    from etude_amd.aligner import AudioAligner, align_audio_many
    from etude_amd.alignfeat import default_align_features
    cover, origin, warp, _ = tn.chain_audio()
    tun = _est().estimate_many([cover, origin])
    assert list(tun) == [tn.estimate(cover)[0], tn.estimate(origin)[0]]
    r = align_audio_many([(cover, origin)], "estimate")[0]
    dev = an.path_deviation(r["wp"], warp)
    print(f"tuning chain: estimates {tun[0]:+d} / {tun[1]:+d} for {tn.CHAIN_CENTS:+d} planted, pitch_shift = {r['pitch_shift']}, path within {dev:.2f} frames (bound {tn.CHAIN_BOUND})")
    assert r["pitch_shift"] == an.PLANTED_PITCH_SHIFT
    assert dev <= tn.CHAIN_BOUND
    same = align_audio_many([(cover, origin)], [(float(tun[0]), float(tun[1]))])[0]
    assert np.array_equal(same["wp"], r["wp"])
    # ... and through AudioAligner: the pass-through, and the feature_fn that estimates
    al = AudioAligner()
    assert np.array_equal(al.align_audio_many([(cover, origin)], "estimate")[0]["wp"], r["wp"])
    wavs = {"origin.wav": origin, "cover.wav": cover}
    for name in wavs:
        (tmp_path / name).write_bytes(b"")
    al = AudioAligner(feature_fn=default_align_features().as_feature_fn(lambda p: wavs[Path(p).name], tuning_fn="estimate"))
    got = al.align(tmp_path / "origin.wav", tmp_path / "cover.wav", tmp_path)
    assert got is not None and np.array_equal(got["wp"], r["wp"]) and got["pitch_shift"] == r["pitch_shift"]
