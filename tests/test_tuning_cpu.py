"""Tuning estimation on the host: the fp64 restatement of DESIGN.md 4g (tests/tuning_np.py) against scipy's spline and numpy's FFT, on hand-made cases and planted
detunings; the decisiveness of every seeded input the device tests compare as an integer; the host restatement of the chain from audio to a warping path; and the C
ABI's host-only entry points."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import alignfeat_np as an  # noqa: E402
import dtw_np as dn  # noqa: E402
import tuning_np as tn  # noqa: E402

_cache = {}


def _song(seed, N, cents):
    if (seed, N, cents) not in _cache:
        x = tn.planted_song(seed, N, cents)
        x.setflags(write=False)
        _cache[(seed, N, cents)] = x
    return _cache[(seed, N, cents)]


def _est(seed, N, cents, dtype=np.float64):
    key = ("est", seed, N, cents, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = tn.estimate(_song(seed, N, cents), dtype)
    return _cache[key]


# ------------------------------------------------------------------ the restatement itself
def test_spline_against_scipy():
    """the restatement's own tridiagonal solve against scipy's not-a-knot CubicSpline on the seven planted inputs: within 1e-10 of the stage's maximum (scipy's two
    cubic routes differ by 3.4e-13 among themselves)"""
    si = pytest.importorskip("scipy.interpolate", reason="scipy is not installed: the spline has nothing to be held to")
    fl, iv, tt = tn.log_axis()
    assert iv.min() >= 0 and iv.max() <= tn.BINS - 2 and (tt >= 0).all() and (tt <= tn.H * (1 + 1e-12)).all()
    worst = 0.0
    for seed, N, d in tn.PLANTED:
        Y = _est(seed, N, d)[1]["Y"]
        ref = si.CubicSpline(np.arange(tn.BINS) * tn.H, Y, bc_type="not-a-knot")(fl)
        got = _est(seed, N, d)[1]["Yi"]
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"spline: restatement against scipy, worst of {len(tn.PLANTED)} inputs: {worst:.3e} of the stage's maximum")
    assert worst <= 1e-10


def test_float32_fft_and_grouping():
    """the float32 route is a float32 FFT (not the fp64 one rounded) and both routes sum over time in the contract's groups"""
    x = _song(21, 32768, 0)
    fr = tn.frames(x)
    P, P32 = tn.power(fr), tn.power(fr.astype(np.float32), np.float32)
    assert P32.dtype == np.float32 and P.shape == P32.shape == (5, tn.BINS)
    rel = float(np.abs(P32 - P).max() / P.max())
    assert 0 < rel < 1e-5, rel
    C = np.arange(19 * 3, dtype=np.float64).reshape(19, 3) * 0.1 + 1e8          # (a sum whose grouping shows in the last bits)
    want = (C[0:8].cumsum(0)[-1] + C[8:16].cumsum(0)[-1]) + C[16:19].cumsum(0)[-1]
    assert np.array_equal(tn.time_sum(C), want)
    assert tn.time_sum(C.astype(np.float32), np.float32).dtype == np.float32


def test_frames_zero_padding_and_group_edges():
    for N, F in ((32768, 5), (40959, 5), (65535, 8), (65536, 9), (131072, 17)):
        assert tn.num_frames(N) == F
        x = np.arange(1, N + 1, dtype=np.float32)
        fr = tn.frames(x, dtype=np.float64)
        w = tn.window().astype(np.float64)
        assert fr.shape == (F, tn.N_FFT)
        assert (fr[0, : tn.HOP] == 0).all() and np.array_equal(fr[0, tn.HOP:], x[: tn.HOP] * w[tn.HOP:])          # the first frame starts 8 192 samples before the song
        last0 = tn.HOP * (F - 2)                                                                                # first sample of the last frame
        inside = N - last0
        assert 0 < inside <= tn.N_FFT
        assert np.array_equal(fr[-1, :inside], x[last0:].astype(np.float64) * w[:inside]) and (fr[-1, inside:] == 0).all()
        groups = [(g, min(F, g + 8)) for g in range(0, F, 8)]
        assert len(groups) == -(-F // 8) and groups[-1][1] == F
    with pytest.raises(ValueError, match="two windows"):
        tn.num_frames(32767)
    with pytest.raises(ValueError, match="two windows"):
        tn.estimate(np.zeros(32767, np.float32))


def test_silence_and_steady_sinusoids():
    t, st = tn.estimate(np.zeros(40000, np.float32))
    assert t == -50 and (st["sim"] == 0).all()          # the first maximum of a constant
    for d in (-50, -20, 0, 13, 49):
        got = tn.estimate(tn.sinusoid(40000, d))[0]
        assert (got - d + 50) % 100 - 50 in (0, 1), (d, got)
    assert tn.estimate(tn.sinusoid(40000, 30, pitch=93))[0] in (30, 31)          # (high up, where a bin of 1.35 Hz is a fraction of a cent)


def test_planted_detuning():
    """the estimate lies within 2 cents of the planted detuning modulo 100 (measured: d + 1 on every fixture, 49 wraps to -50: the third harmonic of the generator
    lies 2 cents above equal temperament)"""
    for seed, N, d in tn.PLANTED:
        got = _est(seed, N, d)[0]
        off = (got - d + 50) % 100 - 50
        print(f"planted {d:+d} cents, N = {N}: estimate {got:+d}")
        assert abs(off) <= 2, (seed, N, d, got)


def _device_inputs():
    """every seeded input the device tests compare as an integer, by name"""
    out = [(f"song seed {s} N {N} {d:+d}", _song(s, N, d)) for s, N, d in tn.DEVICE_INPUTS]
    out += [(f"sinusoid {d:+d}", x) for d, x in zip(tn.SPLIT_CENTS, tn.split_songs())]
    cover, origin = tn.chain_audio()[:2]
    return out + [("chain cover", cover), ("chain origin", origin)]


def test_every_device_input_is_decisive():
    """(sim[best] - sim[second]) / sim[best] of the fp64 restatement exceeds 1e-5 -- a hundred times the deviation of the float32 restatement's sim -- on EVERY input
    whose integer the device tests compare, and the float32 restatement picks the same theta"""
    lo, worst32 = 1.0, 0.0
    for name, x in _device_inputs():
        t, st = tn.estimate(x)
        t32, st32 = tn.estimate(x, np.float32)
        m = tn.margin(st["sim"])
        dev32 = float(np.abs(st32["sim"].astype(np.float64) - st["sim"]).max() / st["sim"].max())
        lo, worst32 = min(lo, m), max(worst32, dev32)
        assert m > 1e-5, (name, m)
        assert t32 == t, (name, t, t32)
    print(f"decisiveness: smallest margin {lo:.3e}; float32 restatement's sim deviates by at most {worst32:.3e} of its maximum")


def test_split_fixture_spans_more_than_one_handle():
    """the 70 sinusoids of the device's bank-split test get more than 64 distinct estimates (the filterbanks of one alignfeat handle)"""
    tun = [tn.estimate(x)[0] for x in tn.split_songs()]
    print(f"split fixture: {len(set(tun))} distinct estimates of {len(tun)}")
    assert len(set(tun)) > 64 and len(set(tun[:64])) == 64


def test_chain_restated_on_the_host():
    """4f's planted warp with both renderings 30 cents flat: restatement estimate -> restatement features at that offset -> dtw_np.  The transposition is found and
    the path lies within CHAIN_MEASURED frames of the planted warp (asserted at twice that, here and in the device chain test)"""
    from etude_amd.alignfeat import pitch_filterbank
    cover, origin, warp, transpose = tn.chain_audio()
    assert min(len(cover), len(origin)) >= tn.MIN_N
    tc, to = tn.estimate(cover)[0], tn.estimate(origin)[0]
    assert abs(tc - tn.CHAIN_CENTS) <= 2 and abs(to - tn.CHAIN_CENTS) <= 2, (tc, to)
    fc, fo = an.features(cover, pitch_filterbank(float(tc))), an.features(origin, pitch_filterbank(float(to)))
    r = dn.align(tuple(f.astype(np.float32) for f in fc), tuple(f.astype(np.float32) for f in fo))
    dev = an.path_deviation(r["wp"], warp)
    print(f"chain on the host: tuning {tc:+d} / {to:+d}, pitch_shift = {r['pitch_shift']}, deviation = {dev:.3f} frames")
    assert r["pitch_shift"] == an.PLANTED_PITCH_SHIFT == -transpose
    assert dev <= tn.CHAIN_BOUND


# ------------------------------------------------------------------ the C ABI's host side (needs no GPU)
def test_host_entry_points_and_refusals():
    from etude_amd import _lib
    from etude_amd import tuning as tu
    lib = _lib.lib()
    assert lib.etd_version() == 3
    lim = tu.limits()
    assert lim == dict(min_samples=32768, max_samples=1 << 27, max_songs=4096)
    est = tu.TuningEstimator()
    assert [est.num_frames(n) for n in (32768, 40959, 65535, 65536)] == [5, 5, 8, 9]
    one, two = est.workspace_bytes([65536]), est.workspace_bytes([65536, 32768])
    assert 0 < one < two
    lay = est.layout([32768, 131072], 1)
    assert (lay["F"], lay["G"]) == (17, 3) and lay["off_Y"] - lay["off_part"] >= 3 * 8193 * 4 and all(lay[k] % 256 == 0 for k in lay if k.startswith("off_"))
    assert lay["off_sim"] + 800 <= est.workspace_bytes([32768, 131072])
    with pytest.raises(ValueError, match="two windows"):
        est.num_frames(32767)
    with pytest.raises(_lib.EtudeHipError, match="N = 32767"):
        est.workspace_bytes([32768, 32767])
    with pytest.raises(_lib.EtudeHipError, match="songs in one call"):
        est.workspace_bytes([32768] * 4097)
    with pytest.raises(_lib.EtudeHipError, match="fixed to"):
        h = C.c_void_p()
        _lib.check(lib.etd_tuning_create(C.byref(_lib.TuningCfg(sample_rate=44100, n_fft=16384, hop=8192)), C.byref(h)), "etd_tuning_create")
    with pytest.raises(ValueError, match="22050"):
        tu.estimate_tuning(np.zeros(40000, np.float32), 44100)
    import etude_amd
    assert etude_amd.TuningEstimator is tu.TuningEstimator and etude_amd.estimate_tuning is tu.estimate_tuning
