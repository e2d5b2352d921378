"""Alignment features on the host: the numpy filter design against scipy's, the exact chunk decomposition the device is given tables for, the restatement
(tests/alignfeat_np.py) on hand-made cases, the planted-warp fixture through dtw_np, and the C ABI's host-only entry points."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.signal as sg

sys.path.insert(0, str(Path(__file__).resolve().parent))
import alignfeat_np as an  # noqa: E402
import dtw_np as dn  # noqa: E402

from etude_amd import alignfeat as af  # noqa: E402

L = 256
_cache = {}


def _bank(t=0.0):
    if t not in _cache:
        _cache[t] = af.pitch_filterbank(t, L)
    return _cache[t]


def _sorted(a):
    return np.array(sorted(a, key=lambda c: (round(c.real, 9), round(c.imag, 9))))


# ------------------------------------------------------------------ filter design
@pytest.mark.parametrize("tuning", [0.0, -50.0, 37.5])
def test_design_equals_scipy(tuning):
    """Same order; poles, zeros and gain equal after sorting.  Largest deviation observed over the 3 x 88 bands (|z|, |p| about 1, the gain relative): 2.9e-15; asserted
    at ten times that."""
    worst = 0.0
    for p in af.PITCHES:
        fs = af.TIER_FS[af.tier_of_pitch(p)]
        fc = 440.0 * 2.0 ** ((p - 69 + tuning / 100.0) / 12.0)
        wp = [fc * (1 - 1 / 50) / (fs / 2), fc * (1 + 1 / 50) / (fs / 2)]
        ws = [fc * (1 - 2 / 50) / (fs / 2), fc * (1 + 2 / 50) / (fs / 2)]
        n, wn = sg.ellipord(wp, ws, 1, 50)
        z, pl, k = sg.ellip(n, 1, 50, wn, btype="bandpass", output="zpk")
        n2, z2, p2, k2 = af.ellip_bandpass_zpk(fc, fs)
        assert n2 == n and n in (4, 5)
        assert len(z2) == len(z) and len(p2) == len(pl)
        worst = max(worst, float(np.abs(_sorted(z) - _sorted(z2)).max()), float(np.abs(_sorted(pl) - _sorted(p2)).max()), abs(k - k2) / abs(k))
        assert np.abs(p2).max() < 1.0
        # the sections hold exactly these poles and zeros
        sos = af.ellip_bandpass_sos(fc, fs)
        assert sos.shape == (n, 6) and (sos[:, 3] == 1.0).all()
        zs, ps, ks = sg.sos2zpk(sos)
        assert np.abs(_sorted(zs) - _sorted(z2)).max() < 1e-9 and np.abs(_sorted(ps) - _sorted(p2)).max() < 1e-9 and abs(ks - k2) <= 1e-12 * abs(k2)
        assert np.abs(ps).max() < 1.0
    print(f"design, tuning {tuning}: largest deviation from scipy {worst:.3e}")
    assert worst <= 2.9e-14


def test_bank_tables():
    bank = _bank()
    assert bank["sos"].shape == (88, 6, 6) and bank["apow"].shape == (88, 12, 12) and set(bank["n_sections"]) == {4, 5}
    for b in (0, 87):
        ns = int(bank["n_sections"][b])
        assert (bank["sos"][b, ns:] == 0).all() and (bank["apow"][b, 2 * ns:] == 0).all() and (bank["apow"][b, :, 2 * ns:] == 0).all()
    assert np.array_equal(af.decimation_fir(), an.fir()) and abs(float(an.fir().astype(np.float64).sum()) - 1.0) < 1e-6
    with pytest.raises(ValueError, match="50 cents"):
        af.pitch_filterbank(50.5)


# ------------------------------------------------------------------ the exact decomposition
@pytest.mark.parametrize("b", [0, 38, 39, 74, 75, 87])          # pitches 21, 59, 60, 95, 108 and 96
def test_chunked_scheme_is_the_sequential_filter(b):
    """every chunk from zero, s_{c+1} = A^L s_c + e_c, every chunk again from its true state: against one straight sosfilt, relative to the output's maximum.  Largest
    deviation observed over these bands (N = 3 L + 17 and the reversed second pass): 2.2e-13; asserted at ten times that."""
    bank = _bank()
    sos, apow = an.bank_sos(bank, b), bank["apow"][b]
    rng = np.random.default_rng(b)
    for N in (3 * L + 17, 7 * L + 1, L - 156):
        x = rng.standard_normal(N)
        ref = sg.sosfilt(sos, x)
        got = an.chunked_sosfilt(sos, apow, x, L)
        dev = float(np.abs(got - ref).max() / np.abs(ref).max())
        ref2 = sg.sosfilt(sos, ref[::-1])[::-1]
        got2 = an.chunked_sosfilt(sos, apow, got[::-1], L)[::-1]
        dev2 = float(np.abs(got2 - ref2).max() / np.abs(ref2).max())
        print(f"chunked scheme, pitch {21 + b}, N = {N}: {dev:.3e} forward, {dev2:.3e} after the backward pass")
        assert dev <= 2.2e-12 and dev2 <= 2.2e-12
        if N < L:
            assert np.array_equal(got, ref)


# ------------------------------------------------------------------ hand-made cases of the restatement
@pytest.mark.parametrize("N", [1, 440, 441, 442, 2205])
def test_frames_and_windows(N):
    T = an.num_frames(N)
    assert T == (N + 440) // 441 and T == {1: 1, 440: 1, 441: 1, 442: 2, 2205: 5}[N]
    for tier, d in enumerate(an.TIER_D):
        n_t = N
        for _ in range(tier):
            n_t = -(-n_t // 5)
        for t in range(T):
            lo, hi = an.energy_bounds(t, d, n_t)
            ks = [k for k in range(n_t) if 441 * (t - 1) <= k * d <= 441 * (t + 1)]          # the samples within one frame of frame t's instant
            assert (lo, hi) == ((ks[0], ks[-1]) if ks else (lo, lo - 1)) or (not ks and hi < lo)
        w, hop = an.TIER_W[tier], an.TIER_W[tier] // 2
        for m in range(-(-n_t // hop)):
            time = (m * hop + w / 2) / (an.FS / d)
            assert an.frame_of(m, tier, T) == min(T - 1, int(np.floor(50 * time + 0.5 + 1e-9)))
    ch, dl = an.features(an.seeded_signal(5, N), _bank())
    assert ch.shape == dl.shape == (12, T) and np.isfinite(dl).all()


def test_impulse():
    x = np.zeros(4000, np.float32)
    x[2000] = 1.0
    ch, dl, d = an.features(x, _bank(), details=True)
    x1 = d["tiers"][1]
    assert int(np.argmax(np.abs(x1))) == 400 and abs(float(x1[400]) - float(an.fir()[240])) < 1e-9          # the centre tap lands on 5 m = 2000
    for b in (75, 87):
        y = d["y"][b]
        assert int(np.argmax(np.abs(y))) in range(1990, 2011)          # zero phase: the response is centred on the impulse
        assert np.abs(y[1000:3001] - y[1000:3001][::-1]).max() < 2e-2 * np.abs(y).max()          # (symmetric up to the ringing the signal's ends cut off)
    assert np.isfinite(dl).all() and dl.max() > 0


def test_silence():
    ch, dl = an.features(np.zeros(3 * an.FS, np.float32), _bank())
    assert (an.chroma_normalized(np.zeros((88, 5))) == 1 / 12).all()
    assert (ch == 0.25).all() and (dl == 0).all()          # 1/12 lies above the first threshold alone: one quarter in every row


def test_steady_sinusoid():
    t = np.arange(3 * an.FS) / an.FS
    ch, dl = an.features((0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32), _bank())
    assert (ch[9, 10:-10] == 1.0).all() and (np.delete(ch, 9, axis=0)[:, 10:-10] == 0).all()


def test_two_planted_onsets():
    N = 3 * an.FS
    x = an.render_roll([(69, 0.5, 0.3), (76, 1.5, 0.3)], N)
    ch, dl, d = an.features(x, _bank(), details=True)
    T = an.num_frames(N)
    for b, frame in ((69 - 21, 25), (76 - 21, 75)):
        rows = [r for r in d["peaks"] if r[0] == b]
        top = max(rows, key=lambda r: r[3])
        assert abs(top[2] - frame) <= 1, (top, frame)
    # the DLNCO tail of an isolated peak: sqrt(1 / (i + 1)) while the local normalisation G is constant
    one = an.dlnco([(48, 100, 30, np.float32(0.5))], T)
    assert np.allclose(one[9, 30:40] / one[9, 30], np.sqrt(1.0 / np.arange(1, 11)), rtol=1e-12) and (one[9, 40:] == 0).all() and (one[9, :30] == 0).all()
    q = (69 % 12)
    t0 = int(np.argmax(dl[q, :40]))
    assert abs(t0 - 25) <= 1 and dl[q, t0 + 1] < dl[q, t0]


def test_chroma_exclusion_stays_below_one_percent():
    """EVERY seeded input whose stages tests/test_gpu_alignfeat.py checks, with its tuning: at most 1 % of the chroma entries lie within 1e-6 of a quantisation
    threshold (observed: none), and no column's sum lies at the 1e-3 switch to 1/12, where a float32 and a float64 sum could choose differently"""
    worst = 0.0
    for seed, N, tuning in an.stage_inputs(L):
        _, _, d = an.features(an.seeded_signal(seed, N), _bank(tuning), details=True)
        worst = max(worst, float(an.near_threshold(d["E"]).mean()))
        assert an.near_threshold(d["E"]).mean() <= 0.01, (seed, N)
        assert not an.near_silence_switch(d["E"]).any(), (seed, N)
    print(f"chroma entries within 1e-6 of a threshold, worst input: {worst:.4%}")


def test_planted_warp_through_dtw():
    """restatement features -> dtw_np: the transposition is found and the path lies within 2.171 origin frames of the planted warp (asserted at twice that)"""
    cover, origin, warp, transpose = an.planted_warp_audio()
    assert max(len(cover), len(origin)) < 20 * an.FS
    fc, fo = an.features(cover, _bank()), an.features(origin, _bank())
    r = dn.align(tuple(f.astype(np.float32) for f in fc), tuple(f.astype(np.float32) for f in fo))
    dev = an.path_deviation(r["wp"], warp)
    print(f"planted warp: pitch_shift = {r['pitch_shift']}, deviation = {dev:.3f} frames")
    assert r["pitch_shift"] == an.PLANTED_PITCH_SHIFT == -transpose
    assert dev <= an.PLANTED_WARP_BOUND


# ------------------------------------------------------------------ the C ABI's host side (needs no GPU)
def test_host_entry_points_and_refusals():
    from etude_amd import _lib
    lib = _lib.lib()
    lim = af.limits()
    assert lim["chunk"] == L and lim["max_sections"] == 6 and lim["max_songs"] == 4096
    feats = af.AlignFeatures()
    assert [feats.num_frames(n) for n in (1, 441, 442)] == [1, 1, 2]
    one, two = feats.workspace_bytes([22050]), feats.workspace_bytes([22050, 22050])
    assert 0 < one < two < 2 * one + 4096
    lay = feats.layout([1000, 22050], 1)
    assert lay["T"] == 50 and (lay["n0"], lay["n1"], lay["n2"]) == (22050, 4410, 882) and (lay["nc0"], lay["nm0"], lay["nm2"]) == (87, 441, 36)
    assert lay["out_off"] == 12 * 3 and lay["off_x1"] % 256 == 0
    with pytest.raises(ValueError):
        feats.num_frames(0)
    with pytest.raises(_lib.EtudeHipError, match="N = 0"):
        feats.workspace_bytes([0])
    with pytest.raises(_lib.EtudeHipError, match="songs in one call"):
        feats.workspace_bytes([10] * 4097)
    bank, fir = _bank(), af.decimation_fir()

    def create(sos, nsec, apow, **kw):
        args = dict(sample_rate=22050, hop=441, fir_taps=481, decimation=5, chunk=L, n_banks=1)
        args.update(kw)
        cfg = _lib.AlignFeatCfg(**args)
        h = C.c_void_p()
        sos, nsec, apow = np.ascontiguousarray(sos), np.ascontiguousarray(nsec, np.int32), np.ascontiguousarray(apow)
        _lib.check(lib.etd_alignfeat_create(C.byref(cfg), fir.ctypes.data, sos.ctypes.data, nsec.ctypes.data, apow.ctypes.data, C.byref(h)), "create")
        lib.etd_alignfeat_destroy(h)
    create(bank["sos"], bank["n_sections"], bank["apow"])
    seven = bank["n_sections"].copy(); seven[5] = 7
    with pytest.raises(_lib.EtudeHipError, match="more than 6"):
        create(bank["sos"], seven, bank["apow"])
    bad = bank["sos"].copy(); bad[3, 1, 2] = np.nan
    with pytest.raises(_lib.EtudeHipError, match="non-finite"):
        create(bad, bank["n_sections"], bank["apow"])
    bad = bank["sos"].copy(); bad[3, 1, 5] = 1.0
    with pytest.raises(_lib.EtudeHipError, match="unstable"):
        create(bad, bank["n_sections"], bank["apow"])
    with pytest.raises(_lib.EtudeHipError, match="chunk"):
        create(bank["sos"], bank["n_sections"], bank["apow"], chunk=128)
    assert lib.etd_version() == 3
