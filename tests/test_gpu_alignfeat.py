"""Alignment features on the MI355X (csrc/alignfeat.hip, etude_amd.AlignFeatures) against the fp64 restatement of DESIGN.md 4f (tests/alignfeat_np.py), every stage on
the device's OWN tapped input, at every edge of the work map; batch invariance, canaries, refusals, and the chain from audio to a warping path.

Continuous stages (decimation, filterbank, pitch energy, novelty, DLNCO): E = max |device - fp64 restatement| must satisfy E <= 4 * E32 + eps, E32 being the same
maximum for the restatement run in float32 on the same input in the same test; eps is 4 float32 ulps of the stage's peak (the device stores each of these stages as
float32) and 1e-6 for the DLNCO.  The device recurrence is fp64, so E sits well below E32 wherever E32 is not zero; both are printed.
Discrete stages (chroma quantisation, peaks) must agree exactly; chroma entries within 1e-6 of a threshold are excluded, at most 1 % of them."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import alignfeat_np as an  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
TAP_BANDS = (0, 38, 39, 74, 75, 87)          # pitches 21, 59, 60, 95, 96, 108
PAD = 4096
_cache = {}


def _af(budget=None):
    from etude_amd.alignfeat import AlignFeatures
    if ("af", budget) not in _cache:
        _cache[("af", budget)] = AlignFeatures() if budget is None else AlignFeatures(workspace_budget=budget)
    return _cache[("af", budget)]


def _bank(t=0.0):
    from etude_amd.alignfeat import pitch_filterbank
    if ("bank", t) not in _cache:
        _cache[("bank", t)] = pitch_filterbank(t, _af().chunk)
    return _cache[("bank", t)]


def _signal(seed, N):
    if ("x", seed, N) not in _cache:
        x = an.seeded_signal(seed, N)
        x.setflags(write=False)
        _cache[("x", seed, N)] = x
    return _cache[("x", seed, N)]


def _boff(b, v):
    return b * v[2] if b < 39 else 39 * v[2] + ((b - 39) * v[1] if b < 75 else 36 * v[1] + (b - 75) * v[0])


def _run_tapped(xs, tunings=None):
    """one call with buffers of the test's own, canaries around the outputs and the workspace -> per song (chroma, dlnco, taps)"""
    af = _af()
    tunings = [0.0] * len(xs) if tunings is None else tunings
    songs = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    Ns = [len(x) for x in xs]
    Ts = [af.num_frames(n) for n in Ns]
    nb, nf = af.workspace_bytes(Ns), 12 * sum(Ts)
    ws = torch.full((nb + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((nf + 128,), 12345.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    af.run_raw(songs, tunings, outs[0][64: 64 + nf], outs[1][64: 64 + nf], ws[PAD: PAD + nb])
    torch.cuda.synchronize()
    assert bool((ws[:PAD] == 0xA5).all()) and bool((ws[PAD + nb:] == 0xA5).all()), "the workspace canaries were overwritten"
    for o in outs:
        assert bool((o[:64] == 12345.0).all()) and bool((o[64 + nf:] == 12345.0).all()), "an output canary was overwritten"
    host = ws[PAD: PAD + nb].cpu().numpy()
    ch, dl = outs[0][64: 64 + nf].cpu().numpy(), outs[1][64: 64 + nf].cpu().numpy()
    res = []
    for s in range(len(xs)):
        lay = af.layout(Ns, s)
        T, n, nm = lay["T"], [lay["n0"], lay["n1"], lay["n2"]], [lay["nm0"], lay["nm1"], lay["nm2"]]

        def arr(off, count, dtype):
            return host[off: off + count * np.dtype(dtype).itemsize].view(dtype)

        def band(off, b, v, dtype):
            t = an.tier_of_pitch(21 + b)
            return arr(off + _boff(b, v) * np.dtype(dtype).itemsize, v[t], dtype)
        taps = dict(T=T, n=n, nm=nm, x=[np.array(xs[s]), arr(lay["off_x1"], n[1], np.float32), arr(lay["off_x2"], n[2], np.float32)],
                    y={b: band(lay["off_y"], b, n, np.float32) for b in range(88)}, E=arr(lay["off_E"], 88 * T, np.float32).reshape(88, T),
                    nov={b: band(lay["off_nov"], b, nm, np.float32) for b in range(88)}, ph={b: band(lay["off_ph"], b, nm, np.float32) for b in range(88)},
                    pf={b: band(lay["off_pf"], b, nm, np.int32) for b in range(88)})
        o = lay["out_off"]
        res.append((ch[o: o + 12 * T].reshape(12, T), dl[o: o + 12 * T].reshape(12, T), taps))
    return res


def _bound(name, got, ref, r32, eps):
    E, E32 = float(np.abs(got - ref).max(initial=0.0)), float(np.abs(r32 - ref).max(initial=0.0))
    print(f"alignfeat {name}: E = {E:.3e}, E32 = {E32:.3e}, bound = {4 * E32 + eps:.3e}")
    assert np.isfinite(got).all()
    assert E <= 4 * E32 + eps, (name, E, E32, eps)


def _check_stages(x, tuning=0.0):
    chroma, dl, tp = _run_tapped([x], [tuning])[0]
    bank, T = _bank(tuning), tp["T"]
    assert T == an.num_frames(len(x)) and chroma.shape == dl.shape == (12, T)
    # tiers, each on the device's own previous tier
    for k in (1, 2):
        ref, r32 = an.decimate(tp["x"][k - 1]), an.decimate(tp["x"][k - 1], np.float32)
        assert len(ref) == tp["n"][k]
        _bound(f"N={len(x)} tier {k}", tp["x"][k], ref, r32, 4 * ULP * float(np.abs(ref).max()))
    # filterbank on the device's own tier signal
    for b in TAP_BANDS:
        xt = tp["x"][an.tier_of_pitch(21 + b)]
        ref, r32 = an.band_filter(xt, an.bank_sos(bank, b)), an.band_filter(xt, an.bank_sos(bank, b), np.float32)
        _bound(f"N={len(x)} y pitch {21 + b}", tp["y"][b], ref, r32, 4 * ULP * float(np.abs(ref).max()))
    # energy and novelty on the device's own y
    ref, r32 = an.pitch_energy(tp["y"], T), an.pitch_energy(tp["y"], T, np.float32)
    _bound(f"N={len(x)} E", tp["E"], ref, r32, 4 * ULP * float(ref.max()))
    for b in TAP_BANDS:
        ref, r32 = an.novelty_band(tp["y"][b], b), an.novelty_band(tp["y"][b], b, np.float32)
        w = an.TIER_W[an.tier_of_pitch(21 + b)]
        peak_e = 0.5 * w * float((tp["y"][b].astype(np.float64) ** 2).max())          # (no local energy is above this: the Hann window sums to w / 2)
        _bound(f"N={len(x)} novelty pitch {21 + b}", tp["nov"][b], ref, r32, 4 * ULP * peak_e)
    # chroma: exact on the device's own E, away from the thresholds
    skip = an.near_threshold(tp["E"])
    assert skip.mean() <= 0.01, skip.mean()
    assert not an.near_silence_switch(tp["E"]).any()          # (no column sits on the 1e-3 switch, where the float32 and the float64 sum could differ: nothing more is excluded)
    want = an.chroma_quantized(tp["E"])
    assert np.array_equal(chroma[~skip], want[~skip].astype(np.float32))
    assert chroma.min() >= 0.0 and np.isfinite(dl).all()
    # peaks: exact on the device's own novelty
    want_rows = an.peaks(tp["nov"], T)
    got_rows = [(b, int(m), int(tp["pf"][b][m]), tp["ph"][b][m]) for b in range(88) for m in np.flatnonzero(tp["ph"][b] > 0)]
    assert got_rows == want_rows
    for b in range(88):
        tier = an.tier_of_pitch(21 + b)
        assert np.array_equal(tp["pf"][b], [an.frame_of(m, tier, T) for m in range(tp["nm"][tier])])
    # DLNCO on the device's own peak list
    ref, r32 = an.dlnco(got_rows, T), an.dlnco(got_rows, T, np.float32)
    _bound(f"N={len(x)} DLNCO", dl, ref, r32, 1e-6)
    return chroma, dl


@pytest.mark.parametrize("N", an.stage_shapes(256))
def test_stages_at_every_edge(N):
    assert _af().chunk == 256          # (the shapes are built around it)
    _check_stages(_signal(an.STAGE_SEED, N))


def test_stages_longer_song_with_tuning():
    for seed, N, tuning in an.STAGE_LONG:
        _check_stages(_signal(seed, N), tuning)


def test_silence_and_sinusoid():
    af = _af()
    ch, dl = af.features(torch.zeros(3 * an.FS, device="cuda"))
    assert bool((ch == 0.25).all()) and bool((dl == 0).all())          # (1/12 in every row lies above the first threshold alone)
    t = np.arange(3 * an.FS) / an.FS
    ch, dl = af.features((0.3 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32))
    ch = ch.cpu().numpy()
    assert (ch[9, 10:-10] == 1.0).all() and (np.delete(ch, 9, axis=0)[:, 10:-10] == 0).all()


def test_invariance_bitwise():
    af = _af()
    xs = [_signal(1, 3 * 256 + 17), _signal(2, an.FS + 77), _signal(3, 25 * 256 + 1)]
    tun = [0.0, 37.5, -50.0]
    alone = [af.features(x, t) for x, t in zip(xs, tun)]
    batch = af.features_many(xs, tun)
    rev = af.features_many(xs[::-1], tun[::-1])[::-1]
    small = _af(budget=max(af.workspace_bytes([len(x)]) for x in xs))          # every song its own sub-batch
    assert [len(g) for g in small._batches([len(x) for x in xs])] == [1, 1, 1]
    sub = small.features_many(xs, tun)
    for a, b, r, s in zip(alone, batch, rev, sub):
        for k in range(2):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], r[k]) and torch.equal(a[k], s[k])
    tapped = _run_tapped(xs, tun)          # (canaries around a ragged batch)
    for a, t in zip(alone, tapped):
        assert np.array_equal(a[0].cpu().numpy(), t[0]) and np.array_equal(a[1].cpu().numpy(), t[1])


def test_refusals():
    from etude_amd import _lib
    from etude_amd.alignfeat import decimation_fir
    af = _af()
    lib = _lib.lib()
    with pytest.raises(ValueError, match="N >= 1"):
        af.features_many([torch.zeros(0, device="cuda")])
    with pytest.raises(ValueError, match="mono"):
        af.features_many([torch.zeros(2, 100, device="cuda")])
    with pytest.raises(ValueError, match="50 cents"):
        af.features_many([torch.zeros(100, device="cuda")], [51.0])
    with pytest.raises(ValueError, match="finite"):
        af.features_many([torch.full((100,), float("nan"), device="cuda")])
    with pytest.raises(_lib.EtudeHipError, match="N = 0"):
        af.workspace_bytes([100, 0])
    with pytest.raises(_lib.EtudeHipError, match="songs in one call"):
        af.workspace_bytes([10] * (af.limits["max_songs"] + 1))
    x = torch.zeros(1000, device="cuda")
    T = af.num_frames(1000)
    out = torch.zeros(2, 12 * T, device="cuda")
    with pytest.raises(_lib.EtudeHipError, match="workspace holds"):
        af.run_raw([x], [0.0], out[0], out[1], torch.zeros(af.workspace_bytes([1000]) - 256, dtype=torch.uint8, device="cuda"))
    # the section tables
    bank, fir = _bank(), decimation_fir()

    def create(sos, nsec, apow):
        cfg = _lib.AlignFeatCfg(sample_rate=22050, hop=441, fir_taps=481, decimation=5, chunk=af.chunk, n_banks=1)
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
    bad = bank["apow"].copy(); bad[0, 0, 0] = np.inf
    with pytest.raises(_lib.EtudeHipError, match="non-finite"):
        create(bank["sos"], bank["n_sections"], bad)
    # after the refusals the engine still answers
    a, b = af.features(_signal(1, 3 * 256 + 17)), af.features(_signal(1, 3 * 256 + 17))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_chain_from_audio(tmp_path):
    from etude_amd.aligner import AudioAligner, align_audio_many
    cover, origin, warp, _ = an.planted_warp_audio()
    r = align_audio_many([(cover, origin)])[0]
    dev = an.path_deviation(r["wp"], warp)
    print(f"alignfeat chain: pitch_shift = {r['pitch_shift']}, path within {dev:.2f} frames of the planted warp (bound {an.PLANTED_WARP_BOUND})")
    assert r["pitch_shift"] == an.PLANTED_PITCH_SHIFT
    assert r["num_frames_cover"] == an.num_frames(len(cover)) and r["num_frames_origin"] == an.num_frames(len(origin))
    assert dev <= an.PLANTED_WARP_BOUND
    # ... and through AudioAligner with the features as its feature_fn: two "files" -> wp.json
    wavs = {"origin.wav": origin, "cover.wav": cover}
    for name in wavs:
        (tmp_path / name).write_bytes(b"")
    al = AudioAligner(feature_fn=_af().as_feature_fn(lambda p: wavs[Path(p).name]))
    got = al.align(tmp_path / "origin.wav", tmp_path / "cover.wav", tmp_path)
    assert got is not None and np.array_equal(got["wp"], r["wp"]) and got["pitch_shift"] == r["pitch_shift"]
    assert (tmp_path / "wp.json").exists() and np.array_equal(al.align(tmp_path / "origin.wav", tmp_path / "cover.wav", tmp_path)["wp"], r["wp"])
