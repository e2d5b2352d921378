"""Separator dropout, the segment sampler and the loop without a GPU: the restatement (tests/separator_data_np.py) against Random123's known answers, the binomial
law, scipy's linear interpolation and finite differences; the mistakes it must be able to see; and what ``SeparatorTrainer`` / ``SegmentSampler`` refuse, draw and
save before any device is touched."""
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_data_np as sd  # noqa: E402
import separator_train_np as st  # noqa: E402

from etude_amd import _lib  # noqa: E402
from etude_amd import separator_data as data  # noqa: E402
from etude_amd.separator import SeparatorConfig, init_separator_state  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer  # noqa: E402

F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
ROOT = Path(__file__).resolve().parent.parent
SEED, P = 0x1234567890ABCDEF, 0.5
_cache = {}


def _tiny(B=2, filters=(2, 2, 3, 2, 2, 2), instruments=("a", "b"), C=1):
    key = (B, filters, instruments, C)
    if key not in _cache:
        cfg = SeparatorConfig(instruments=instruments, n_fft=1024, hop=256, T=64, F=64, n_channels=C, conv_n_filters=filters)
        state = init_separator_state(cfg, 11)
        for k in state:
            if k.endswith(".bias"):
                state[k] = np.random.default_rng(len(k)).normal(0, 0.1, state[k].shape).astype(np.float32)
        g = torch.Generator().manual_seed(5)
        mix = torch.rand(B, 64, 64, C, generator=g) * 2.0
        target = torch.rand(len(instruments), B, 64, 64, C, generator=g) * mix[None]
        _cache[key] = (cfg, state, mix, target)
    return _cache[key]


def _truth():
    if "truth" not in _cache:
        cfg, state, mix, target = _tiny()
        _cache["truth"] = (sd.loss_and_grads(mix, target, state, cfg, F64, P, SEED, 3), sd.loss_and_grads(mix, target, state, cfg, F32, P, SEED, 3))
    return _cache["truth"]


def _err(g, g64):
    return float((g.to(F64) - g64).abs().max()) / float(g64.abs().max())


# ------------------------------------------------------------------ the generator and the mask
def test_philox_known_answers():
    """the three known-answer vectors of Random123's kat_vectors for philox4x32-10"""
    hexs = lambda ws: " ".join(f"{int(w):08x}" for w in ws)      # noqa: E731
    assert hexs(sd.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(sd.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(sd.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    many = sd.philox4x32_10((np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]), np.array([0, 0x03707344])), (0, 0))
    assert int(many[0][0]) == 0x6627E8D5                # vectorised over the counter


@pytest.mark.parametrize("p", [0.5, 0.1, 0.9])
def test_kept_share_is_within_five_binomial_sigmas(p):
    n = 2 ** 16
    keep = sd.dropout_keep(n, 2, 7, SEED, p)
    share, sigma = keep.mean(), math.sqrt(p * (1 - p) / n)
    print(f"p = {p}: kept {share:.5f}, expected {1 - p}, sigma {sigma:.2e}")
    assert abs(share - (1 - p)) <= 5 * sigma
    assert not np.array_equal(keep, sd.dropout_keep(n, 2, 8, SEED, p)) and not np.array_equal(keep, sd.dropout_keep(n, 3, 7, SEED, p))
    assert np.array_equal(keep[:1001], sd.dropout_keep(1001, 2, 7, SEED, p))      # a count that ends inside a block
    assert sd.drop_threshold(0.0) == 2 ** 32 - 1 and sd.drop_threshold(0.5) == 2 ** 31 and float(sd.drop_scale(0.5)) == 2.0


# ------------------------------------------------------------------ the gather
def _track(K=3, frames=128, F=64, C=2, seed=1):
    return np.random.default_rng(seed).random((K, frames, F, C)).astype(np.float32) * 3.0


def test_identity_draw_is_a_copy():
    S = _track()
    for dt in (np.float32, np.float64):
        got = sd.gather(S, 100, 64, 17, 1.0, 1.0, dt)
        assert got.dtype == dt and np.array_equal(got, S[:, 17:81].astype(dt))
    got = sd.gather(S, 100, 64, 60, 1.0, 1.0, np.float32)      # the window runs past Tf = 100 into zeros
    assert np.array_equal(got[:, :40], S[:, 60:100]) and not got[:, 40:].any()


@pytest.mark.parametrize("a", [0.9, 1.0, 1.1])
@pytest.mark.parametrize("q", [2.0 ** (-1 / 12), 1.0, 2.0 ** (1 / 12)])
def test_gather_equals_scipy_linear_interpolation_on_the_cropped_and_padded_geometry(a, q):
    """fp64, bound 1e-12 of the tensor's largest value: two nested lerps against scipy's four-point bilinear sum differ by a few ulp of fp64"""
    T = F = 64
    S, Tf, t0 = _track().astype(np.float64), 100, 50      # 14 frames of the window lie past Tf
    got = sd.gather(S, Tf, T, t0, a, q, np.float64)
    W = sd.window(S, Tf, T, t0, np.float64)
    Tp, Fp = sd.stretched_sizes(T, F, a, q)
    r = np.arange(T) + (Tp - T) // 2 if Tp >= T else np.arange(T) - (T - Tp) // 2
    tin, fin = (r >= 0) & (r < Tp), np.arange(F) < min(F, Fp)
    pt, pf = r * (T - 1) / (Tp - 1), np.arange(F) * (F - 1) / (Fp - 1)
    coords = np.stack(np.meshgrid(np.clip(pt, 0, T - 1), np.clip(pf, 0, F - 1), indexing="ij"))
    want = np.zeros_like(got)
    for k in range(S.shape[0]):
        for c in range(S.shape[3]):
            want[k, :, :, c] = ndimage.map_coordinates(W[k, :, :, c], coords, order=1, mode="nearest") * (tin[:, None] & fin[None, :])
    rel = float(np.abs(got - want).max()) / float(np.abs(want).max())
    print(f"a = {a} q = {q:.4f}: T' = {Tp} F' = {Fp}, vs scipy {rel:.2e}")
    assert rel <= 1e-12
    if a < 1:
        assert not got[:, :(T - Tp) // 2].any() and not got[:, (T - Tp) // 2 + Tp:].any() and got[:, (T - Tp) // 2].any()
    if q < 1:
        assert not got[:, :, Fp:].any() and got[:, :, Fp - 1].any()
    g32 = sd.gather(S.astype(np.float32), Tf, T, t0, a, q, np.float32)
    assert g32.dtype == np.float32 and float(np.abs(g32 - got).max()) / float(np.abs(got).max()) <= 8 * 2.0 ** -24      # three roundings of at most half an ulp each, on values <= max


def test_a_units_output_does_not_depend_on_its_batch():
    S0, S1 = _track(seed=1), _track(seed=2)
    tracks = [(S0, 100), (S1, 128)]
    d = [(0, 3, 0.93, 1.04), (1, 60, 1.07, 0.97), (0, 99, 1.0, 1.0)]
    mix, target = sd.batch(tracks, d, 64, np.float32)
    assert mix.shape == (3, 64, 64, 2) and target.shape == (2, 3, 64, 64, 2)
    for u in range(3):
        m1, t1 = sd.batch(tracks, [d[u]], 64, np.float32)
        assert np.array_equal(m1[0], mix[u]) and np.array_equal(t1[:, 0], target[:, u])


# ------------------------------------------------------------------ dropout's gradient
def test_fp64_gradients_with_dropout_agree_with_central_finite_differences():
    """4n's settings: h = 1e-6 on the fp64 loss, bound 1e-6 of the tensor's largest gradient entry (the mask is a constant of the call, so the loss is as smooth as
    without it and 4n's reasoning holds).  Measured: at most 4.7e-8 (a.deconv2.bias)."""
    cfg, state, mix, target = _tiny()
    (L, g64, _), _ = _truth()
    h, worst = 1e-6, 0.0
    for k in ("a.conv1.weight", "b.conv4.weight", "a.deconv1.weight", "b.deconv2.weight", "a.deconv3.weight", "b.deconv4.weight", "a.bn7.gamma", "b.bn8.beta",
              "a.bn9.gamma", "b.bn10.beta", "a.deconv2.bias", "b.head.weight"):
        idx = int(g64[k].abs().argmax())
        vals = []
        for sgn in (1.0, -1.0):
            Pm = st.params(state, F64, requires_grad=False)
            Pm[k].view(-1)[idx] += sgn * h
            vals.append(float(st.loss_fn(sd.forward(mix.to(F64), Pm, cfg, P, SEED, 3), mix.to(F64), target.to(F64))))
        fd, an = (vals[0] - vals[1]) / (2 * h), float(g64[k].view(-1)[idx])
        rel = abs(fd - an) / float(g64[k].abs().max())
        print(f"FD {k}[{idx}]: autograd {an:.9e} differences {fd:.9e} rel {rel:.2e}")
        worst = max(worst, rel)
        assert rel <= 1e-6, (k, fd, an)
    print(f"FD worst {worst:.2e}")


@pytest.mark.parametrize("variant", ["no_backward_mask", "mask_before_norm"])
def test_each_wrong_variant_moves_a_result_far_past_the_bound(variant):
    cfg, state, mix, target = _tiny()
    (_, g64, _), (_, g32, _) = _truth()
    _, gv, _ = sd.loss_and_grads(mix, target, state, cfg, F64, P, SEED, 3, variant=variant)
    live = [k for k in g64 if float(g64[k].abs().max()) > 0]
    worst_v = max(_err(gv[k], g64[k]) for k in live)
    bound = max(max(4.0 * _err(g32[k], g64[k]), FLOOR) for k in live)
    print(f"variant {variant}: moves a gradient by {worst_v:.3e}, the widest bound is {bound:.3e}")
    assert worst_v > 100.0 * bound


def test_dropout_changes_the_loss_and_p_zero_is_the_plain_forward():
    cfg, state, mix, target = _tiny()
    (L, _, s64), _ = _truth()
    L0, g0, s0 = sd.loss_and_grads(mix, target, state, cfg, F64, 0.0, SEED, 3)
    Lp, gp, sp_ = st.loss_and_grads(mix, target, state, cfg, F64)
    assert float(L0) == float(Lp) and all(torch.equal(g0[k], gp[k]) for k in gp)
    assert float(L) != float(L0)
    assert torch.equal(s64["a.bn7"][0], s0["a.bn7"][0])      # the first dropped norm's statistics are taken before the drop
    assert not torch.equal(s64["a.bn8"][0], s0["a.bn8"][0])


# ------------------------------------------------------------------ refusals, draws and checkpoints without a device
def test_dropout_outside_zero_to_one_is_refused():
    cfg, state, _, _ = _tiny()
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dropout must be in"):
            SeparatorTrainer(cfg, state, dropout=p)
    tr = SeparatorTrainer(cfg, state, dropout=0.25, dropout_seed=SEED)
    lib = _lib.lib()
    assert lib.etd_septrain_set_dropout(tr.h, 1.0, 0) == -22 and b"outside [0, 1)" in lib.etd_last_error()
    assert lib.etd_septrain_set_dropout_calls(tr.h, -1) == -22
    assert tr.dropout_calls == 0 and tr.optimizer_state_dict()["dropout_calls"] == 0
    _lib.check(lib.etd_septrain_set_dropout_calls(tr.h, 41), "set")
    assert tr.dropout_calls == 41
    tr.close()


def test_bad_draws_are_refused_naming_the_unit():
    ok = (0, 5, 1.0, 1.0)
    frames = [100, 70]
    data.check_draws([ok, (1, 69, 0.9, 1.05)], frames, 64, 64)
    for bad, msg in (((2, 0, 1.0, 1.0), "unit 1: track 2"), ((-1, 0, 1.0, 1.0), "unit 1: track -1"), ((0, -1, 1.0, 1.0), "unit 1: t0 = -1"),
                     ((1, 70, 1.0, 1.0), "unit 1: t0 = 70"), ((0, 0, 0.02, 1.0), r"unit 1: T' = floor\(64 x 0.02\) = 1"), ((0, 0, 1.0, 0.03), "unit 1: F' ="),
                     ((0, 0, float("nan"), 1.0), "unit 1: a = nan"), ((0, 0, 1.0, float("inf")), "unit 1: a = 1.0 and q = inf")):
        with pytest.raises(ValueError, match=msg):
            data.check_draws([ok, bad], frames, 64, 64)
    with pytest.raises(ValueError, match="at least one"):
        data.check_draws([], frames, 64, 64)


def test_sampler_refusals_and_draws_without_a_device():
    cfg, _, _, _ = _tiny()
    with pytest.raises(ValueError, match="max_bytes"):
        data.SegmentSampler(cfg, max_bytes=0)
    with pytest.raises(ValueError, match="stretch"):
        data.SegmentSampler(cfg, stretch=(1.1, 0.9))
    sm = data.SegmentSampler(cfg, seed=7)
    with pytest.raises(ValueError, match="track 0: 1 stems for 2 instruments"):
        sm.add_track([np.zeros((1, 4000), np.float32)])
    with pytest.raises(ValueError, match="track 0: .*one length"):
        sm.add_track([np.zeros(4000, np.float32), np.zeros(4001, np.float32)])
    with pytest.raises(ValueError, match="track 0: song 1: audio must be"):
        sm.add_track([np.zeros(4000, np.float32), np.zeros((2, 2, 2), np.float32)])
    with pytest.raises(ValueError, match="no track"):
        sm.draw(2, 0, 0)
    with pytest.raises(ValueError, match="unit 0: track 0, the sampler holds 0"):
        sm.batch([(0, 0, 1.0, 1.0)])
    assert sm.num_tracks == 0 and sm.held_bytes == 0 and sm.track_bytes(65) == 3 * 128 * 64 * 1 * 4
    sm.frames = [100, 300]                              # the draws are host arithmetic on the tracks' lengths
    d = sm.draw(64, 1, 2)
    assert d == sm.draw(64, 1, 2) and d != sm.draw(64, 1, 3) and d != sm.draw(64, 2, 2)
    assert {k for k, _, _, _ in d} == {0, 1}
    assert all(0 <= t0 <= sm.frames[k] - 64 and 0.9 <= a < 1.1 and 2 ** (-1 / 12) <= q < 2 ** (1 / 12) for k, t0, a, q in d)
    plain = sm.draw(64, 1, 2, augment=False)
    assert [(k, t0) for k, t0, _, _ in plain] == [(k, t0) for k, t0, _, _ in d] and all(a == 1.0 and q == 1.0 for _, _, a, q in plain)
    data.check_draws(d, sm.frames, cfg.T, cfg.F)
    sm.frames = [10]                                    # a track shorter than a segment starts at 0
    assert all(t0 == 0 for _, t0, _, _ in sm.draw(8, 0, 0))
    ident = data.SegmentSampler(cfg, seed=7, stretch=None, pitch=None)
    ident.frames = [100]
    assert all(a == 1.0 and q == 1.0 for _, _, a, q in ident.draw(8, 0, 0))
    lib = _lib.lib()
    bad = _lib.SepDataCfg(n_instr=0, n_channels=1, T=64, F=64, max_bytes=0)
    import ctypes as C
    h = C.c_void_p()
    assert lib.etd_sepdata_create(C.byref(bad), C.byref(h)) == -22 and b"n_instr" in lib.etd_last_error()
    sm.frames = []
    sm.close(); ident.close()


def test_fit_and_validate_refuse_bad_arguments():
    with pytest.raises(ValueError, match="steps_per_epoch"):
        data.fit(None, None, 1, 0, 1)
    with pytest.raises(ValueError, match="start"):
        data.fit(None, None, 2, 3, 1, start=(0, 3))
    assert data.fit(None, None, 2, 3, 1, start=(2, 0)) == (2, 0)      # nothing left to do
    with pytest.raises(ValueError, match="un-augmented"):
        data.validate(None, None, [(0, 0, 0.95, 1.0)])


def test_checkpoint_round_trip_of_the_host_side_pieces(tmp_path):
    cfg, state, _, _ = _tiny()
    tr = SeparatorTrainer(cfg, state, max_units=3, lr=2e-3, betas=(0.8, 0.99), max_norm=1.5, dropout=0.5, dropout_seed=SEED)
    _lib.check(_lib.lib().etd_septrain_set_dropout_calls(tr.h, 6), "set")
    data.save_checkpoint(tmp_path / "c.ckpt", tr, 2, 1)
    ck = data.read_checkpoint(tmp_path / "c.ckpt")
    assert ck["cursor"] == (2, 1) and ck["config"] == cfg
    assert ck["hyper"] == dict(max_units=3, workspace_bytes=16 << 30, lr=2e-3, betas=(0.8, 0.99), eps=1e-8, max_norm=1.5, dropout=0.5, dropout_seed=SEED)
    assert list(ck["state"]) == list(state) and all(np.array_equal(ck["state"][k], state[k]) for k in state)
    assert ck["optimizer"]["step"] == 0 and ck["optimizer"]["dropout_calls"] == 6
    assert set(ck["optimizer"]["exp_avg"]) == set(tr.grads()) and not any(v.any() for v in ck["optimizer"]["exp_avg_sq"].values())
    torch.save({"format": "something else"}, tmp_path / "x.ckpt")
    with pytest.raises(ValueError, match="not a separator training checkpoint"):
        data.read_checkpoint(tmp_path / "x.ckpt")
    tr.close()


def test_symbols_declared_and_exported():
    lib = _lib.lib()
    public = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "etude_hip.h").read_text(), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "etude_hip_debug.h").read_text(), flags=re.S)
    for name in ("etd_septrain_set_dropout", "etd_septrain_set_dropout_calls", "etd_septrain_get_dropout_calls", "etd_sepdata_create", "etd_sepdata_destroy",
                 "etd_sepdata_track_bytes", "etd_sepdata_bytes", "etd_sepdata_num_tracks", "etd_sepdata_track_frames", "etd_sepdata_add_track", "etd_sepdata_sum_stems",
                 "etd_sepdata_gather"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", public), name
    assert hasattr(lib, "etd_septrain_debug_dropout") and "etd_septrain_debug_dropout" in _lib.SIGNATURES and re.search(r"\betd_septrain_debug_dropout\s*\(", debug)
    assert lib.etd_version() == 3
    import etude_amd
    assert etude_amd.SegmentSampler is data.SegmentSampler and etude_amd.fit_separator is data.fit and "SegmentSampler" in etude_amd.__all__
