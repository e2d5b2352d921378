"""Decoder dropout, the segment sampler and the training loop on the MI355X (csrc/separator_train.hip, csrc/separator_data.hip) against the restatement
(tests/separator_data_np.py): the mask bit for bit, the whole gradient under dropout, p = 0 against a trainer built without the argument, the gather against
``training_segments`` (identity) and against fp64 (stretched and shifted), batch independence, guards, refusals, a resumed run and a direction check.

The yardstick is tests/test_gpu_separator_train.py's: ``err = max|g - g64| / max|g64|`` against fp64, held to 4 x the same figure of the fp32 restatement on the same
input, with a floor of 4 * 2^-24."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_data_np as sd  # noqa: E402

from etude_amd import _lib, synth  # noqa: E402
from etude_amd import separator_data as data  # noqa: E402
from etude_amd.separator import SeparatorConfig, StemSeparator, init_separator_state  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer, training_segments  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
ODD = (3, 5, 8, 16, 24, 40)
SEED = 0x1234567890ABCDEF
T = F = 64
_cache = {}
_bad = []


def _rel(y, y64):
    y, y64 = torch.as_tensor(y), torch.as_tensor(y64)
    return float((y.to(F64) - y64.to(F64)).abs().max()) / float(y64.abs().max())


def _hold(what, dev, y32, y64):
    dev = torch.as_tensor(dev).cpu()
    y32, y64 = torch.as_tensor(y32), torch.as_tensor(y64)
    assert tuple(dev.shape) == tuple(y64.shape), (what, tuple(dev.shape), tuple(y64.shape))
    assert bool(torch.isfinite(dev).all()), what
    if float(y64.abs().max()) == 0.0:
        assert float(dev.abs().max()) == 0.0, what
        return
    e_dev, e_32 = _rel(dev, y64), _rel(y32, y64)
    print(f"SEPDATA_ERR {what}: device {e_dev:.3e} yardstick {e_32:.3e} ratio {e_dev / max(e_32, 2.0 ** -24):.2f}")
    if not e_dev <= max(4.0 * e_32, FLOOR):
        _bad.append((what, e_dev, e_32))


@pytest.fixture(autouse=True)
def _fresh_violations():
    _bad.clear()
    yield
    _bad.clear()


def _verdict():
    bad = list(_bad)
    _bad.clear()
    assert not bad, bad


def _cfg(Cn):
    return SeparatorConfig(instruments=("a", "b"), n_fft=1024, hop=256, T=T, F=F, n_channels=Cn, conv_n_filters=ODD)


def _case(B, Cn, seed=3):
    key = ("case", B, Cn, seed)
    if key not in _cache:
        cfg = _cfg(Cn)
        state = init_separator_state(cfg, seed)
        r = np.random.default_rng(seed)
        for k in state:
            if k.endswith(".bias"):
                state[k] = r.normal(0, 0.1, state[k].shape).astype(np.float32)
        g = torch.Generator().manual_seed(seed)
        mix = torch.rand(B, T, F, Cn, generator=g) * 2.0
        target = torch.rand(2, B, T, F, Cn, generator=g) * mix[None]
        _cache[key] = dict(cfg=cfg, state=state, mix=mix, target=target)
    return _cache[key]


def _set_calls(tr, n):
    _lib.check(_lib.lib().etd_septrain_set_dropout_calls(tr.h, n), "etd_septrain_set_dropout_calls")


# ------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_debug_dropout_is_the_restatements_mask_bit_for_bit(p):
    c = _case(3, 2)
    tr = SeparatorTrainer(c["cfg"], c["state"], max_units=3, dropout=p, dropout_seed=SEED)
    g = torch.Generator().manual_seed(41)
    for j in (1, 2, 3):
        y = torch.randn((3, 2) + tr._dec_shape(j), generator=g)
        for call in (0, 2 ** 32 + 5):                   # the counter's word is lo32(call)
            got = tr.debug_dropout(j, y.cuda(), call).cpu().numpy()
            want = sd.dropout_apply(y.numpy(), j, call, SEED, p)
            assert np.array_equal(got, want), (j, call)
            assert 0 < int((got == 0).sum()) < got.size
        n = y.numel() - 3                               # a count that is no multiple of 4: the last block is cut after one word
        got = tr.debug_dropout(j, y.cuda(), 5, numel=n).cpu().numpy().reshape(-1)
        assert np.array_equal(got[:n], sd.dropout_apply(y.numpy().reshape(-1)[:n].copy(), j, 5, SEED, p)) and np.array_equal(got[n:], y.numpy().reshape(-1)[n:])
    assert tr.dropout_calls == 0                        # the tap moves no counter
    with pytest.raises(_lib.EtudeHipError, match="level j = 4"):
        tr.debug_dropout(4, torch.zeros((3, 2) + tr._dec_shape(4)).cuda(), 0)
    tr.close()


@pytest.mark.parametrize("B,Cn", [(2, 2), (3, 1)])
def test_whole_gradient_and_loss_with_dropout(B, Cn):
    c = _case(B, Cn)
    key = ("drop", B, Cn)
    if key not in _cache:
        _cache[key] = tuple(sd.loss_and_grads(c["mix"], c["target"], c["state"], c["cfg"], dt, 0.5, SEED, 3) for dt in (F64, F32))
    (L64, g64, _), (L32, g32, _) = _cache[key]
    tr = SeparatorTrainer(c["cfg"], c["state"], max_units=3, dropout=0.5, dropout_seed=SEED)
    _set_calls(tr, 3)
    loss = tr.loss_and_backward(c["mix"], c["target"])
    print(f"SEPDATA_LOSS B={B} C={Cn}: device {loss:.9e} fp64 {float(L64):.9e} fp32 {float(L32):.9e}")
    assert abs(loss - float(L64)) <= max(4.0 * abs(float(L32) - float(L64)), FLOOR * abs(float(L64)))
    got = tr.grads()
    for k in g64:
        _hold(f"dropout grad {k} B={B} C={Cn}", got[k], g32[k], g64[k])
    assert tr.dropout_calls == 4
    tr.close()
    _verdict()


def test_dropout_is_a_function_of_the_seed_and_the_call_counter_and_loss_never_drops():
    c = _case(2, 2)
    out = []
    for _ in range(2):
        tr = SeparatorTrainer(c["cfg"], c["state"], max_units=2, dropout=0.5, dropout_seed=SEED)
        plain = tr.loss(c["mix"], c["target"])
        first = (tr.loss_and_backward(c["mix"], c["target"]), tr.grads())
        tr.zero_grad()
        second = (tr.loss_and_backward(c["mix"], c["target"], frozen_stats=True), tr.grads())
        out.append((plain, first, second, tr.dropout_calls))
        tr.close()
    a, b = out
    assert a[0] == b[0] and a[1][0] == b[1][0] and a[2][0] == b[2][0] and a[3] == b[3] == 2
    for k in a[1][1]:
        assert np.array_equal(a[1][1][k], b[1][1][k]) and np.array_equal(a[2][1][k], b[2][1][k]), k
    tr = SeparatorTrainer(c["cfg"], c["state"], max_units=2, dropout=0.5, dropout_seed=SEED)
    _set_calls(tr, 1)                                   # the second call's mask on the first call's statistics: the counter alone changes the result
    moved = tr.loss_and_backward(c["mix"], c["target"])
    assert moved != a[1][0]
    tr.close()
    tr0 = SeparatorTrainer(c["cfg"], c["state"], max_units=2)
    assert tr0.loss(c["mix"], c["target"]) == a[0]      # loss() is unchanged by p ...
    assert tr0.loss_and_backward(c["mix"], c["target"]) != a[1][0] and tr0.dropout_calls == 0      # ... and loss_and_backward is not
    tr0.close()
    other = SeparatorTrainer(c["cfg"], c["state"], max_units=2, dropout=0.5, dropout_seed=SEED + 1)
    assert other.loss_and_backward(c["mix"], c["target"]) != a[1][0]
    other.close()


def test_dropout_zero_is_the_trainer_built_without_the_argument_bit_for_bit():
    c = _case(2, 2)
    out = []
    for kw in ({}, {"dropout": 0.0, "dropout_seed": SEED}):
        tr = SeparatorTrainer(c["cfg"], c["state"], max_units=2, lr=1e-3, **kw)
        loss = tr.loss_and_backward(c["mix"], c["target"])
        grads = tr.grads()
        tr.step()
        out.append((loss, grads, tr.state_dict(), tr.optimizer_state_dict()))
        assert tr.dropout_calls == 0
        tr.close()
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    for k in out[0][2]:
        assert np.array_equal(out[0][2][k], out[1][2][k]), k
    assert any(not np.array_equal(out[0][2][k], c["state"][k]) for k in c["state"])
    assert out[0][3]["dropout_calls"] == 0 and all(np.array_equal(out[0][3]["exp_avg"][k], out[1][3]["exp_avg"][k]) for k in out[0][3]["exp_avg"])


# ------------------------------------------------------------------ the gather
def _audio(N, seed, Cn):
    x = np.ascontiguousarray(synth.clip_audio(seed, seconds=(N + 4410) / 44100.0)[:, :N], np.float32)
    return x if Cn == 2 else np.ascontiguousarray(x[:1])


NS = (95 * 256 + 5, 37 * 256 + 100)                     # Tf = 100 (a segment and a part) and 42 (shorter than a segment)


def _corpus(Cn):
    """a sampler over two tracks (the first with its own mix, the second with the stems' sum) and the tracks' magnitudes as ``training_segments`` gives them"""
    key = ("corpus", Cn)
    if key not in _cache:
        cfg = _cfg(Cn)
        sm = data.SegmentSampler(cfg, seed=5)
        sep = StemSeparator(cfg, seed=1)
        tracks, wavs = [], []
        for k, N in enumerate(NS):
            stems = [_audio(N, 80 + 10 * k + 2 * i, Cn) for i in range(2)]
            own_mix = _audio(N, 90 + 10 * k, Cn) if k == 0 else None
            assert sm.add_track(stems, own_mix) == k
            mix_wav = own_mix if own_mix is not None else (torch.from_numpy(stems[0]).cuda() + torch.from_numpy(stems[1]).cuda())
            m, t = training_segments(sep, mix_wav, stems)
            S = torch.cat([m[None], t]).reshape(3, -1, F, Cn).cpu().numpy()
            tracks.append((S, sep.num_frames(N)))
            wavs.append(stems)
        sep.close()
        _cache[key] = (sm, tracks, wavs)
    return _cache[key]


@pytest.mark.parametrize("Cn", [1, 2])
def test_identity_draws_are_the_frames_of_training_segments(Cn):
    sm, tracks, _ = _corpus(Cn)
    assert sm.frames == [100, 42] and sm.num_tracks == 2 and sm.held_bytes == sm.track_bytes(100) + sm.track_bytes(42)
    draws = [(0, 0, 1.0, 1.0), (0, 17, 1.0, 1.0), (0, 60, 1.0, 1.0), (0, 99, 1.0, 1.0), (1, 0, 1.0, 1.0), (1, 41, 1.0, 1.0)]
    for part in (draws[:3], draws[3:]):
        mix, target = sm.batch(part)
        assert mix.is_cuda and tuple(mix.shape) == (3, T, F, Cn) and tuple(target.shape) == (2, 3, T, F, Cn)
        got = torch.cat([mix[None], target]).cpu().numpy()
        for u, (k, t0, _, _) in enumerate(part):
            S, Tf = tracks[k]
            want = np.zeros((3, T, F, Cn), np.float32)
            n = min(T, Tf - t0)
            want[:, :n] = S[:, t0:t0 + n]
            assert np.array_equal(got[:, u], want), (k, t0)
            assert want[:, :n].any() and (n == T or not got[:, u, n:].any())
    # the mix of the track given by its stems alone is the magnitude of their fp32 sum: tracks[1] was made from that sum by training_segments


@pytest.mark.parametrize("Cn", [1, 2])
def test_stretched_and_shifted_draws_against_fp64(Cn):
    """the pad branch (a = 0.9), the crop branch (a = 1.1), the zero band above F' (q < 1), q > 1, and windows that run past Tf"""
    sm, tracks, _ = _corpus(Cn)
    lo, hi = 2.0 ** (-1 / 12), 2.0 ** (1 / 12)
    draws = [(0, 3, 0.9, 1.0), (0, 30, 1.1, 1.0), (0, 36, 1.0, lo), (1, 0, 1.0, hi), (0, 70, 0.9, hi), (1, 20, 1.1, lo), (0, 11, 0.9371, 1.0312), (1, 5, 1.0629, 0.9713),
             (0, 0, 1.0, 1.0)]
    for b in range(0, len(draws), 3):
        part = draws[b:b + 3]
        mix, target = sm.batch(part)
        got = torch.cat([mix[None], target]).cpu()
        m64, t64 = sd.batch(tracks, part, T, np.float64)
        m32, t32 = sd.batch(tracks, part, T, np.float32)
        w64, w32 = np.concatenate([m64[None], t64]), np.concatenate([m32[None], t32])
        for u, d in enumerate(part):
            _hold(f"gather C={Cn} {d}", got[:, u], w32[:, u], w64[:, u])
            Tp, Fp = sd.stretched_sizes(T, F, d[2], d[3])
            if Tp < T:
                assert not got[:, u, :(T - Tp) // 2].any() and not got[:, u, (T - Tp) // 2 + Tp:].any()
            if Fp < F:
                assert not got[:, u, :, Fp:].any()
            assert np.array_equal(got[:, u].numpy() == 0, w32[:, u] == 0), d      # the zeros of the geometry sit where the restatement's do
    _verdict()


def test_a_units_output_is_the_same_alone_and_anywhere_in_a_batch():
    sm, _, _ = _corpus(2)
    d = [(0, 11, 0.9371, 1.0312), (1, 5, 1.0629, 0.9713), (0, 70, 0.9, 2.0 ** (1 / 12))]
    alone = [sm.batch([x]) for x in d]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        mix, target = sm.batch([d[i] for i in order])
        for pos, i in enumerate(order):
            assert torch.equal(mix[pos], alone[i][0][0]) and torch.equal(target[:, pos], alone[i][1][:, 0]), (order, pos)


def test_the_mix_of_a_track_without_one_is_the_fp32_sum_of_its_stems():
    cfg = _cfg(2)
    sm = data.SegmentSampler(cfg)
    lib = _lib.lib()
    g = torch.Generator().manual_seed(3)
    stems = [torch.randn(2, 1001, generator=g).cuda() for _ in range(2)]
    mix = torch.full((2 * 1001 + 64,), float("nan"), device="cuda")
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in stems])
    _lib.check(lib.etd_sepdata_sum_stems(sm.h, ptrs, 2 * 1001, C.c_void_p(mix.data_ptr() + 128), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sum")
    torch.cuda.synchronize()
    assert torch.equal(mix[32:32 + 2002], (stems[0] + stems[1]).reshape(-1)) and bool(torch.isnan(mix[:32]).all()) and bool(torch.isnan(mix[32 + 2002:]).all())
    sm.close()


GUARD = 64
NAN_BITS = 0x7FC0DEAD


class _Guarded:
    """n floats on the device between two guards, all holding NAN_BITS until a kernel writes them (tests/test_gpu_separator_train.py)"""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def check(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == NAN_BITS).all(), f"{what}: written below the buffer"
        assert (b[GUARD + self.n:] == NAN_BITS).all(), f"{what}: written beyond the buffer"
        assert not (b[GUARD:GUARD + self.n] == NAN_BITS).any(), f"{what}: a float inside was never written"


def _arrays(draws):
    B = len(draws)
    return ((C.c_int32 * B)(*[d[0] for d in draws]), (C.c_int64 * B)(*[d[1] for d in draws]), (C.c_double * B)(*[d[2] for d in draws]),
            (C.c_double * B)(*[d[3] for d in draws]))


@pytest.mark.parametrize("Cn", [1, 2])
def test_guard_floats_around_both_outputs_are_untouched(Cn):
    sm, _, _ = _corpus(Cn)
    lib = _lib.lib()
    draws = [(0, 70, 0.9, 2.0 ** (1 / 12)), (1, 41, 1.1, 2.0 ** (-1 / 12)), (0, 99, 1.0, 1.0)]
    mix, target = _Guarded(3 * T * F * Cn), _Guarded(2 * 3 * T * F * Cn)
    _lib.check(lib.etd_sepdata_gather(sm.h, 3, *_arrays(draws), mix.ptr, target.ptr, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gather")
    mix.check("mix"); target.check("target")


def test_bad_draws_and_tracks_are_refused_and_the_engine_goes_on():
    sm, _, _ = _corpus(2)
    lib = _lib.lib()
    ok = (0, 5, 1.0, 1.0)
    want = sm.batch([ok])
    out = _Guarded(3 * T * F * 2), _Guarded(2 * 3 * T * F * 2)
    st0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad, msg in (((2, 0, 1.0, 1.0), b"unit 1: track 2"), ((0, 100, 1.0, 1.0), b"unit 1: t0 = 100"), ((0, -1, 1.0, 1.0), b"unit 1: t0 = -1"),
                     ((0, 0, 0.02, 1.0), b"unit 1: T' ="), ((0, 0, 1.0, 0.02), b"unit 1: F' ="), ((0, 0, float("nan"), 1.0), b"unit 1: a = nan")):
        assert lib.etd_sepdata_gather(sm.h, 2, *_arrays([ok, bad]), out[0].ptr, out[1].ptr, st0) == -22      # the library's own refusal, before the launch
        assert msg in lib.etd_last_error(), (bad, lib.etd_last_error())
        with pytest.raises(ValueError, match="unit 1"):
            sm.batch([ok, bad])
    torch.cuda.synchronize()
    assert (out[0].buf.cpu().numpy() == NAN_BITS).all() and (out[1].buf.cpu().numpy() == NAN_BITS).all()      # nothing was launched
    with pytest.raises(ValueError, match="track 2: stem 1 holds a non-finite"):
        sm.add_track([np.zeros((2, 3000), np.float32), np.full((2, 3000), np.inf, np.float32)])
    again = sm.batch([ok])
    assert sm.num_tracks == 2 and torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    small = data.SegmentSampler(_cfg(2), max_bytes=sm.track_bytes(42))
    z = np.zeros((2, NS[1]), np.float32)
    assert small.add_track([z, z]) == 0
    with pytest.raises(_lib.EtudeHipError, match=f"needs {small.track_bytes(42)} bytes"):
        small.add_track([z, z])
    assert small.num_tracks == 1 and not small.batch([(0, 0, 1.0, 1.0)])[0].any()
    small.close()


# ------------------------------------------------------------------ the loop
def _band_sampler():
    cfg = _cfg(2)
    sm = data.SegmentSampler(cfg, seed=5)
    for k, N in enumerate((95 * 256 + 5, 150 * 256 + 77)):
        sm.add_track(list(sd.two_band_stems(N, 70 + k)))
    return cfg, sm


def test_a_resumed_run_continues_with_the_bits_of_an_uninterrupted_one(tmp_path):
    cfg, sm = _band_sampler()
    state = init_separator_state(cfg, 3)
    kw = dict(max_units=2, lr=1e-3, max_norm=5.0, dropout=0.5, dropout_seed=9)
    whole = SeparatorTrainer(cfg, state, **kw)
    seen = []
    assert data.fit(whole, sm, 3, 3, 2, accumulate=2, on_step=lambda e, s, loss: seen.append((e, s, loss))) == (3, 0)
    assert [(e, s) for e, s, _ in seen] == [(e, s) for e in range(3) for s in range(3)] and all(np.isfinite(l) for _, _, l in seen)
    first = SeparatorTrainer(cfg, state, **kw)
    cursor = data.fit(first, sm, 2, 3, 2, accumulate=2)
    assert cursor == (2, 0)
    data.save_checkpoint(tmp_path / "run.ckpt", first, *cursor)
    first.close()
    resumed, start = data.load_checkpoint(tmp_path / "run.ckpt")
    assert start == (2, 0) and resumed.dropout == 0.5 and resumed.dropout_seed == 9 and resumed.max_norm == 5.0 and resumed.dropout_calls == 12
    tail = []
    assert data.fit(resumed, sm, 3, 3, 2, accumulate=2, on_step=lambda e, s, loss: tail.append((e, s, loss)), start=start) == (3, 0)
    assert tail == seen[6:]
    a, b = whole.state_dict(), resumed.state_dict()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    oa, ob = whole.optimizer_state_dict(), resumed.optimizer_state_dict()
    assert oa["step"] == ob["step"] == 9 and oa["dropout_calls"] == ob["dropout_calls"] == 18
    for part in ("exp_avg", "exp_avg_sq"):
        for k in oa[part]:
            assert np.array_equal(oa[part][k], ob[part][k]), (part, k)
    assert any(not np.array_equal(a[k], state[k]) for k in state)
    whole.close(); resumed.close(); sm.close()


def test_a_few_augmented_steps_with_dropout_lower_the_validation_loss():
    """Two tracks of two sources in disjoint bands, six steps of two augmented units at lr = 2e-3 with p = 0.5; validation on four held-out un-augmented units with
    the running statistics and no dropout.  The fp32 restatement alone (tests/separator_data_np.py: batch, train_steps, frozen_loss on the restated STFT magnitudes
    of the same audio and the same draws) goes from 2.356194 before to 2.251264 after these six steps (2.217804 after twelve): a drop of 4.5 %, some four orders of
    magnitude above what fp32 rounding moves a loss by.  A direction check with no threshold."""
    cfg, sm = _band_sampler()
    tr = SeparatorTrainer(cfg, init_separator_state(cfg, 3), max_units=4, lr=2e-3, dropout=0.5, dropout_seed=9)
    held_out = sm.draw(4, 10 ** 6, 0, augment=False)
    before = data.validate(tr, sm, held_out)
    losses = []
    data.fit(tr, sm, 1, 6, 2, on_step=lambda e, s, loss: losses.append(loss))
    after = data.validate(tr, sm, held_out)
    print("SEPDATA_LEARN before", f"{before:.6e}", "after", f"{after:.6e}", "steps", " ".join(f"{v:.6e}" for v in losses))
    assert tr.dropout_calls == 6 and after < before
    tr.close(); sm.close()
