"""The separator's multichannel Wiener stage on the MI355X (csrc/separator_mwf.hip, StemSeparator(mwf_iterations=...)) against the restatement of DESIGN.md 4r
(tests/separator_mwf_np.py): the stage on its own tapped input at every chunk edge of the source model, inputs whose covariances are singular, the whole chain,
"off means off", and bit identity across batches and workspace budgets.  Beside the small config, the tile edges the product's shape (five stereo stems,
F = 1024) lies beyond: F above one 64-bin tile, 1, 4, 5 and 16 sources, and a song longer than k_mwf_scale's grid.

The yardstick is the 4 x rule of tests/test_gpu_separator.py, copied: every device figure is ``err = max|y_dev - y64| / max|y64|``, y64 the restatement in fp64, and is
held to 4 x the same figure of the restatement run in fp32 through torch-CPU ops on the same input, with a floor of 4 * 2^-24.  (Where the truth is all zeros -- a
silent song -- the figure is the absolute error, which the floor then holds to zero for all purposes; the test asks for exact zeros besides.)
The small config (n_fft = 1024, T = F = 64) is that file's; the cases that need more bins widen F alone."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_mwf_np as mw  # noqa: E402
import separator_np as sp  # noqa: E402

from etude_amd.separator import SeparatorConfig, StemSeparator, init_separator_state  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
ODD = (3, 5, 8, 16, 24, 40)
N_FFT = 1024
_cache = {}
_bad = []


def _rel(y, y64):
    y, y64 = torch.as_tensor(y), torch.as_tensor(y64)
    if y.is_complex():
        y, y64 = torch.view_as_real(y), torch.view_as_real(y64)
    den = float(y64.abs().max())
    return float((y.to(F64) - y64.to(F64)).abs().max()) / (den if den > 0 else 1.0)


def _hold(what, dev, y32, y64):
    """the 4 x rule: prints both figures and notes a violation for ``_verdict``, which every test ends with"""
    assert tuple(dev.shape) == tuple(y64.shape), (what, tuple(dev.shape), tuple(y64.shape))
    assert bool(torch.isfinite(torch.view_as_real(dev) if dev.is_complex() else dev).all()), what
    e_dev, e_32 = _rel(dev.cpu(), y64), _rel(y32, y64)
    print(f"SEP_ERR {what}: device {e_dev:.3e} yardstick {e_32:.3e} ratio {e_dev / max(e_32, 2.0 ** -24):.2f}")
    if not e_dev <= max(4.0 * e_32, FLOOR):
        _bad.append((what, e_dev, e_32))


@pytest.fixture(autouse=True)
def _fresh_violations():
    """a test that raised before its ``_verdict`` leaves nothing behind for the next one"""
    _bad.clear()
    yield
    _bad.clear()


def _verdict():
    """every figure of a test is printed before the first one fails it"""
    bad = list(_bad)
    _bad.clear()
    assert not bad, bad


def _engine(instruments=("a", "b"), channels=2, seed=3, F=64, T=64, **kw):
    key = (instruments, channels, seed, F, T, tuple(sorted(kw.items())))
    if key not in _cache:
        cfg = SeparatorConfig(instruments=instruments, n_fft=N_FFT, hop=N_FFT // 4, T=T, F=F, conv_n_filters=ODD, n_channels=channels)
        skey = ("state", instruments, channels, seed)            # (the weights' shapes depend on neither F nor T)
        if skey not in _cache:
            _cache[skey] = init_separator_state(cfg, seed)
        _cache[key] = StemSeparator(cfg, _cache[skey], **kw)
    return _cache[key]


def _audio(N, channels=2, seed=0):
    r = np.random.default_rng(seed)
    t = np.arange(N) / 44100.0
    x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 + 110.0 * c) * t + c) + 0.1 * r.standard_normal(N) for c in range(channels)])
    return x.astype(np.float32)


def _tapped(sep, wav):
    """the engine's own X (its STFT below bin F) and Y (its mask pass on the logits of the fp32 restatement's U-Nets with the engine's random weights), as CPU
    complex64 tensors: the input the stage is tapped on"""
    cfg = sep.config
    X = sep.debug_stft(torch.from_numpy(wav).cuda())[:, :, :cfg.F].contiguous()
    M = sp.magnitudes(X.cpu(), cfg.F, cfg.T)
    logits = torch.stack([torch.stack([sp.unet(M[s], sep.state, name, cfg.bn_eps, F32) for name in cfg.instruments]) for s in range(M.shape[0])])
    Y = sep.debug_mask(logits.cuda(), M.reshape(-1, cfg.F, cfg.n_channels).cuda(), X)
    return X.cpu(), Y.cpu()


def _stage(sep, what, X, Y, iterations=(1, 2)):
    for n in iterations:
        got = sep.debug_mwf(X.cuda(), Y.cuda(), n)
        assert got.is_cuda and got.dtype == torch.complex64
        _hold(f"mwf {what} n={n}", got, mw.wiener(X, Y, n, F32), mw.wiener(X.to(torch.complex128), Y.to(torch.complex128), n, F64))
    return got


# ------------------------------------------------------------------ the stage on its own tapped input
FRAMES = ((1, 5), (15104, 64), (15360, 65), (20000, 83))          # (N, Tf)
PRODUCT = ("vocals", "piano", "drums", "bass", "other")


@pytest.mark.parametrize("channels,instruments,F,frames", [(2, ("a", "b"), 64, FRAMES), (2, ("a", "b", "c"), 64, FRAMES), (1, ("a", "b", "c"), 64, FRAMES),
                                                           (2, PRODUCT, 192, (FRAMES[0], FRAMES[3])), (1, ("a", "b", "c"), 128, (FRAMES[0], FRAMES[3]))],
                         ids=["2-instruments0", "2-instruments1", "1-instruments2", "C2-I5-F192", "C1-I3-F128"])
def test_stage_at_every_chunk_edge(channels, instruments, F, frames):
    """Tf = 5 (one short chunk), 64 (the chunk edge), 65 (one frame past it), 83 (a ragged second chunk); 1 and 2 iterations.  F = 192 with five sources: I F = 960
    is four column blocks of k_mwf_stats and 15 workgroups of k_mwf_reduce, and k_mwf_apply reads R at k0 = 0, 64, 128; F = 128 with three: two of each, mono"""
    sep = _engine(instruments, channels, F=F)
    for N, Tf in frames:
        assert sep.num_frames(N) == Tf
        X, Y = _tapped(sep, _audio(N, channels, seed=N))
        assert tuple(Y.shape) == (len(instruments), channels, Tf, F)
        got = _stage(sep, f"C={channels} I={len(instruments)}{'' if F == 64 else f' F={F}'} Tf={Tf}", X, Y)
        assert float((got.cpu() - Y).abs().max()) > 1e-4 * float(Y.abs().max())          # (the stage does move the estimates)
    assert torch.equal(sep.debug_mwf(X.cuda(), Y.cuda(), 0).cpu(), Y)                      # n = 0 returns Y untouched
    _verdict()


@pytest.mark.parametrize("n_instr,channels", [(1, 2), (4, 2), (16, 2), (16, 1)])
def test_stage_at_the_edges_of_the_source_count(n_instr, channels):
    """k_mwf_apply<C, I> is compiled per source count: the first (1), the last (16, mono too) and 4; Tf = 65.  A single source is still moved (reg is not zero);
    "the stage does move the estimates" is asked of the device wherever the fp64 restatement says so"""
    sep = _engine(tuple(f"s{i}" for i in range(n_instr)), channels)
    N, Tf = FRAMES[2]
    X, Y = _tapped(sep, _audio(N, channels, seed=100 + n_instr))
    assert tuple(Y.shape) == (n_instr, channels, Tf, 64)
    got = _stage(sep, f"C={channels} I={n_instr} Tf={Tf}", X, Y)
    y64 = mw.wiener(X.to(torch.complex128), Y.to(torch.complex128), 2, F64)
    moved = float((y64 - Y).abs().max()) / float(Y.abs().max())
    print(f"SEP_MOVED C={channels} I={n_instr}: the fp64 restatement moves Y by {moved:.3e} of its largest entry")
    if moved > 2e-4:                                 # (twice what is asked of the device: its own error, held above to some 1e-6, cannot close that gap)
        assert float((got.cpu() - Y).abs().max()) > 1e-4 * float(Y.abs().max())
    _verdict()


def test_the_scale_sees_a_maximum_beyond_its_grid():
    """k_mwf_scale runs at most 1024 workgroups of 256 and strides from there: C Tf F = 2 x 300 x 512 = 307200 > 262144.  X is of unit scale but for one entry of
    magnitude 500 at a flat index past 262144, so s = 50 exists only if the strided part is read; s = 1 instead moves the result by far more than the rule allows"""
    C, Tf, F = 2, 300, 512
    sep = _engine(("a", "b"), C, F=F)
    g = torch.Generator().manual_seed(31)
    X = torch.complex(torch.randn(C, Tf, F, generator=g), torch.randn(C, Tf, F, generator=g)) * 0.5 ** 0.5
    spike = (1, Tf - 1, 137)
    flat = (spike[0] * Tf + spike[1]) * F + spike[2]
    assert C * Tf * F > 262144 and flat >= 262144
    X[spike] = torch.polar(torch.tensor(500.0), torch.tensor(0.7))
    assert float(X.reshape(-1)[:262144].abs().max()) < 10.0 and float(mw.song_scale(X, F64)) == pytest.approx(50.0, rel=1e-6)
    m = 0.1 + 0.8 * torch.rand(C, Tf, F, generator=g)
    Y = torch.stack([m * X, (1.0 - m) * X])
    X128, Y128 = X.to(torch.complex128), Y.to(torch.complex128)
    for n in (1, 2):
        got = sep.debug_mwf(X.cuda(), Y.cuda(), n)
        y32, y64 = mw.wiener(X, Y, n, F32), mw.wiener(X128, Y128, n, F64)
        _hold(f"mwf strided maximum C={C} I=2 F={F} Tf={Tf} n={n}", got, y32, y64)
        allowed, unscaled = max(4.0 * _rel(y32, y64), FLOOR), _rel(mw.wiener(X128, Y128, n, F64, scale=1.0), y64)
        print(f"SEP_DISCRIMINATES n={n}: s = 1 moves the fp64 restatement by {unscaled:.3e}, the rule allows {allowed:.3e}")
        assert unscaled > allowed
    _verdict()


def test_a_loud_song_is_scaled():
    """max|X| far above 10: s > 1 takes part (the songs above have s = 1 at their shortest only)"""
    sep = _engine(("a", "b", "c"))
    X, Y = _tapped(sep, 40.0 * _audio(15360, seed=7))
    assert float(X.abs().max()) > 1000.0
    _stage(sep, "loud", X, Y)
    _verdict()


def test_degenerate_inputs_stay_finite_and_within_the_rule():
    sep = _engine(("a", "b", "c"))
    N = 15360
    X, Y = _tapped(sep, np.zeros((2, N), np.float32))                                       # silence
    assert float(X.abs().max()) == 0.0 and float(Y.abs().max()) == 0.0
    got = _stage(sep, "all-zero song", X, Y)
    assert float(got.abs().max()) == 0.0
    quiet = _audio(N, seed=11)
    quiet[1] = 0.0                                                                          # one silent channel
    X, Y = _tapped(sep, quiet)
    got = _stage(sep, "silent channel", X, Y)
    assert float(got[:, 1].abs().max()) == 0.0 and float(got[:, 0].abs().max()) > 0.0
    mono = _audio(N, channels=1, seed=12)
    X, Y = _tapped(sep, np.concatenate([mono, mono]))                                       # mono duplicated to stereo: rank-1 covariances
    assert torch.equal(X[0], X[1])
    _stage(sep, "mono duplicated", X, Y)
    _verdict()


# ------------------------------------------------------------------ the whole chain
def _songs():
    if "songs" not in _cache:
        _cache["songs"] = [_audio(64 * 256 + 5, seed=21), _audio(5000, channels=1, seed=23)[0]]
    return _cache["songs"]


def _chain(wav, cfg, state, dtype, iterations):
    """tests/separator_np.py's ``separate`` with the Wiener restatement between the masks and the inverse STFT"""
    x = torch.as_tensor(wav).to(dtype)
    N = x.shape[1]
    X = sp.stft(x, cfg.n_fft, dtype)
    Xf = X[:, :, :cfg.F]
    M = sp.magnitudes(X, cfg.F, cfg.T)
    logits = torch.stack([torch.stack([sp.unet(M[s], state, name, cfg.bn_eps, dtype) for name in cfg.instruments]) for s in range(M.shape[0])])
    Y = sp.apply_masks(logits, M, Xf, cfg.separation_exponent, cfg.mask_eps)
    return sp.istft(mw.wiener(Xf, Y, iterations, dtype), N, cfg.n_fft)


@pytest.mark.parametrize("which,names", [(0, ("vocals", "drums", "other")), (1, ("vocals", "drums", "other")), (0, PRODUCT)], ids=["0", "1", "0-five-stems"])
def test_whole_chain(which, names):
    sep = _engine(names, seed=4)
    x = _songs()[which]
    got = sep.separate_many([x], mwf_iterations=1)[0]
    x2 = x if x.ndim == 2 else np.stack([x, x])
    assert got.is_cuda and tuple(got.shape) == (len(names), 2, x2.shape[1]) and sep.mwf_iterations == 0
    _hold(f"mwf chain song {which}{'' if len(names) == 3 else f' I={len(names)}'}", got, _chain(x2, sep.config, sep.state, F32, 1), _chain(x2, sep.config, sep.state, F64, 1))
    plain = sep.separate_many([x])[0]
    assert float((got - plain).abs().max()) > 1e-4 * float(plain.abs().max())              # (the filter took part)
    _verdict()


def test_off_means_off_and_the_per_call_override_is_the_engine_built_with_that_value():
    songs = _songs()
    base, zero, two = _engine(("vocals", "drums", "other"), seed=4), _engine(("vocals", "drums", "other"), seed=4, mwf_iterations=0), \
        _engine(("vocals", "drums", "other"), seed=4, mwf_iterations=2)
    assert (base.mwf_iterations, zero.mwf_iterations, two.mwf_iterations) == (0, 0, 2)
    plain, off, on = base.separate_many(songs), zero.separate_many(songs), two.separate_many(songs)
    over, back = base.separate_many(songs, mwf_iterations=2), two.separate_many(songs, mwf_iterations=0)
    assert base.mwf_iterations == 0 and two.mwf_iterations == 2                             # (an override does not stick)
    for i in range(len(songs)):
        assert torch.equal(plain[i], off[i]) and torch.equal(plain[i], back[i]), i
        assert torch.equal(on[i], over[i]) and not torch.equal(on[i], plain[i]), i
    assert two.workspace_total_bytes([5000]) >= base.workspace_total_bytes([5000])


def test_with_the_filter_on_a_song_is_bit_identical_alone_in_a_batch_under_a_tight_budget_and_again():
    songs = _songs() + [_audio(20000, seed=25)]
    for names in (("vocals", "drums", "other"), PRODUCT):
        sep, tight = _engine(names, seed=4, mwf_iterations=2), _engine(names, seed=4, mwf_iterations=2, workspace_bytes=1)
        batch = sep.separate_many(songs)
        again = sep.separate_many(songs[::-1])[::-1]
        small = tight.separate_many(songs)              # 1 byte: one song per group, one unit per launch, the work region at the stage's floor
        for i, x in enumerate(songs):
            alone = sep.separate_many([x])[0]
            assert bool(torch.isfinite(alone).all())
            assert torch.equal(alone, batch[i]) and torch.equal(alone, again[i]) and torch.equal(alone, small[i]), (names, i)
