"""The source separator on the MI355X (csrc/separator.hip, etude_amd.StemSeparator) against the restatement of DESIGN.md 4m (tests/separator_np.py): every stage on
its own tapped fp32 input, the whole chain, bit identity across batches and workspace budgets, and the route from audio to tempo.json.

The yardstick is not a constant (the rule of tests/test_gpu_train.py).  Every device figure is ``err = max|y_dev - y64| / max|y64|``, y64 the restatement in fp64, and
is held to 4 x the same figure of the restatement run in fp32 through torch-CPU ops on the same input, with a floor of 4 * 2^-24 where fp32 torch happens to be exact.
The small config (n_fft = 1024, T = F = 64) puts the bottleneck at 1 x 1, so every padding edge of every layer is live."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_np as sp  # noqa: E402

from etude_amd import synth  # noqa: E402
from etude_amd.separator import SeparatorConfig, StemSeparator, init_separator_state  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
DEFAULT = (16, 32, 64, 128, 256, 512)
ODD = (3, 5, 8, 16, 24, 40)
_cache = {}
_bad = []


def _rel(y, y64):
    y, y64 = torch.as_tensor(y), torch.as_tensor(y64)
    if y.is_complex():
        y, y64 = torch.view_as_real(y), torch.view_as_real(y64)
    return float((y.to(F64) - y64.to(F64)).abs().max()) / float(y64.abs().max())


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


def _engine(filters=DEFAULT, T=64, F=64, n_fft=1024, instruments=("a", "b"), seed=3, **kw):
    key = (filters, T, F, n_fft, instruments, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        cfg = SeparatorConfig(instruments=instruments, n_fft=n_fft, hop=n_fft // 4, T=T, F=F, conv_n_filters=filters)
        skey = ("state", filters, instruments, seed)
        if skey not in _cache:
            _cache[skey] = init_separator_state(cfg, seed)
        _cache[key] = StemSeparator(cfg, _cache[skey], **kw)
    return _cache[key]


def _audio(N, channels=2, seed=0):
    r = np.random.default_rng(seed)
    t = np.arange(N) / 44100.0
    x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 + 110.0 * c) * t + c) + 0.1 * r.standard_normal(N) for c in range(channels)])
    return x.astype(np.float32)


# ------------------------------------------------------------------ STFT and its inverse
@pytest.mark.parametrize("n_fft", [1024, 4096])
def test_stft_stage(n_fft):
    sep = _engine(ODD, n_fft=n_fft)
    hop = n_fft // 4
    for N in (1, hop - 1, hop, n_fft + 1, 3 * n_fft + 17):
        x = _audio(N, seed=N)
        got = sep.debug_stft(torch.from_numpy(x).cuda())
        _hold(f"stft n_fft={n_fft} N={N}", got, sp.stft(x, n_fft, F32), sp.stft(x, n_fft, F64))
    _verdict()


@pytest.mark.parametrize("n_fft", [1024, 4096])
def test_inverse_stft_stage(n_fft):
    sep = _engine(ODD, n_fft=n_fft)
    hop, Fb = n_fft // 4, 64
    for N in (1, hop - 1, hop, n_fft + 1, 3 * n_fft + 17):
        g = torch.Generator().manual_seed(N)
        Tf = sep.num_frames(N)
        Y = torch.complex(torch.randn(2, 2, Tf, Fb, generator=g), torch.randn(2, 2, Tf, Fb, generator=g))
        got = sep.debug_istft(Y.cuda(), N)
        _hold(f"istft n_fft={n_fft} N={N}", got, sp.istft(Y, N, n_fft), sp.istft(Y.to(torch.complex128), N, n_fft))
    _verdict()


def test_stft_then_inverse_on_the_device_returns_the_band_limited_waveform():
    sep = _engine(ODD, F=512)                          # F = n_fft / 2: every bin but the Nyquist bin passes
    N = 3 * 1024 + 17
    x = _audio(N, seed=1)
    X = sep.debug_stft(torch.from_numpy(x).cuda())[:, :, :512]
    got = sep.debug_istft(torch.stack([X, X]).contiguous(), N)
    want = sp.istft(sp.stft(x, 1024, F64)[:, :, :512], N, 1024)
    assert _rel(got[0].cpu(), want) < 1e-5 and torch.equal(got[0], got[1])


# ------------------------------------------------------------------ the layers, each on the fp32 restatement's own tensors
def _taps(sep, n_units=2, seed=5):
    """per unit, the fp32 restatement's tensors around every layer of instrument 1, from that unit's own magnitudes"""
    key = ("taps", id(sep), n_units, seed)
    if key not in _cache:
        cfg, out = sep.config, []
        for u in range(n_units):
            g = torch.Generator().manual_seed(seed + u)
            M = torch.rand(cfg.T, cfg.F, cfg.n_channels, generator=g) * 2.0
            taps = {}
            sp.unet(M, sep.state, cfg.instruments[1], cfg.bn_eps, F32, taps)
            out.append(taps)
        _cache[key] = out
    return _cache[key]


CASES = [(DEFAULT, 64, 64), (DEFAULT, 128, 64), (ODD, 64, 64), (ODD, 128, 64)]


@pytest.mark.parametrize("filters,T,F", CASES)
def test_encoder_layers(filters, T, F):
    sep = _engine(filters, T=T, F=F)
    cfg, name, taps = sep.config, sep.config.instruments[1], _taps(sep)
    for l in range(1, 7):
        x = torch.stack([t[f"conv{l}"][0] for t in taps])
        pre, act = sep.debug_layer(1, 0, l, x.cuda())
        r32 = [sp.encoder_layer(xu, sep.state, name, l, cfg.bn_eps, F32) for xu in x]
        r64 = [sp.encoder_layer(xu.to(F64), sep.state, name, l, cfg.bn_eps, F64) for xu in x]
        _hold(f"conv{l} pre {filters[0]} {T}x{F}", pre, torch.stack([r[0] for r in r32]), torch.stack([r[0] for r in r64]))
        _hold(f"conv{l} act {filters[0]} {T}x{F}", act, torch.stack([r[1] for r in r32]), torch.stack([r[1] for r in r64]))
    _verdict()


@pytest.mark.parametrize("filters,T,F", CASES)
def test_decoder_layers_read_skip_and_up_from_two_pointers(filters, T, F):
    sep = _engine(filters, T=T, F=F)
    cfg, name, taps = sep.config, sep.config.instruments[1], _taps(sep)
    for j in range(1, 7):
        skip = torch.stack([t[f"deconv{j}"][0] for t in taps])
        up = torch.stack([t[f"deconv{j}"][1] for t in taps]) if j > 1 else None
        got = sep.debug_layer(1, 1, j, skip.cuda(), up.cuda() if j > 1 else None)
        r32 = torch.stack([sp.decoder_layer(skip[u], up[u] if j > 1 else None, sep.state, name, j, cfg.bn_eps, F32) for u in range(len(taps))])
        r64 = torch.stack([sp.decoder_layer(skip[u].to(F64), up[u].to(F64) if j > 1 else None, sep.state, name, j, cfg.bn_eps, F64) for u in range(len(taps))])
        _hold(f"deconv{j} {filters[0]} {T}x{F}", got, r32, r64)
    _verdict()


@pytest.mark.parametrize("filters,T,F", [(DEFAULT, 64, 64), (ODD, 128, 64)])
def test_head(filters, T, F):
    sep = _engine(filters, T=T, F=F)
    name, taps = sep.config.instruments[1], _taps(sep)
    x = torch.stack([t["head"][0] for t in taps])
    got = sep.debug_layer(1, 2, 0, x.cuda())
    _hold(f"head {T}x{F}", got, torch.stack([sp.head_layer(xu, sep.state, name, F32) for xu in x]), torch.stack([sp.head_layer(xu.to(F64), sep.state, name, F64) for xu in x]))
    _verdict()


def test_default_config_bottleneck_layers():
    """the small configs above never reach the default config's 8 x 16 bottleneck: its two layers (K = 6400 and 9 x 512), fp64 included, on random inputs"""
    sep = _engine(DEFAULT, T=512, F=1024, n_fft=4096, instruments=("a",), seed=6)
    cfg = sep.config
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 32, 256, generator=g)
    pre, act = sep.debug_layer(0, 0, 6, x.cuda())
    r32, r64 = sp.encoder_layer(x[0], sep.state, "a", 6, cfg.bn_eps, F32), sp.encoder_layer(x[0].to(F64), sep.state, "a", 6, cfg.bn_eps, F64)
    assert tuple(pre.shape) == (1, 8, 16, 512)
    _hold("conv6 pre default 512x1024", pre[0], r32[0], r64[0])
    _hold("conv6 act default 512x1024", act[0], r32[1], r64[1])
    y = torch.randn(1, 8, 16, 512, generator=g)
    up = sep.debug_layer(0, 1, 1, y.cuda())
    assert tuple(up.shape) == (1, 16, 32, 256)
    _hold("deconv1 default 512x1024", up[0], sp.decoder_layer(y[0], None, sep.state, "a", 1, cfg.bn_eps, F32),
          sp.decoder_layer(y[0].to(F64), None, sep.state, "a", 1, cfg.bn_eps, F64))
    _verdict()


def test_mask_stage_with_a_bin_whose_estimates_are_all_zero():
    sep = _engine(ODD, instruments=("a", "b", "c"))
    cfg = sep.config
    g = torch.Generator().manual_seed(8)
    Tf, segs = 69, 2
    logits = torch.randn(segs, 3, cfg.T, cfg.F, 2, generator=g) * 3.0
    M = torch.rand(segs, cfg.T, cfg.F, 2, generator=g) * 5.0
    M[0, 3, 7] = 0.0                                    # every estimate of this bin is 0: the masks are 1 / 3
    M[1, 2, :, 1] = 0.0
    X = torch.complex(torch.randn(2, Tf, cfg.F, generator=g), torch.randn(2, Tf, cfg.F, generator=g))
    got = sep.debug_mask(logits.cuda(), M.reshape(segs * cfg.T, cfg.F, 2).cuda(), X.cuda())
    y32 = sp.apply_masks(logits, M, X, 2, cfg.mask_eps)
    y64 = sp.apply_masks(logits.to(F64), M.to(F64), X.to(torch.complex128), 2, cfg.mask_eps)
    _hold("mask", got, y32, y64)
    third = X[:, 3, 7] * torch.tensor(1.0 / 3.0)
    assert float((got.cpu()[:, :, 3, 7] - third[None]).abs().max()) <= 4 * 2.0 ** -24 * float(third.abs().max()) * 4
    _verdict()


# ------------------------------------------------------------------ the whole chain
def _chain_engine(**kw):
    return _engine(DEFAULT, instruments=("vocals", "piano", "drums", "bass", "other"), seed=4, **kw)


def _songs():
    if "songs" not in _cache:
        _cache["songs"] = [_audio(64 * 256 + 5, seed=21), _audio(1, seed=22), _audio(5000, channels=1, seed=23)[0]]
    return _cache["songs"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_whole_chain(which):
    sep = _chain_engine()
    x = _songs()[which]
    got = sep.separate_many([x])[0]
    x2 = x if x.ndim == 2 else np.stack([x, x])
    assert got.is_cuda and tuple(got.shape) == (5, 2, x2.shape[1])
    _hold(f"chain song {which}", got, sp.separate(x2, sep.config, sep.state, F32), sp.separate(x2, sep.config, sep.state, F64))
    _verdict()


def test_a_song_is_bit_identical_alone_in_a_batch_under_a_tight_budget_and_again():
    sep, tight = _chain_engine(), _chain_engine(workspace_bytes=1)      # 1 byte: one unit per sub-batch, one stem per inverse-STFT pass
    songs = _songs()
    batch = sep.separate_many(songs)
    again = sep.separate_many(songs[::-1])[::-1]
    small = tight.separate_many(songs)
    mid = _chain_engine(workspace_bytes=2_400_000).separate_many(songs)      # songs 0 and 1 share a group, song 2 follows in the same workspace; 5 units per launch
    for i, x in enumerate(songs):
        alone = sep.separate_many([x])[0]
        assert torch.equal(alone, batch[i]) and torch.equal(alone, again[i]) and torch.equal(alone, small[i]) and torch.equal(alone, mid[i]), i
    d = sep.separate(songs[2])
    assert list(d) == list(sep.config.instruments) and d["drums"].shape == (5000, 2) and d["drums"].dtype == np.float32
    assert np.array_equal(d["drums"], batch[2][2].cpu().numpy().T)


def test_non_finite_audio_is_refused():
    sep = _chain_engine()
    x = _audio(3000, seed=3)
    x[1, 17] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        sep.separate_many([_audio(100), x])


# ------------------------------------------------------------------ from audio to tempo.json
def test_stems_stay_on_the_device_and_structuralize_audio_many_equals_the_stems_path():
    from etude_amd import structuralize_audio_many, structuralize_stems_many
    from etude_amd.beat import BeatDetector
    from etude_amd.stemfeat import StemFeatures
    det = BeatDetector(state_dict=synth.beat_state_dict(20240607), tracker="native")
    sep = _chain_engine()
    wavs = [_audio(44100 * 4 + 77, seed=31), _audio(44100 * 3, seed=32)]
    stems = sep.separate_many(wavs)
    sf = StemFeatures(framing="spleeter")
    for w, s in zip(wavs, stems):
        assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == (5, 2, w.shape[1]) and s.is_contiguous()
    feat, Ts = sf.features_many(stems)                  # device tensors in: nothing is uploaded
    assert feat.is_cuda and Ts == [sf.num_frames(w.shape[1]) for w in wavs]
    got = structuralize_audio_many(det, sep, wavs)
    assert got == structuralize_stems_many(det, stems, stem_features=sf)
    assert len(got) == 2 and all(isinstance(r, list) for r in got)
