"""The separator's contract on the host (tests/separator_np.py): its convolutions against torch.nn.functional with the paddings written out, the
STFT / inverse STFT round trip, "the stems sum to the mixture", and what etude_amd.separator refuses or promises without a GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as tf

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_np as sp  # noqa: E402

from etude_amd import _lib  # noqa: E402
from etude_amd.separator import (SeparatorConfig, StemSeparator, check_separator_state, expected_keys, init_separator_state,  # noqa: E402
                                 load_separator_state)

F64 = torch.float64
SMALL = dict(n_fft=1024, hop=256, T=64, F=64, conv_n_filters=(2, 3, 4, 5, 6, 7), instruments=("a", "b", "c"))


def _nchw(x):
    return x.permute(2, 0, 1)[None]


@pytest.mark.parametrize("shape", [(2, 2), (1, 1), (8, 4)])
def test_transposed_conv_is_conv_transpose2d_cropped_by_one_leading_and_two_trailing(shape):
    g = torch.Generator().manual_seed(3)
    Ci, Co = 3, 4
    x = torch.randn(*shape, Ci, generator=g, dtype=F64)
    w = torch.randn(5, 5, Co, Ci, generator=g, dtype=F64)
    b = torch.randn(Co, generator=g, dtype=F64)
    got = sp.conv_up(x, w, b)
    full = tf.conv_transpose2d(_nchw(x), w.permute(3, 2, 0, 1), b, stride=2)[0]            # [Co][2T + 3][2F + 3]
    want = full[:, 1:full.shape[1] - 2, 1:full.shape[2] - 2].permute(1, 2, 0)
    assert got.shape == want.shape == (2 * shape[0], 2 * shape[1], Co)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 2), (8, 4)])
def test_conv_is_conv2d_stride_2_padded_one_before_and_two_after(shape):
    g = torch.Generator().manual_seed(4)
    Ci, Co = 3, 4
    x = torch.randn(*shape, Ci, generator=g, dtype=F64)
    w = torch.randn(5, 5, Ci, Co, generator=g, dtype=F64)
    b = torch.randn(Co, generator=g, dtype=F64)
    got = sp.conv_down(x, w, b)
    want = tf.conv2d(tf.pad(_nchw(x), (1, 2, 1, 2)), w.permute(3, 2, 0, 1), b, stride=2)[0].permute(1, 2, 0)
    assert got.shape == want.shape == (shape[0] // 2, shape[1] // 2, Co)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 2), (1, 1), (8, 4)])
def test_head_is_conv2d_dilation_2_padded_three(shape):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, 1, generator=g, dtype=F64)
    w = torch.randn(4, 4, 1, 2, generator=g, dtype=F64)
    b = torch.randn(2, generator=g, dtype=F64)
    got = sp.head(x, w, b)
    want = tf.conv2d(tf.pad(_nchw(x), (3, 3, 3, 3)), w.permute(3, 2, 0, 1), b, dilation=2)[0].permute(1, 2, 0)
    assert got.shape == want.shape == (shape[0], shape[1], 2)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("n_fft", [1024, 4096])
def test_stft_then_inverse_with_unit_masks_returns_the_waveform(n_fft):
    hop = n_fft // 4
    for N in (1, hop - 1, hop, n_fft + 1, 3 * n_fft + 17):
        x = torch.from_numpy(np.random.default_rng(N).standard_normal((2, N)))
        X = sp.stft(x, n_fft, F64)
        assert X.shape == (2, 1 + (N + n_fft) // hop, n_fft // 2 + 1)
        y = sp.istft(X, N, n_fft)
        assert float((y - x).abs().max()) <= 1e-12


def test_the_stems_sum_to_the_mixture_below_bin_F():
    cfg = SeparatorConfig(**SMALL)
    state = init_separator_state(cfg, 1)
    N = 64 * 256 + 5                                   # two segments
    x = np.random.default_rng(2).standard_normal((2, N)).astype(np.float32) * 0.3
    stems = sp.separate(x, cfg, state, F64)
    assert stems.shape == (3, 2, N)
    assert sp.num_frames(N, cfg.n_fft) > cfg.T
    want = sp.separate(x, cfg, state, F64, all_pass=True)[0]
    assert float((stems.sum(0) - want).abs().max()) <= 1e-9 * float(want.abs().max())
    assert float((stems[0] - stems[1]).abs().max()) > 1e-6       # (the instruments' masks differ)


def test_masks_where_every_estimate_is_zero_are_uniform():
    lg = torch.randn(3, 4, dtype=F64)
    m = sp.masks(lg, torch.zeros(4, dtype=F64), 2, 1e-10)
    assert float((m - 1 / 3).abs().max()) < 1e-12


@pytest.mark.parametrize("bad", [dict(hop=512), dict(n_fft=512, hop=128), dict(n_fft=8192, hop=2048), dict(n_fft=3000, hop=750), dict(F=1024), dict(T=96),
                                 dict(F=32), dict(conv_n_filters=(2, 3, 0, 5, 6, 7)), dict(instruments=()), dict(conv_n_filters=(2, 3, 4)),
                                 dict(separation_exponent=0), dict(n_channels=0)])
def test_bad_configs_are_refused_without_a_gpu(bad):
    with pytest.raises(ValueError):
        SeparatorConfig(**{**SMALL, **bad}).check()
    with pytest.raises(ValueError):
        StemSeparator(SeparatorConfig(**{**SMALL, **bad}))


def test_the_library_refuses_what_the_config_check_refuses():
    import ctypes as C
    lib = _lib.lib()
    cfg = SeparatorConfig(**SMALL)
    state = init_separator_state(cfg, 0)
    names, ptrs, numels, n, keep = _lib.weights_arrays(state)
    instr = (C.c_char_p * 3)(b"a", b"b", b"c")

    def create(**kw):
        base = dict(n_instr=3, n_channels=2, n_fft=1024, hop=256, T=64, F=64, filters=(C.c_int * 6)(2, 3, 4, 5, 6, 7), separation_exponent=2, mask_eps=1e-10, bn_eps=1e-3,
                    workspace_bytes=0)
        base.update(kw)
        h = C.c_void_p()
        rc = lib.etd_sep_create(C.byref(_lib.SepCfg(**base)), instr, names, ptrs, numels, n, C.byref(h))
        if rc == 0:
            lib.etd_sep_destroy(h)
        return rc

    assert create() == 0
    for kw in (dict(hop=512), dict(n_fft=512, hop=128), dict(F=1024), dict(T=96), dict(filters=(C.c_int * 6)(2, 3, 0, 5, 6, 7)), dict(n_instr=0), dict(mask_eps=0.0),
               dict(separation_exponent=9), dict(workspace_bytes=-1)):
        assert create(**kw) == -22, kw
    # each check by its own message: a filter count of 0 (with weights sized to match, so nothing else can refuse it), a negative one, and T past the int range of a unit
    for filt in ((2, 3, 0, 5, 6, 7), (2, 3, -4, 5, 6, 7), (2, 3, 4, 5, 6, 4097)):
        zcfg = SeparatorConfig(**{**SMALL, "conv_n_filters": tuple(max(f, 0) for f in filt)})
        zstate = {k: np.zeros(shp, np.float32) for k, shp in expected_keys(zcfg).items()}
        names, ptrs, numels, n, keep2 = _lib.weights_arrays(zstate)
        assert create(filters=(C.c_int * 6)(*filt)) == -22
        assert f"filters[{2 if filt[2] < 1 else 5}]" in lib.etd_last_error().decode(), lib.etd_last_error()
    names, ptrs, numels, n, keep = _lib.weights_arrays(state)
    assert create(T=65536 + 64) == -22 and "T = 65600 must be <= 65536" in lib.etd_last_error().decode(), lib.etd_last_error()
    assert create(T=65536) == 0
    assert create(n_fft=4096, hop=1024, F=2048) == 0 and create(n_fft=4096, hop=1024, F=2112) == -22


def test_state_errors_name_the_key():
    cfg = SeparatorConfig(**SMALL)
    state = init_separator_state(cfg, 0)
    check_separator_state(state, cfg)
    assert set(state) == set(expected_keys(cfg))
    assert len(state) == 3 * (6 * 4 + 12 * 4 + 2)
    miss = dict(state)
    del miss["b.deconv3.weight"]
    with pytest.raises(ValueError, match="b.deconv3.weight"):
        StemSeparator(cfg, miss)
    bad = dict(state)
    bad["c.bn12.var"] = np.ones(2, np.float32)
    with pytest.raises(ValueError, match="c.bn12.var"):
        StemSeparator(cfg, bad)
    nan = dict(state)
    nan["a.head.bias"] = np.array([0.0, np.nan], np.float32)
    with pytest.raises(ValueError, match="a.head.bias"):
        StemSeparator(cfg, nan)
    assert state["a.conv1.weight"].shape == (5, 5, 2, 2) and state["a.deconv1.weight"].shape == (5, 5, 6, 7) and state["a.deconv2.weight"].shape == (5, 5, 5, 12)
    assert state["a.deconv6.weight"].shape == (5, 5, 1, 4) and state["a.head.weight"].shape == (4, 4, 1, 2)


def test_init_is_a_function_of_the_seed():
    cfg = SeparatorConfig(**SMALL)
    a, b, c = init_separator_state(cfg, 5), init_separator_state(cfg, 5), init_separator_state(cfg, 6)
    assert all(a[k].dtype == np.float32 and a[k].tobytes() == b[k].tobytes() for k in a)
    assert any(a[k].tobytes() != c[k].tobytes() for k in a)
    w = a["a.conv2.weight"]
    assert float(np.abs(w).max()) <= np.sqrt(6.0 / (25 * 2)) and not a["a.conv2.bias"].any()
    assert 0.5 <= float(a["a.bn3.gamma"].min()) and float(a["a.bn3.var"].max()) <= 1.5


def test_save_and_load_round_trip(tmp_path):
    cfg = SeparatorConfig(**SMALL)
    sep = StemSeparator(cfg, seed=9)                   # (constructing needs no GPU)
    sep.save(tmp_path / "sep.pt")
    back = load_separator_state(tmp_path / "sep.pt")
    assert set(back) == set(sep.state) and all(back[k].tobytes() == sep.state[k].tobytes() for k in back)
    assert sep.num_frames(1) == 5 and sep.num_frames(256 * 7) == 1 + (256 * 7 + 1024) // 256
    assert sep.unit_bytes > 0 and sep.workspace_total_bytes([1000, 20000]) > sep.unit_bytes


def test_the_budget_bounds_what_a_call_holds_whatever_the_batch():
    cfg = SeparatorConfig(**SMALL)
    state = init_separator_state(cfg, 0)
    B = 8 << 20
    sep, free = StemSeparator(cfg, state, workspace_bytes=B), StemSeparator(cfg, state, workspace_bytes=1 << 40)
    one = free.workspace_total_bytes([20000])
    assert one < B // 2
    for n in (1, 7, 40):
        held = sep.workspace_total_bytes([20000] * n)
        assert held <= B + 5 * 256, (n, held)              # (five 256-byte roundings)
    assert free.workspace_total_bytes([20000] * 40) > 4 * B        # ... which the same batch exceeds without it
    tight = StemSeparator(cfg, state, workspace_bytes=1)
    assert tight.workspace_total_bytes([20000] * 40) == tight.workspace_total_bytes([20000]) < one


def test_input_errors_come_before_the_device():
    sep = StemSeparator(SeparatorConfig(**SMALL), seed=0)
    for bad in (np.zeros((3, 100), np.float32), np.zeros((2, 0), np.float32), np.zeros((2, 2, 5), np.float32)):
        with pytest.raises(ValueError):
            sep.separate_many([bad])


def test_symbols_exported():
    lib = _lib.lib()
    for name in ("etd_sep_create", "etd_sep_destroy", "etd_sep_num_frames", "etd_sep_unit_bytes", "etd_sep_workspace_bytes", "etd_sep_run", "etd_sep_segment_flops",
                 "etd_sep_debug_stft", "etd_sep_debug_layer", "etd_sep_debug_mask", "etd_sep_debug_istft"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.etd_version() == 3
    import etude_amd
    for name in ("StemSeparator", "SeparatorConfig", "init_separator_state", "load_separator_state", "structuralize_audio_many"):
        assert name in etude_amd.__all__ and getattr(etude_amd, name) is not None
    from etude_amd.beat import BeatDetector
    assert callable(BeatDetector.detect_audio_many)
