"""Separator training without a GPU: the restatement (tests/separator_train_np.py) against finite differences, against separator_np in frozen mode and against
torch.optim.Adam; the mistakes it must be able to see; and what ``SeparatorTrainer`` refuses and packs before any device is touched."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_np as sp  # noqa: E402
import separator_train_np as st  # noqa: E402

from etude_amd import _lib  # noqa: E402
from etude_amd.separator import SeparatorConfig, expected_keys, init_separator_state  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer  # noqa: E402

F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
_cache = {}


def _tiny(B=2, filters=(2, 2, 3, 2, 2, 2), instruments=("a", "b"), C=1):
    key = (B, filters, instruments, C)
    if key not in _cache:
        cfg = SeparatorConfig(instruments=instruments, n_fft=1024, hop=256, T=64, F=64, n_channels=C, conv_n_filters=filters)
        state = init_separator_state(cfg, 11)
        for k in state:                                 # biases off zero, so that nothing about them passes by symmetry
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
        _cache["truth"] = (st.loss_and_grads(mix, target, state, cfg, F64), st.loss_and_grads(mix, target, state, cfg, F32))
    return _cache["truth"]


def _err(g, g64):
    return float((g.to(F64) - g64).abs().max()) / float(g64.abs().max())


def test_fp64_gradients_agree_with_central_finite_differences():
    """One entry (the one of largest gradient) of twelve tensors of every kind, central differences with h = 1e-6 on the fp64 loss.  The loss is O(1) and piecewise
    smooth: the truncation term is O(h^2) = 1e-12, the rounding term eps64 L / h = 2e-10, and a residual that changes sign inside +-h (a kink of |.|) moves the
    quotient by at most its own share 1 / (I B T F C) = 6e-5 of the gradient's scale times the fraction of the step it spends past the kink.  Bound: 1e-6 of the
    tensor's largest gradient entry; measured: at most 4.2e-7 (b.bn3.beta)."""
    cfg, state, mix, target = _tiny()
    (L, g64, _), _ = _truth()
    h, worst = 1e-6, 0.0
    for k in ("a.conv1.weight", "b.conv3.weight", "a.conv6.bias", "b.deconv1.weight", "a.deconv4.weight", "b.deconv6.bias", "a.bn2.gamma", "b.bn3.beta",
              "a.bn9.gamma", "b.bn12.beta", "a.head.weight", "b.head.bias"):
        idx = int(g64[k].abs().argmax())
        vals = []
        for sgn in (1.0, -1.0):
            P = st.params(state, F64, requires_grad=False)
            P[k].view(-1)[idx] += sgn * h
            vals.append(float(st.loss_fn(st.forward(mix.to(F64), P, cfg), mix.to(F64), target.to(F64))))
        fd, an = (vals[0] - vals[1]) / (2 * h), float(g64[k].view(-1)[idx])
        rel = abs(fd - an) / float(g64[k].abs().max())
        print(f"FD {k}[{idx}]: autograd {an:.9e} differences {fd:.9e} rel {rel:.2e}")
        worst = max(worst, rel)
        assert rel <= 1e-6, (k, fd, an)
    print(f"FD worst {worst:.2e}")


@pytest.mark.parametrize("variant", ["one_unit", "unbiased", "no_skip_grad", "no_coupling", "norm_by_B"])
def test_each_wrong_variant_moves_the_gradient_far_past_the_bound(variant):
    cfg, state, mix, target = _tiny()
    (_, g64, _), (_, g32, _) = _truth()
    _, gv, _ = st.loss_and_grads(mix, target, state, cfg, F64, variant=variant)
    worst_v = max(_err(gv[k], g64[k]) for k in g64 if float(g64[k].abs().max()) > 0)
    bound = max(max(4.0 * _err(g32[k], g64[k]), FLOOR) for k in g64 if float(g64[k].abs().max()) > 0)
    print(f"variant {variant}: moves a gradient by {worst_v:.3e}, the widest bound is {bound:.3e}")
    assert worst_v > 100.0 * bound


def test_unused_norm_has_zero_gradient_and_every_other_tensor_a_live_one():
    (_, g64, stats), _ = _truth()
    for k, g in g64.items():
        if ".bn6." in k:
            assert float(g.abs().max()) == 0.0, k      # conv_6's normalised output is read by nothing
        else:
            assert float(g.abs().max()) > 0.0, k
    assert set(stats) == {f"{n}.bn{i}" for n in ("a", "b") for i in range(1, 13)}


def test_frozen_statistics_equal_the_inference_unet():
    """training mode on the running statistics is separator_np.unet: the two differ only by where the norm's affine is rounded (bn_affine folds it to float32 once),
    2^-24 per norm through twelve norms.  Bound 1e-5 of the largest logit; measured 4.2e-8."""
    cfg, state, mix, _ = _tiny()
    P = st.params(state, F64, requires_grad=False)
    got = st.forward(mix.to(F64), P, cfg, frozen=True)
    want = torch.stack([torch.stack([sp.unet(mix[b], state, name, cfg.bn_eps, F64) for b in range(mix.shape[0])]) for name in cfg.instruments])
    e = _err(got, want)
    print(f"frozen vs separator_np.unet: {e:.3e}")
    assert e <= 1e-5


def test_batched_convolutions_equal_separator_np():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 6, 3, generator=g, dtype=F64)
    w, b = torch.randn(5, 5, 3, 4, generator=g, dtype=F64), torch.randn(4, generator=g, dtype=F64)
    wu = torch.randn(5, 5, 4, 3, generator=g, dtype=F64)
    wh = torch.randn(4, 4, 3, 2, generator=g, dtype=F64)
    for u in range(2):
        assert torch.allclose(st.conv_down(x, w, b)[u], sp.conv_down(x[u], w, b), rtol=0, atol=1e-12)
        assert torch.allclose(st.conv_up(x, wu, b)[u], sp.conv_up(x[u], wu, b), rtol=0, atol=1e-12)
        assert torch.allclose(st.head(x, wh, b[:2])[u], sp.head(x[u], wh, b[:2]), rtol=0, atol=1e-12)


def test_adam_restated_equals_torch_optim_adam_bit_for_bit():
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(257, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=3e-3, betas=(0.9, 0.98), eps=1e-8, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 8):
        grad = torch.randn(257, generator=g) * (10.0 ** (step % 3 - 1))
        ref.grad = grad.clone()
        opt.step()
        p, m, v = st.adam_step(p, grad, m, v, step, 3e-3, (0.9, 0.98), 1e-8)
        assert torch.equal(p, ref.detach()), step
    s = opt.state[ref]
    assert torch.equal(m, s["exp_avg"]) and torch.equal(v, s["exp_avg_sq"])


def test_running_statistics_update():
    r, b = torch.tensor([1.0, -2.0, 0.5]), torch.tensor([3.0, 0.0, 0.5])
    got = st.running_update(r, b)
    assert got.dtype == F32 and torch.allclose(got, 0.99 * r + 0.01 * b, rtol=1e-6) and float(got[2]) == pytest.approx(0.5, abs=1e-7)


# ------------------------------------------------------------------ the engine's host side
def test_state_dict_keys_and_packing_round_trip_without_a_device():
    cfg, state, _, _ = _tiny(filters=(3, 5, 8, 16, 24, 40), instruments=("x", "y", "z"), C=2)
    tr = SeparatorTrainer(cfg, state, max_units=3)
    sd = tr.state_dict()
    assert list(sd) == list(expected_keys(cfg))
    for k, v in state.items():
        assert sd[k].shape == v.shape and np.array_equal(sd[k], v), k
    assert set(tr.grads()) == {k for k in expected_keys(cfg) if not k.endswith((".mean", ".var"))}
    assert tr.workspace_total_bytes(3) > tr.workspace_total_bytes(1) > 0 and tr.step_flops(2) == 2 * tr.step_flops(1) > 0
    tr.close()


def test_config_state_and_input_refusals():
    cfg, state, mix, target = _tiny()
    with pytest.raises(ValueError, match="multiples of 64"):
        SeparatorTrainer(SeparatorConfig(instruments=("a",), n_fft=1024, hop=256, T=96, F=64))
    with pytest.raises(ValueError, match="max_units"):
        SeparatorTrainer(cfg, state, max_units=0)
    with pytest.raises(ValueError, match="max_units"):
        SeparatorTrainer(cfg, state, max_units=10000)
    with pytest.raises(ValueError, match="workspace_bytes"):
        SeparatorTrainer(cfg, state, workspace_bytes=0)
    with pytest.raises(ValueError, match="betas"):
        SeparatorTrainer(cfg, state, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="missing key 'b.bn7.var'"):
        SeparatorTrainer(cfg, {k: v for k, v in state.items() if k != "b.bn7.var"})
    bad = dict(state)
    bad["a.conv2.weight"] = np.full_like(state["a.conv2.weight"], np.nan)
    with pytest.raises(ValueError, match="non-finite"):
        SeparatorTrainer(cfg, bad)
    tr = SeparatorTrainer(cfg, state, max_units=2)
    with pytest.raises(ValueError, match=r"mix must be \[B\]\[T\]\[F\]\[C\]"):
        tr.loss_and_backward(mix[:, :32], target)
    with pytest.raises(ValueError, match="target must be"):
        tr.loss_and_backward(mix, target[:1])
    with pytest.raises(ValueError, match="max_units is 2"):
        tr.loss_and_backward(torch.cat([mix, mix]), torch.cat([target, target], 1))
    tr.close()


# ------------------------------------------------------------------ the parameter store, before any device call (reads are answered from the host's copy)
def _store_call(tr, entry, *args):
    _lib.check(getattr(_lib.lib(), entry)(tr.h, *args), entry)


def _store_refusal(tr, match, entry, *args):
    with pytest.raises(_lib.EtudeHipError, match=match):
        _store_call(tr, entry, *args)


def test_store_reads_return_the_state_and_zeros_without_a_device():
    cfg, state, _, _ = _tiny()
    tr = SeparatorTrainer(cfg, state, max_units=2)
    sd = tr._read(0, tr._shapes)
    assert list(sd) == list(expected_keys(cfg)) and all(np.array_equal(sd[k], state[k]) for k in sd)
    trainable = [k for k in expected_keys(cfg) if not k.endswith((".mean", ".var"))]
    for which in (1, 2, 3):
        got = tr._read(which, trainable)
        assert list(got) == trainable and all(v.shape == state[k].shape and not v.any() for k, v in got.items()), which
    tr.close()


def test_store_refusals_name_the_key_the_counts_and_the_buffer():
    cfg, state, _, _ = _tiny()
    tr = SeparatorTrainer(cfg, state, max_units=2)
    n = state["a.conv1.weight"].size
    buf = np.zeros(n + 1, np.float32)
    _store_refusal(tr, r"etd_septrain: no tensor 'a\.conv9\.weight'", "etd_septrain_read", b"a.conv9.weight", 0, buf.ctypes.data, n, None)
    _store_refusal(tr, rf"etd_septrain: 'a\.conv1\.weight' has {n} elements, the buffer {n + 1}", "etd_septrain_read", b"a.conv1.weight", 0, buf.ctypes.data, n + 1, None)
    for which in (-1, 4):
        _store_refusal(tr, rf"etd_septrain: which = {which} is not 0 \.\. 3", "etd_septrain_read", b"a.conv1.weight", which, buf.ctypes.data, n, None)
    for key in ("b.bn7.mean", "a.bn1.var"):
        m = state[key].size
        for which in (1, 2, 3):
            _store_refusal(tr, rf"etd_septrain: '{key}' is a running statistic", "etd_septrain_read", key.encode(), which, buf.ctypes.data, m, None)
        got = np.empty(m, np.float32)
        _store_call(tr, "etd_septrain_read", key.encode(), 0, got.ctypes.data, m, None)
        assert np.array_equal(got, state[key].reshape(-1))
    _store_refusal(tr, "septrain_read: null buffer", "etd_septrain_read", b"a.conv1.weight", 0, None, n, None)
    tr.close()


def test_step_counter_follows_set_step_and_refuses_a_negative_one():
    cfg, state, _, _ = _tiny()
    tr = SeparatorTrainer(cfg, state, max_units=2)
    lib = _lib.lib()
    assert lib.etd_septrain_get_step(tr.h) == 0
    for s in (7, 0, 2 ** 40):
        _store_call(tr, "etd_septrain_set_step", s)
        assert lib.etd_septrain_get_step(tr.h) == s
    _store_refusal(tr, "septrain_set_step: null handle or negative step", "etd_septrain_set_step", -1)
    assert lib.etd_septrain_get_step(tr.h) == 2 ** 40
    assert lib.etd_septrain_set_step(None, 1) == -22 and lib.etd_septrain_get_step(None) == -22
    tr.close()
