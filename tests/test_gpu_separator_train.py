"""Separator training on the MI355X (csrc/separator_train.hip, etude_amd.SeparatorTrainer) against the restatement of DESIGN.md 4n (tests/separator_train_np.py):
every backward kernel on its own tapped input, the whole gradient, accumulation, determinism, an Adam trajectory, the hand-over to StemSeparator, a direction check
and the refusals.

The yardstick is tests/test_gpu_separator.py's: ``err = max|g - g64| / max|g64|`` per tensor against fp64 (autograd of the restatement), held to 4 x the same figure of
fp32 torch-CPU autograd on the same input, with a floor of 4 * 2^-24.  Units are [B][I] on the device: unit (b, i) runs with instrument i's weights."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import separator_np as sp  # noqa: E402
import separator_train_np as st  # noqa: E402

from etude_amd import _lib, synth  # noqa: E402
from etude_amd.separator import SeparatorConfig, init_separator_state, load_separator_state  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer, training_segments  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FLOOR = 4.0 * 2.0 ** -24
DEFAULT = (16, 32, 64, 128, 256, 512)
ODD = (3, 5, 8, 16, 24, 40)
# (filters, T, F, instruments, B, channels): the four shapes of test_gpu_separator.py; between them B = 1, 2, 3, I = 1, 2, 3, C = 1, 2
CASES = [(DEFAULT, 64, 64, 2, 2, 2), (DEFAULT, 128, 64, 1, 3, 2), (ODD, 64, 64, 3, 1, 1), (ODD, 128, 64, 2, 3, 2)]
_cache = {}
_bad = []


def _rel(y, y64):
    y, y64 = torch.as_tensor(y), torch.as_tensor(y64)
    return float((y.to(F64) - y64.to(F64)).abs().max()) / float(y64.abs().max())


def _hold(what, dev, y32, y64):
    dev = torch.as_tensor(dev).cpu()
    assert tuple(dev.shape) == tuple(y64.shape), (what, tuple(dev.shape), tuple(y64.shape))
    assert bool(torch.isfinite(dev).all()), what
    if float(y64.abs().max()) == 0.0:                   # a tensor the loss does not depend on: exact zeros
        assert float(dev.abs().max()) == 0.0, what
        return
    e_dev, e_32 = _rel(dev, y64), _rel(y32, y64)
    print(f"SEPTRAIN_ERR {what}: device {e_dev:.3e} yardstick {e_32:.3e} ratio {e_dev / max(e_32, 2.0 ** -24):.2f}")
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


def _case(filters, T, F, I, B, Cn, seed=3):
    """config, state (biases off zero), a batch and its fp64 / fp32 losses, gradients and batch statistics -- computed once"""
    key = ("case", filters, T, F, I, B, Cn, seed)
    if key not in _cache:
        cfg = SeparatorConfig(instruments=tuple("abc"[:I]), n_fft=1024, hop=256, T=T, F=F, n_channels=Cn, conv_n_filters=filters)
        state = init_separator_state(cfg, seed)
        r = np.random.default_rng(seed)
        for k in state:
            if k.endswith(".bias"):
                state[k] = r.normal(0, 0.1, state[k].shape).astype(np.float32)
        g = torch.Generator().manual_seed(seed)
        mix = torch.rand(B, T, F, Cn, generator=g) * 2.0
        target = torch.rand(I, B, T, F, Cn, generator=g) * mix[None]
        _cache[key] = dict(cfg=cfg, state=state, mix=mix, target=target, r64=st.loss_and_grads(mix, target, state, cfg, F64),
                           r32=st.loss_and_grads(mix, target, state, cfg, F32))
    return _cache[key]


def _trainer(c, **kw):
    kw.setdefault("max_units", 4)
    return SeparatorTrainer(c["cfg"], c["state"], **kw)


# ------------------------------------------------------------------ the whole gradient
@pytest.mark.parametrize("filters,T,F,I,B,Cn", CASES)
def test_whole_gradient_and_loss(filters, T, F, I, B, Cn):
    c = _case(filters, T, F, I, B, Cn)
    tr = _trainer(c)
    loss = tr.loss_and_backward(c["mix"], c["target"])
    (L64, g64, s64), (L32, g32, s32) = c["r64"], c["r32"]
    tag = f"{filters[0]} {T}x{F} I={I} B={B}"
    print(f"SEPTRAIN_LOSS {tag}: device {loss:.9e} fp64 {float(L64):.9e} fp32 {float(L32):.9e}")
    assert abs(loss - float(L64)) <= max(4.0 * abs(float(L32) - float(L64)), FLOOR * abs(float(L64)))
    got = tr.grads()
    assert list(got) == list(g64)
    for k in g64:
        _hold(f"grad {k} {tag}", got[k], g32[k], g64[k])
    sd = tr.state_dict()                                # one call moved the running statistics once
    for key, (mean, var) in s64.items():
        for part, b64, b32 in (("mean", mean, s32[key][0]), ("var", var, s32[key][1])):
            r0 = torch.from_numpy(c["state"][f"{key}.{part}"])
            _hold(f"running {key}.{part} {tag}", sd[f"{key}.{part}"], st.running_update(r0, b32), st.running_update(r0.to(F64), b64))
    tr.close()
    _verdict()


def test_accumulation_and_zero_grad():
    c = _case(ODD, 64, 64, 3, 1, 1)
    c2 = _case(ODD, 64, 64, 3, 1, 1, seed=4)
    tr = _trainer(c)
    tr.loss_and_backward(c["mix"], c["target"], loss_scale=0.5)
    tr.loss_and_backward(c2["mix"], c2["target"], loss_scale=0.5)
    got = tr.grads()
    ga64, gb64 = c["r64"][1], st.loss_and_grads(c2["mix"], c2["target"], c["state"], c["cfg"], F64)[1]
    ga32, gb32 = c["r32"][1], st.loss_and_grads(c2["mix"], c2["target"], c["state"], c["cfg"], F32)[1]
    for k in ga64:
        _hold(f"accumulated {k}", got[k], 0.5 * ga32[k] + 0.5 * gb32[k], 0.5 * ga64[k] + 0.5 * gb64[k])
    tr.zero_grad()
    assert all(not v.any() for v in tr.grads().values())
    tr.close()
    _verdict()


def test_the_same_call_gives_the_same_bits():
    c = _case(ODD, 128, 64, 2, 3, 2)
    out = []
    for _ in range(2):
        tr = _trainer(c, lr=1e-3)
        loss = tr.loss_and_backward(c["mix"], c["target"])
        grads = tr.grads()
        tr.step()
        out.append((loss, grads, tr.state_dict()))
        tr.close()
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    for k in out[0][2]:
        assert np.array_equal(out[0][2][k], out[1][2][k]), k
    assert any(not np.array_equal(out[0][2][k], c["state"][k]) for k in c["state"])


def test_adam_trajectory_of_five_steps():
    c = _case(ODD, 64, 64, 2, 2, 2)
    lr = 1e-3
    if "traj" not in _cache:
        _cache["traj"] = (st.train_steps(c["mix"], c["target"], c["state"], c["cfg"], F64, 5, lr), st.train_steps(c["mix"], c["target"], c["state"], c["cfg"], F32, 5, lr))
    (l64, s64), (l32, s32) = _cache["traj"]
    tr = _trainer(c, lr=lr)
    for s in range(5):
        loss = tr.train_step(c["mix"], c["target"])
        d_dev, d_32 = abs(loss - l64[s]), abs(l32[s] - l64[s])
        print(f"SEPTRAIN_TRAJ step {s}: device {loss:.9e} fp64 {l64[s]:.9e} fp32 {l32[s]:.9e} deviation {d_dev:.3e} yardstick {d_32:.3e}")
        if not d_dev <= max(4.0 * d_32, FLOOR * abs(l64[s])):
            _bad.append((f"loss at step {s}", d_dev, d_32))
    sd = tr.state_dict()
    for k in sd:
        if k.endswith((".mean", ".var")):
            _hold(f"trajectory {k}", sd[k], s32[k], s64[k])
    osd = tr.optimizer_state_dict()
    assert osd["step"] == 5 and set(osd["exp_avg"]) == set(tr.grads())
    tr2 = _trainer(c, lr=lr)
    tr2.load_optimizer_state_dict(osd)
    back = tr2.optimizer_state_dict()
    assert back["step"] == 5 and all(np.array_equal(back["exp_avg_sq"][k], osd["exp_avg_sq"][k]) for k in osd["exp_avg_sq"])
    tr.close(); tr2.close()
    _verdict()


# (filters, T, F, instruments, B): the MFMA path with K = 600 and N = 40 inside one 64-column tile and M = 2 below one tile; K = 50 < SEP_MFMA_MIN_K, the VALU path;
# 16 x 8 = 128 output positions and N = 72: two M tiles and two N tiles, the second N tile ragged
SHARED_CONV_CASES = [((3, 5, 8, 16, 24, 40), 128, 64, 2, 3), ((3, 5, 8, 16, 2, 40), 128, 64, 2, 3), ((3, 5, 8, 16, 24, 72), 1024, 512, 1, 1)]


@pytest.mark.parametrize("filters,T,F,I,B", SHARED_CONV_CASES)
def test_the_trainer_and_the_separator_convolve_alike(filters, T, F, I, B):
    """the input gradient of transposed convolution 1 is the GEMM of encoder convolution 6 -- a 5 x 5 stride-2 convolution of dy with deconv1.weight [5][5][Cout][Cin]
    read as [K][N]: with conv6.weight holding deconv1.weight's flat contents and no bias, the trainer's dskip and the separator's pre-norm output are the same bits"""
    cfg = SeparatorConfig(instruments=tuple("abc"[:I]), n_fft=1024, hop=256, T=T, F=F, n_channels=2, conv_n_filters=filters)
    state = init_separator_state(cfg, 5)
    for n in cfg.instruments:
        state[f"{n}.conv6.weight"] = state[f"{n}.deconv1.weight"].reshape(state[f"{n}.conv6.weight"].shape).copy()
        state[f"{n}.conv6.bias"] = np.zeros_like(state[f"{n}.conv6.bias"])
    tr = SeparatorTrainer(cfg, state, max_units=4)
    sep = tr.to_separator()
    dy = torch.randn(B, I, T >> 5, F >> 5, filters[4], generator=torch.Generator().manual_seed(37)).cuda()
    dskip, dup = tr.debug_dx(1, 1, dy)
    assert dup is None and tuple(dskip.shape) == (B, I, T >> 6, F >> 6, filters[5])
    for i in range(I):
        pre, _ = sep.debug_layer(i, 0, 6, dy[:, i])
        assert np.array_equal(dskip[:, i].cpu().numpy(), pre.cpu().numpy()), i
    assert bool(dskip.any())
    tr.close()


# ------------------------------------------------------------------ stage by stage
def _taps(c):
    """the fp32 restatement's tensors around every layer, [B][I][..] as the device holds them"""
    key = ("taps", id(c))
    if key not in _cache:
        P = st.params(c["state"], F32, requires_grad=False)
        per = []
        for name in c["cfg"].instruments:
            t = {}
            st.unet_train(c["mix"], P, name, c["cfg"].bn_eps, taps=t)
            per.append(t)
        _cache[key] = per
    return _cache[key]


def _stack(per, layer, idx):
    return torch.stack([t[layer][idx] for t in per], dim=1).contiguous()


def _grads_of(fn, inputs, dy, dtype):
    xs = [x.to(dtype).clone().requires_grad_(True) for x in inputs]
    return torch.autograd.grad(fn(*xs), xs, dy.to(dtype))


STAGE_CASES = [(DEFAULT, 64, 64, 2, 2, 2), (ODD, 128, 64, 2, 3, 2)]


@pytest.mark.parametrize("filters,T,F,I,B,Cn", STAGE_CASES)
def test_input_gradients_of_every_convolution(filters, T, F, I, B, Cn):
    c = _case(filters, T, F, I, B, Cn)
    tr, per, names = _trainer(c), _taps(c), c["cfg"].instruments
    W = lambda k, dt: torch.from_numpy(c["state"][k]).to(dt)      # noqa: E731
    g = torch.Generator().manual_seed(17)
    tag = f"{filters[0]} {T}x{F}"
    for l in range(2, 7):
        x, pre = _stack(per, f"conv{l}", 0), _stack(per, f"conv{l}", 1)
        dy = torch.randn(pre.shape, generator=g)
        got = tr.debug_dx(0, l, dy.cuda())
        r = [[_grads_of(lambda a: st.conv_down(a, W(f"{n}.conv{l}.weight", dt), W(f"{n}.conv{l}.bias", dt)), [x[:, i]], dy[:, i], dt)[0] for i, n in enumerate(names)]
             for dt in (F32, F64)]
        _hold(f"conv{l} dX {tag}", got, torch.stack(r[0], 1), torch.stack(r[1], 1))
    for j in range(1, 7):
        skip, v = _stack(per, f"deconv{j}", 0), _stack(per, f"deconv{j}", 2)
        up = _stack(per, f"deconv{j}", 1) if j > 1 else None
        dy = torch.randn(v.shape, generator=g)
        dskip, dup = tr.debug_dx(1, j, dy.cuda())
        res = {}
        for dt in (F32, F64):
            rows = []
            for i, n in enumerate(names):
                w, b = W(f"{n}.deconv{j}.weight", dt), W(f"{n}.deconv{j}.bias", dt)
                if j > 1:
                    rows.append(_grads_of(lambda a, u: st.conv_up(torch.cat([a, u], -1), w, b), [skip[:, i], up[:, i]], dy[:, i], dt))
                else:
                    rows.append(_grads_of(lambda a: st.conv_up(a, w, b), [skip[:, i]], dy[:, i], dt))
            res[dt] = [torch.stack([r[k] for r in rows], 1) for k in range(2 if j > 1 else 1)]
        _hold(f"deconv{j} dX skip {tag}", dskip, res[F32][0], res[F64][0])
        if j > 1:
            _hold(f"deconv{j} dX up {tag}", dup, res[F32][1], res[F64][1])
    x, lg = _stack(per, "head", 0), _stack(per, "head", 1)
    dy = torch.randn(lg.shape, generator=g)
    got = tr.debug_dx(2, 0, dy.cuda())
    r = [[_grads_of(lambda a: st.head(a, W(f"{n}.head.weight", dt), W(f"{n}.head.bias", dt)), [x[:, i]], dy[:, i], dt)[0] for i, n in enumerate(names)] for dt in (F32, F64)]
    _hold(f"head dX {tag}", got, torch.stack(r[0], 1), torch.stack(r[1], 1))
    tr.close()
    _verdict()


@pytest.mark.parametrize("filters,T,F,I,B,Cn", STAGE_CASES)
def test_weight_gradients_of_every_layer_kind(filters, T, F, I, B, Cn):
    """K = B x positions runs from 3 (the ODD case's 2 x 1 ... 1 x 1 bottleneck with B = 3: below a K tile of 32) over 6144 (conv1 at 128 x 64: one and a half slices
    of 4096) to 24576 (the head); Cout below, at and above the 64-wide tile"""
    c = _case(filters, T, F, I, B, Cn)
    tr, per, names = _trainer(c), _taps(c), c["cfg"].instruments
    W = lambda k, dt: torch.from_numpy(c["state"][k]).to(dt)      # noqa: E731
    g = torch.Generator().manual_seed(19)
    tag = f"{filters[0]} {T}x{F}"
    for l in range(1, 7):
        x, pre = _stack(per, f"conv{l}", 0), _stack(per, f"conv{l}", 1)
        dy = torch.randn(pre.shape, generator=g)
        got = tr.debug_dw(0, l, (c["mix"] if l == 1 else x).cuda(), None, dy.cuda())
        r = [[_grads_of(lambda w: st.conv_down(x[:, i].to(dt), w, W(f"{n}.conv{l}.bias", dt)), [W(f"{n}.conv{l}.weight", dt)], dy[:, i], dt)[0] for i, n in enumerate(names)]
             for dt in (F32, F64)]
        _hold(f"conv{l} dW {tag}", got, torch.stack(r[0]), torch.stack(r[1]))
    for j in range(1, 7):
        skip, v = _stack(per, f"deconv{j}", 0), _stack(per, f"deconv{j}", 2)
        up = _stack(per, f"deconv{j}", 1) if j > 1 else None
        dy = torch.randn(v.shape, generator=g)
        got = tr.debug_dw(1, j, skip.cuda(), up.cuda() if j > 1 else None, dy.cuda())
        xin = torch.cat([skip, up], -1) if j > 1 else skip
        r = [[_grads_of(lambda w: st.conv_up(xin[:, i].to(dt), w, W(f"{n}.deconv{j}.bias", dt)), [W(f"{n}.deconv{j}.weight", dt)], dy[:, i], dt)[0]
              for i, n in enumerate(names)] for dt in (F32, F64)]
        _hold(f"deconv{j} dW {tag}", got, torch.stack(r[0]), torch.stack(r[1]))
    x, lg = _stack(per, "head", 0), _stack(per, "head", 1)
    dy = torch.randn(lg.shape, generator=g)
    got = tr.debug_dw(2, 0, x.cuda(), None, dy.cuda())
    r = [[_grads_of(lambda w: st.head(x[:, i].to(dt), w, W(f"{n}.head.bias", dt)), [W(f"{n}.head.weight", dt)], dy[:, i], dt)[0] for i, n in enumerate(names)]
         for dt in (F32, F64)]
    _hold(f"head dW {tag}", got, torch.stack(r[0]), torch.stack(r[1]))
    tr.close()
    _verdict()


@pytest.mark.parametrize("filters,T,F,I,B,Cn", STAGE_CASES)
def test_norm_statistics_elu_and_their_backward(filters, T, F, I, B, Cn):
    c = _case(filters, T, F, I, B, Cn)
    tr, per, names, eps = _trainer(c), _taps(c), c["cfg"].instruments, c["cfg"].bn_eps
    g = torch.Generator().manual_seed(23)
    tag = f"{filters[0]} {T}x{F}"
    for n in (1, 3, 5, 7, 9, 12):
        dec = n > 6
        x = _stack(per, f"deconv{n - 6}", 2) if dec else _stack(per, f"conv{n}", 1)
        dy = torch.randn(x.shape, generator=g)
        tr.zero_grad()
        y, stats, dx = tr.debug_norm(n, x.cuda(), dy.cuda())
        res = {}
        for dt in (F32, F64):
            rows = []
            for i, name in enumerate(names):
                P = st.params({k: v for k, v in c["state"].items() if k.startswith(f"{name}.bn{n}.")}, dt)
                xi = x[:, i].to(dt).clone().requires_grad_(True)
                s = {}
                out = st.norm(sp.elu(xi), P, f"{name}.bn{n}", eps, False, s) if dec else sp.elu(st.norm(xi, P, f"{name}.bn{n}", eps, False, s))
                gx, gg, gb = torch.autograd.grad(out, [xi, P[f"{name}.bn{n}.gamma"], P[f"{name}.bn{n}.beta"]], dy[:, i].to(dt))
                rows.append((out.detach(), gx, gg, gb) + s[f"{name}.bn{n}"])
            res[dt] = rows
        col = lambda dt, k, dim: torch.stack([r[k] for r in res[dt]], dim)      # noqa: E731
        _hold(f"norm{n} y {tag}", y, col(F32, 0, 1), col(F64, 0, 1))
        _hold(f"norm{n} dx {tag}", dx, col(F32, 1, 1), col(F64, 1, 1))
        _hold(f"norm{n} mean {tag}", stats[0], col(F32, 4, 0), col(F64, 4, 0))
        _hold(f"norm{n} var {tag}", stats[1], col(F32, 5, 0), col(F64, 5, 0))
        gr = tr.grads()
        for i, name in enumerate(names):
            _hold(f"norm{n} dgamma {name} {tag}", gr[f"{name}.bn{n}.gamma"], res[F32][i][2], res[F64][i][2])
            _hold(f"norm{n} dbeta {name} {tag}", gr[f"{name}.bn{n}.beta"], res[F32][i][3], res[F64][i][3])
    tr.close()
    _verdict()


def test_loss_and_dlogits_with_a_silent_bin_and_an_exact_bin():
    c = _case(ODD, 64, 64, 3, 1, 1)
    c2 = _case(ODD, 128, 64, 2, 3, 2)
    for cc in (c, c2):
        cfg = cc["cfg"]
        I, B = len(cfg.instruments), cc["mix"].shape[0]
        g = torch.Generator().manual_seed(29)
        logits = torch.randn(B, I, cfg.T, cfg.F, cfg.n_channels, generator=g) * 3.0
        mix, target = cc["mix"].clone(), cc["target"].clone()
        mix[0, 3, 7] = 0.0                               # a silent bin: every estimate is 0
        target[:, 0, 3, 7] = 0.0                         # ... and so is the truth there: the residual is exactly 0, the subgradient 0
        logits[0, :, 5, 9] = 0.0                         # equal logits: s_i = 1 / I exactly (I = 2) ...
        mix[0, 5, 9] = 1.0
        target[:, 0, 5, 9] = 1.0 / I                     # ... and s_i mix == target_i exactly for I = 2 (for I = 3 a residual of an ulp: still a live bin)
        tr = _trainer(cc)
        loss, d = tr.debug_loss(logits.cuda(), mix.cuda(), target.cuda(), loss_scale=0.5)
        res = {}
        for dt in (F32, F64):
            lg = logits.permute(1, 0, 2, 3, 4).to(dt).clone().requires_grad_(True)
            L = st.loss_fn(lg, mix.to(dt), target.to(dt))
            res[dt] = (float(L), 0.5 * torch.autograd.grad(L, lg)[0].permute(1, 0, 2, 3, 4))
        print(f"SEPTRAIN_LOSS stage I={I}: device {loss:.9e} fp64 {res[F64][0]:.9e} fp32 {res[F32][0]:.9e}")
        assert abs(loss - res[F64][0]) <= max(4.0 * abs(res[F32][0] - res[F64][0]), FLOOR * abs(res[F64][0]))
        _hold(f"dlogits I={I}", d, res[F32][1], res[F64][1])
        assert float(d[0, :, 3, 7].abs().max()) == 0.0
        if I == 2:
            assert float(d[0, :, 5, 9].abs().max()) == 0.0
        tr.close()
    _verdict()


# ------------------------------------------------------------------ hand-over, segments, learning
def _audio(N, seed):
    return np.ascontiguousarray(synth.clip_audio(seed, seconds=(N + 4410) / 44100.0)[:, :N], np.float32)


def test_training_segments_are_the_separators_magnitudes():
    c = _case(ODD, 64, 64, 2, 2, 2)
    sep = _trainer(c).to_separator()
    N = 64 * 256 + 5
    wavs = [_audio(N, 40 + 2 * k) for k in range(3)]
    mix, target = training_segments(sep, wavs[0], wavs[1:])
    assert mix.is_cuda and tuple(mix.shape) == (2, 64, 64, 2) and tuple(target.shape) == (2, 2, 64, 64, 2)
    for k, w in enumerate(wavs):
        got = mix if k == 0 else target[k - 1]
        _hold(f"segments {k}", got, sp.magnitudes(sp.stft(w, 1024, F32), 64, 64), sp.magnitudes(sp.stft(w, 1024, F64), 64, 64))
    assert float(mix[1, 5:].abs().max()) == 0.0         # the frames past the song's last are zeros
    with pytest.raises(ValueError, match="one length"):
        training_segments(sep, wavs[0], [wavs[1], wavs[2][:, :100]])
    _verdict()


def test_hand_over_to_the_separator_and_save_round_trip(tmp_path):
    c = _case(ODD, 64, 64, 2, 2, 2)
    tr = _trainer(c, lr=1e-3)
    tr.train_step(c["mix"], c["target"])
    sd = tr.state_dict()
    assert any(not np.array_equal(sd[k], c["state"][k]) for k in sd if k.endswith(".mean"))
    sep = tr.to_separator()
    x = _audio(64 * 256 + 5, 50)
    got = sep.separate_many([x])[0]
    _hold("chain on the trained state", got, sp.separate(x, sep.config, sd, F32), sp.separate(x, sep.config, sd, F64))
    tr.save(tmp_path / "sep.pth")
    back = load_separator_state(tmp_path / "sep.pth")
    assert list(back) == list(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    tr.close()
    _verdict()


def test_a_few_steps_lower_the_loss_on_two_sources_in_disjoint_bands():
    """a direction check with no threshold: a sign error anywhere between the loss and Adam cannot pass it by symmetry"""
    c = _case(ODD, 64, 64, 2, 2, 2)
    tr = _trainer(c, lr=2e-3)
    sep = tr.to_separator()
    N = 2 * 64 * 256 - 1024 - 256
    zero = np.zeros((2, N), np.float32)
    a, _ = training_segments(sep, _audio(N, 60), [zero, zero])
    b, _ = training_segments(sep, _audio(N, 62), [zero, zero])
    a[:, :, 32:] = 0.0                                  # source a below bin 32, source b from bin 32 up
    b[:, :, :32] = 0.0
    mix, target = a + b, torch.stack([a, b])
    losses = [tr.train_step(mix, target) for _ in range(6)]
    losses.append(tr.loss(mix, target, frozen_stats=False))
    print("SEPTRAIN_LEARN", " ".join(f"{v:.6e}" for v in losses))
    assert losses[-1] < losses[0]
    tr.close()


# ------------------------------------------------------------------ refusals and bounds
def test_a_batch_over_the_budget_is_refused_with_the_bytes_and_the_engine_goes_on():
    c = _case(ODD, 64, 64, 2, 2, 2)
    probe = _trainer(c)
    need1, need2 = probe.workspace_total_bytes(1), probe.workspace_total_bytes(2)
    probe.close()
    tr = _trainer(c, workspace_bytes=need1)
    with pytest.raises(_lib.EtudeHipError, match=str(need2)):
        tr.loss_and_backward(c["mix"], c["target"])
    assert all(not v.any() for v in tr.grads().values())
    loss = tr.loss_and_backward(c["mix"][:1], c["target"][:, :1])
    assert np.isfinite(loss) and any(v.any() for v in tr.grads().values())
    tr.close()


def test_non_finite_or_negative_input_is_refused():
    c = _case(ODD, 64, 64, 2, 2, 2)
    tr = _trainer(c)
    bad = c["mix"].clone()
    bad[1, 2, 3, 0] = float("nan")
    with pytest.raises(ValueError, match="mix holds"):
        tr.loss_and_backward(bad, c["target"])
    neg = c["target"].clone()
    neg[1, 0, 0, 0, 0] = -1e-3
    with pytest.raises(ValueError, match="target holds"):
        tr.loss_and_backward(c["mix"], neg)
    tr.close()


from _util import Guarded as _Guarded  # noqa: E402  (n floats between guard floats, all holding a NaN pattern until a kernel writes them)


def test_guard_floats_around_every_tap_output_are_untouched():
    c = _case(ODD, 128, 64, 2, 3, 2)
    tr, per, lib = _trainer(c), _taps(c), _lib.lib()
    cfg, B, I = c["cfg"], 3, 2
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(31)
    for j in (1, 4, 6):
        skip, up, v = _stack(per, f"deconv{j}", 0), (_stack(per, f"deconv{j}", 1) if j > 1 else None), _stack(per, f"deconv{j}", 2)
        dy = torch.randn(v.shape, generator=g).cuda()
        o0, o1 = _Guarded(skip.numel()), _Guarded(up.numel() if j > 1 else 1, fill=0)
        _lib.check(lib.etd_septrain_debug_dx(tr.h, 1, j, p(dy), B, o0.ptr, o1.ptr, st0), "dx")
        o0.check(f"deconv{j} dskip"); o1.check(f"deconv{j} dup")
        dw = _Guarded(I * c["state"][f"a.deconv{j}.weight"].size, fill=0)
        sk, u = skip.cuda(), up.cuda() if j > 1 else None
        _lib.check(lib.etd_septrain_debug_dw(tr.h, 1, j, p(sk), p(u) if j > 1 else None, p(dy), B, dw.ptr, st0), "dw")
        dw.check(f"deconv{j} dW")
    for l in (2, 6):
        x, pre = _stack(per, f"conv{l}", 0), _stack(per, f"conv{l}", 1)
        dy = torch.randn(pre.shape, generator=g).cuda()
        o0 = _Guarded(x.numel())
        _lib.check(lib.etd_septrain_debug_dx(tr.h, 0, l, p(dy), B, o0.ptr, None, st0), "dx")
        o0.check(f"conv{l} dX")
    x, lg = _stack(per, "head", 0), _stack(per, "head", 1)
    dy = torch.randn(lg.shape, generator=g).cuda()
    o0 = _Guarded(x.numel())
    _lib.check(lib.etd_septrain_debug_dx(tr.h, 2, 0, p(dy), B, o0.ptr, None, st0), "dx")
    o0.check("head dX")
    xs = _stack(per, "conv3", 1).cuda()
    y, dx, stats = _Guarded(xs.numel()), _Guarded(xs.numel()), _Guarded(2 * I * xs.shape[-1])
    dyn = torch.randn(xs.shape, generator=g).cuda()
    _lib.check(lib.etd_septrain_debug_norm(tr.h, 3, p(xs), B, p(dyn), y.ptr, dx.ptr, stats.ptr, st0), "norm")
    y.check("norm y"); dx.check("norm dx"); stats.check("norm stats")
    d = _Guarded(lg.numel())
    loss = C.c_double()
    mix, target = c["mix"].cuda(), c["target"].cuda()
    _lib.check(lib.etd_septrain_debug_loss(tr.h, p(lg.cuda()), p(mix), p(target), B, 1.0, C.byref(loss), d.ptr, st0), "loss")
    d.check("dlogits")
    tr.close()
