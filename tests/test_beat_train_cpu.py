"""No GPU: the restatement tests/beat_train_np.py against goldens recorded from the reference model (tests/golden/make_golden_beat_train.py), the power of the GPU
test's bound against five wrong variants, and the argument refusals of the C ABI, which all run before the device is touched.

Goldens: the reference's Demixed_DilatedTransformerModel in eval() and fp64 with this project's loss on its outputs.  Every tensor's checksums (and the small
tensors in full) must agree to 1e-9 of the tensor's own magnitude.  One family is exempt from a RELATIVE figure: ``self_attn.key.bias`` of the time layers.  Adding a
bias to every key moves all of a query's logits by the same q . b, which the softmax cancels, so that gradient is identically zero; both sides hold rounding residue
of about 1e-17 and the test holds it to 1e-9 of the same layer's key.weight gradient instead.
"""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import beat_train_np as bt
from etude_amd import _lib, synth
from etude_amd.beat import expected_keys
from etude_amd.beat_train import check_beat_train_config, init_beat_state, pack_targets, train_cfg
from etude_amd.config import BeatDetectorModelConfig

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from make_golden_beat_train import CASES, checksums  # noqa: E402

YARD = 2.0 ** -24          # fp32's unit roundoff: the floor of the GPU test's bound is 4 x this


@pytest.fixture(scope="module", params=[c[0] for c in CASES])
def case(request, golden_dir):
    name, over, T, seed, wseed = next(c for c in CASES if c[0] == request.param)
    g = np.load(golden_dir / f"beat_train_{name}.npz")
    dims = synth.beat_dims(**over)
    state = synth.beat_state_dict(wseed, dims)
    batch = bt.make_batch(seed, [T], instr=dims["instr"], ntoken=dims["ntoken"])
    assert hashlib.sha256(np.ascontiguousarray(batch["feats"][0], np.float32).tobytes()).hexdigest() == str(g["feat_sha256"])
    kw = dict(pos_weight=g["pos_weight"], tempo_weight=float(g["tempo_weight"]))
    loss, grads = bt.loss_and_grads(state, dims["nlayers"], batch, torch.float64, **kw)
    return dict(name=name, golden=g, dims=dims, state=state, batch=batch, kw=kw, loss=loss, grads=grads)


def test_restatement_reproduces_the_reference_golden(case):
    g, grads = case["golden"], case["grads"]
    assert abs(case["loss"] - float(g["loss"])) <= 1e-12 * abs(float(g["loss"]))
    assert set(grads) == {k[4:] for k in g.files if k.startswith("sum:")}
    for k, v in grads.items():
        ref, got = g["sum:" + k], checksums(k, v)
        if k.endswith("self_attn.key.bias") and "time_attention" in k:
            scale = float(g["sum:" + k[:-4] + "weight"][2])
            assert np.abs(v).max() <= 1e-9 * scale and ref[2] <= 1e-9 * scale, k
            continue
        assert np.abs(got[[0, 1, 3, 4, 5, 6]] - ref[[0, 1, 3, 4, 5, 6]]).max() <= 1e-9 * ref[1], k
        assert abs(got[2] - ref[2]) <= 1e-9 * ref[2], k
        if "grad:" + k in g.files:
            assert np.abs(v - g["grad:" + k]).max() <= 1e-9 * ref[2], k


def test_head7_key_rows_are_exactly_zero(case):
    for l in range(case["dims"]["nlayers"]):
        p = f"Transformer_layers.time_attention_{l}.self_attn.key."
        assert not case["grads"][p + "weight"][224:].any() and not case["grads"][p + "bias"][224:].any()
        if l == 0:      # (a layer whose dilation reaches past the song has one tap in range and no key gradient at all)
            assert case["grads"][p + "weight"][:224].any()


def test_inputs_have_no_tie_and_no_zero_qk(case):
    """the index mask and the first-maximum rule are not in play on these inputs: no max-pool tie, no pooled maximum at the ReLU's kink, no in-range q . k == 0"""
    d = bt.diagnostics(case["state"], case["dims"]["nlayers"], case["batch"]["feats"])
    assert d["pool_gap"] > 0 and d["relu_gap"] > 0 and d["qk_min"] > 0, d


@pytest.mark.parametrize("mutant", ["der0", "h7own", "skip_instr-1", "fold_kw", "tempo_T-1"])
def test_wrong_variants_move_a_gradient_far_beyond_the_bound(case, mutant):
    _, gm = bt.loss_and_grads(case["state"], case["dims"]["nlayers"], case["batch"], torch.float64, mutant=mutant, **case["kw"])
    worst = max(bt.rel_err(gm[k], case["grads"][k]) for k in gm if np.abs(case["grads"][k]).max() > 0)
    assert worst >= 100 * YARD, (mutant, worst)


def test_init_state_has_the_checkpoint_keys_and_shapes():
    cfg = BeatDetectorModelConfig()
    s = init_beat_state(cfg, 3)
    assert {k: v.shape for k, v in s.items()} == {k: tuple(v) for k, v in expected_keys(cfg).items()}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in s.values())
    assert np.array_equal(init_beat_state(cfg, 3)["conv2.weight"], s["conv2.weight"]) and not np.array_equal(init_beat_state(cfg, 4)["conv2.weight"], s["conv2.weight"])


def _check(cfg, Ts, beat, tempo, has):
    lib = _lib.lib()
    Tarr = (C.c_int64 * len(Ts))(*Ts)
    ptr = lambda a: a.ctypes.data if a is not None else None      # noqa: E731
    return lib.etd_btrain_check_batch(C.byref(cfg), len(Ts), Tarr, ptr(beat), ptr(tempo), ptr(has), None, None), lib.etd_last_error()


def test_malformed_arguments_are_refused_before_the_device_is_touched():
    m = BeatDetectorModelConfig()
    lib = _lib.lib()
    with pytest.raises(ValueError, match="dropout"):
        check_beat_train_config(m, dropout=0.1)
    # ---- create: architecture and dropout (the handle is never made, no HIP call is reached)
    names, ptrs, numels, n, keep = _lib.weights_arrays({"x": np.zeros(1, np.float32)})
    h = C.c_void_p()
    for over, msg in ((dict(dropout=0.1), b"dropout"), (dict(nhead=4), b"8 heads"), (dict(d_hid=300), b"d_hid"), (dict(instr=9), b"instr"), (dict(max_rows=0), b"max_rows")):
        c = train_cfg(m, 64, 4)
        for k, v in over.items():
            setattr(c, k, v)
        assert lib.etd_btrain_create(C.byref(c), names, ptrs, numels, n, None, C.byref(h)) == -22 and msg in lib.etd_last_error(), over
        assert lib.etd_btrain_workspace_bytes(C.byref(c)) == -22
    c = train_cfg(m, 64, 4)
    assert lib.etd_btrain_workspace_bytes(C.byref(c)) > 0
    assert lib.etd_btrain_create(C.byref(c), names, ptrs, numels, n, None, C.byref(h)) == -22 and b"missing weight" in lib.etd_last_error()
    bad_pw = np.array([1.0, -2.0], np.float32)
    assert lib.etd_btrain_create(C.byref(c), names, ptrs, numels, n, bad_pw.ctypes.data, C.byref(h)) == -22 and b"pos_weight" in lib.etd_last_error()
    # ---- a batch: 64 rows = 12 frames of 5 instruments at most
    y = np.zeros((10, 2), np.float32)
    tempo = np.zeros((2, 300), np.float32)
    tempo[:, 100] = 1.0
    has = np.array([1, 1], np.int32)
    assert _check(c, [4, 6], y, tempo, has)[0] == 0
    assert _check(c, [4, 6], y, None, None)[0] == 0
    rc, msg = _check(c, [4, 9], np.zeros((13, 2), np.float32), tempo, has)
    assert rc == -22 and b"max_rows" in msg
    rc, msg = _check(c, [1] * 5, np.zeros((5, 2), np.float32), None, None)
    assert rc == -22 and b"songs" in msg
    for bad in (np.nan, 1.5, -0.5, np.inf):
        yb = y.copy()
        yb[3, 1] = bad
        rc, msg = _check(c, [4, 6], yb, tempo, has)
        assert rc == -22 and b"beat target" in msg, bad
    yb = y.copy()
    yb[3, 1] = -1.0
    assert _check(c, [4, 6], yb, tempo, has)[0] == 0
    tb = tempo.copy()
    tb[1, 7] = 1e-4
    rc, msg = _check(c, [4, 6], y, tb, has)
    assert rc == -22 and b"sums to" in msg
    assert _check(c, [4, 6], y, tb, np.array([1, 0], np.int32))[0] == 0      # a row without a target is not read
    tb = tempo.copy()
    tb[0, 5] = np.nan
    assert _check(c, [4, 6], y, tb, has)[0] == -22
    assert _check(c, [4, 0], y, tempo, has)[0] == -22
    # ---- the Python mirror's shape checks
    with pytest.raises(ValueError, match="beat target"):
        pack_targets(m, [4, 6], [np.zeros((4, 2)), np.zeros((5, 2))], None)
    with pytest.raises(ValueError, match="tempo target"):
        pack_targets(m, [4], [np.zeros((4, 2))], [np.zeros(299)])
