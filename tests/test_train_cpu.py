"""CPU checks of the training feature: the fp64 restatement (tests/train_np.py) against the golden recorded from the reference's EtudeDecoder, the hand-written
clip + AdamW against torch's, the schedule against transformers', and what DecoderTrainer refuses before it needs a GPU."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import train_np as tn  # noqa: E402
from etude_amd import _lib  # noqa: E402
from etude_amd import train as T  # noqa: E402

OPT = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
RAGGED = (1, 2, 63, 64, 65, 127, 128, 129, 256)


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) <= tol * max(float(np.abs(b).max()), 1e-300)


def test_restatement_reproduces_the_reference_golden(golden_dir):
    g = np.load(golden_dir / "train_tiny.npz")
    cfg = tn.tiny_config()
    state = tn.seeded_state(cfg, 3)
    batch = tn.ragged_batch(cfg, RAGGED, seed=5, ignore_all=(4,))
    loss, grads = tn.loss_and_grads(state, cfg, batch, torch.float64)
    assert abs(loss - float(g["loss"])) <= 1e-10 * abs(float(g["loss"]))
    total = max(float(g["grad_norm/" + k]) for k in grads)
    for k, gr in grads.items():
        assert abs(float(np.linalg.norm(gr)) - float(g["grad_norm/" + k])) <= 1e-10 * total, k
        idx = g["sample_index/" + k]
        assert np.abs(gr.reshape(-1)[idx] - g["grad_sample/" + k]).max() <= 1e-10 * max(float(np.abs(gr).max()), 1e-300), k
    assert not grads[tn.FROZEN].any() and float(g["grad_norm/" + tn.FROZEN]) == 0.0
    # one clip + AdamW step
    p = {k: np.array(v, np.float64) for k, v in state.items()}
    z = lambda: {k: np.zeros_like(v) for k, v in p.items()}      # noqa: E731
    tn.clip_and_adamw(p, grads, z(), z(), 1, 1.0, **OPT)
    for k in p:
        assert close(p[k].reshape(-1)[g["sample_index/" + k]], g["param_sample/" + k], 1e-10), k
    # five steps on the trajectory batch
    tb = tn.ragged_batch(cfg, (40, 64, 17), seed=21)
    losses = [s[0] for s in tn.trajectory(state, cfg, [tb, tb], 6, torch.float64, **OPT)]
    assert abs(losses[5] - float(g["loss_after_5_steps"])) <= 1e-10 * abs(losses[5])
    assert losses[5] < losses[0]


@pytest.mark.parametrize("max_norm", [0.05, 1e3])
def test_hand_written_clip_and_adamw_is_torchs(max_norm):
    rng = np.random.default_rng(0)
    params = {"a.weight": rng.standard_normal((7, 5)), "b.bias": rng.standard_normal(11), tn.FROZEN: rng.standard_normal((3, 2))}
    m = {k: np.zeros_like(v) for k, v in params.items()}
    v = {k: np.zeros_like(p) for k, p in params.items()}
    mine = {k: p.copy() for k, p in params.items()}
    for step in range(1, 4):
        grads = {k: 0.3 * rng.standard_normal(p.shape) for k, p in params.items()}
        theirs = tn.torch_clip_and_adamw(mine, grads, step - 1, m, v, max_norm, dtype=torch.float64, **OPT)
        norm = tn.clip_and_adamw(mine, {k: g.copy() for k, g in grads.items()}, m, v, step, max_norm, **OPT)
        assert (norm > max_norm) == (max_norm < 1.0)
        for k in mine:
            assert close(mine[k], theirs[k], 1e-12), (k, step)
    assert np.array_equal(mine[tn.FROZEN], params[tn.FROZEN])


def test_schedule_is_transformers():
    tf = pytest.importorskip("transformers")
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sch = tf.get_cosine_schedule_with_warmup(opt, num_warmup_steps=7, num_training_steps=40)
    for step in range(45):
        want = sch.get_last_lr()[0]
        assert abs(T.cosine_schedule_with_warmup(step, 7, 40) - want) <= 1e-15, step
        assert T.cosine_schedule_with_warmup(step, 7, 40) == tn.cosine_schedule_with_warmup(step, 7, 40)
        opt.step(); sch.step()


def test_init_is_the_reference_distribution():
    cfg = tn.tiny_config(initializer_range=0.02)
    sd = T.init_decoder_state(cfg, seed=1)
    assert list(sd) == list(T.state_shapes(cfg))
    assert not sd["word_embeddings.weight"][cfg.pad_token_id].any() and not sd["polyphony_embeddings.weight"][cfg.attribute_pad_id].any()
    assert np.all(sd["transformer.final_layer_norm.weight"] == 1) and not sd["attribute_projection.bias"].any()
    w = sd["transformer.layers.0.mlp.dense_h_to_4h.weight"]
    assert abs(float(w.std()) - 0.02) < 5e-4 and abs(float(w.mean())) < 5e-4


def test_trainer_refuses_bad_batches_and_shapes():
    cfg = tn.tiny_config()
    good = tn.ragged_batch(cfg, (5, 3), seed=0)
    Tn, ids, cls, attrs4, labels = T.pack_batch(cfg, good)
    assert Tn.tolist() == [5, 3] and ids.shape == (8,) and attrs4.shape == (4, 8) and labels.dtype == np.int32
    assert np.array_equal(attrs4[2], good["sustain_bin_ids"][good["attention_mask"] == 1])          # C-ABI order: overlap, polyphony, sustain, rhythm

    def broken(**kw):
        b = {k: v.copy() for k, v in good.items()}
        for k, (i, j, val) in kw.items():
            b[k][i, j] = val
        return b
    left = {k: v[:, ::-1].copy() for k, v in good.items()}
    with pytest.raises(ValueError, match="right padding"):
        T.pack_batch(cfg, left)
    with pytest.raises(ValueError, match="padded position"):
        T.pack_batch(cfg, broken(labels=(1, 4, 9)))
    for key, val in (("input_ids", cfg.vocab_size), ("class_ids", cfg.num_classes), ("sustain_bin_ids", cfg.num_attribute_bins), ("labels", cfg.vocab_size),
                     ("input_ids", -1), ("labels", -7)):
        with pytest.raises(ValueError, match="outside"):
            T.pack_batch(cfg, broken(**{key: (0, 1, val)}))
    with pytest.raises(ValueError, match="lacks"):
        T.pack_batch(cfg, {k: v for k, v in good.items() if k != "sustain_bin_ids"})
    with pytest.raises(ValueError, match="max_position_embeddings"):
        T.pack_batch(tn.tiny_config(max_position_embeddings=4), good)
    # shapes outside the limits: a ValueError from the constructor before any GPU is needed ...
    for over in (dict(hidden_size=128, num_attention_heads=2), dict(hidden_size=256, num_attention_heads=8), dict(intermediate_size=192), dict(rotary_pct=0.5)):
        with pytest.raises(ValueError):
            T.DecoderTrainer(tn.tiny_config(**over))
    with pytest.raises(ValueError, match="shape"):
        T.DecoderTrainer(cfg, {**tn.seeded_state(cfg), "lm_head.weight": np.zeros((3, 3), np.float32)})
    # ... and ETD_EINVAL with a message from the library before it touches the device
    c = _lib.DecCfg(vocab_size=157, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=512, max_position_embeddings=64, num_classes=3,
                    num_attribute_bins=3, attribute_emb_dim=64, rotary_pct=0.25, rope_theta=10000.0, layer_norm_eps=1e-5)
    h = C.c_void_p()
    names, ptrs, numels, n, keep = _lib.weights_arrays({"x": np.zeros(1, np.float32)})
    assert _lib.lib().etd_dtrain_create(C.byref(c), names, ptrs, numels, n, 0, 0, 0, 64, C.byref(h)) == -22
    assert b"multiple of 256" in _lib.lib().etd_last_error()
    assert _lib.lib().etd_dtrain_workspace_bytes(C.byref(c), 64) == -22
    c.hidden_size, c.num_attention_heads = 256, 4
    assert _lib.lib().etd_dtrain_workspace_bytes(C.byref(c), 64) > 0
    assert _lib.lib().etd_dtrain_create(C.byref(c), names, ptrs, numels, n, 0, 0, 0, 64, C.byref(h)) == -22
    assert b"missing weight" in _lib.lib().etd_last_error()


def test_stage_references_chained_reproduce_the_restatement():
    """tests/train_stage_np.py states each kernel of the trainer on its own (the references of tests/test_gpu_train_stages.py); chained in fp64 in the engine's
    order they are the model: the loss and every gradient of tn.loss_and_grads to 1e-12 relative."""
    import train_stage_np as ts
    cfg = tn.tiny_config()
    state = tn.seeded_state(cfg, 3)
    batch = tn.ragged_batch(cfg, (1, 2, 63, 65, 40), seed=5, ignore_all=(3,))
    loss, grads = tn.loss_and_grads(state, cfg, batch, torch.float64)
    loss_c, grads_c = ts.chain(state, cfg, batch, torch.float64)
    assert abs(loss_c - loss) <= 1e-12 * abs(loss), (loss_c, loss)
    assert list(grads_c) == list(grads)
    for k in grads:
        assert close(grads_c[k], grads[k], 1e-12), (k, float(np.abs(grads_c[k] - grads[k]).max()), float(np.abs(grads[k]).max()))
    assert not grads_c[tn.FROZEN].any()


def test_stage_taps_refuse_malformed_arguments_before_any_launch():
    """ETD_EINVAL from every etd_debug_dtrain_* tap without a GPU: the checks run before the device is touched (`dev` stands for a device pointer that is never read)"""
    lib, dev = _lib.lib(), C.c_void_p(4096)
    i32 = lambda *v: np.array(v, np.int32)      # noqa: E731
    ids, ptr = i32(0, 1, 2), lambda a: a.ctypes.data      # noqa: E731
    calls = {
        "ln: no input": lib.etd_debug_dtrain_ln(None, 2, 8, 1e-5, dev, dev, dev, dev, dev, None, None, None, None, None, None),
        "ln: H = 0": lib.etd_debug_dtrain_ln(dev, 2, 0, 1e-5, dev, dev, dev, dev, dev, None, None, None, None, None, None),
        "ln: mean without rstd": lib.etd_debug_dtrain_ln(dev, 2, 8, 1e-5, dev, None, dev, dev, dev, None, None, None, None, None, None),
        "ln: y2 without its gain": lib.etd_debug_dtrain_ln(dev, 2, 8, 1e-5, dev, dev, dev, dev, dev, None, None, dev, None, None, None),
        "ln: dy without dx": lib.etd_debug_dtrain_ln(dev, 2, 8, 1e-5, dev, dev, dev, dev, dev, None, None, None, dev, None, None),
        "ln: backward without statistics": lib.etd_debug_dtrain_ln(dev, 2, 8, 1e-5, None, None, dev, dev, dev, None, None, None, dev, dev, None),
        "gelu: n = 0": lib.etd_debug_dtrain_gelu(dev, 0, dev, None, None),
        "gelu: no output": lib.etd_debug_dtrain_gelu(dev, 4, None, dev, None),
        "add3: n = 0": lib.etd_debug_dtrain_add3(dev, dev, dev, 0, dev, None),
        "rope: no handle": lib.etd_debug_dtrain_rope(None, dev, 1, 2, dev, 1, None),
        "embed: M = 0": lib.etd_debug_dtrain_embed(0, 256, 8, 5, 3, 3, ptr(ids), ptr(ids), ptr(ids), *([dev] * 9), None),
        "embed: token id past the table": lib.etd_debug_dtrain_embed(3, 256, 8, 2, 3, 3, ptr(ids), ptr(ids), ptr(i32(*[0] * 12)), *([dev] * 9), None),
        "embed: no table": lib.etd_debug_dtrain_embed(3, 256, 8, 5, 3, 3, ptr(ids), ptr(ids), ptr(i32(*[0] * 12)), dev, dev, dev, None, dev, dev, dev, dev, dev, None),
        "ce: label = V": lib.etd_debug_dtrain_ce(dev, 3, 2, ptr(ids), 1.0, dev, None),
        "ce: V = 0": lib.etd_debug_dtrain_ce(dev, 3, 0, ptr(ids), 1.0, dev, None),
        "colred: mode 2": lib.etd_debug_dtrain_colred(2, dev, 8, 4, 8, dev, dev, dev, dev, dev, None),
        "colred: stride below the row": lib.etd_debug_dtrain_colred(0, dev, 7, 4, 8, None, None, None, dev, None, None),
        "colred: mode 1 without x": lib.etd_debug_dtrain_colred(1, dev, 8, 4, 8, None, dev, dev, dev, dev, None),
        "embed_grad: index past the table": lib.etd_debug_dtrain_embed_grad(dev, 8, 0, 8, 3, ptr(ids), 2, 0, dev, None),
        "embed_grad: columns past the row": lib.etd_debug_dtrain_embed_grad(dev, 8, 4, 8, 3, ptr(ids), 3, 0, dev, None),
        "embed_grad: padding row outside": lib.etd_debug_dtrain_embed_grad(dev, 8, 0, 8, 3, ptr(ids), 3, 3, dev, None),
        "adamw: step 0": lib.etd_debug_dtrain_adamw(dev, dev, dev, dev, 4, 1.0, 1.0, 1e-3, 0.9, 0.98, 1e-8, 0.01, 0, None),
        "adamw: beta1 = 1": lib.etd_debug_dtrain_adamw(dev, dev, dev, dev, 4, 1.0, 1.0, 1e-3, 1.0, 0.98, 1e-8, 0.01, 1, None),
        "adamw: n = 0": lib.etd_debug_dtrain_adamw(dev, dev, dev, dev, 0, 1.0, 1.0, 1e-3, 0.9, 0.98, 1e-8, 0.01, 1, None),
        "sumsq: n = 0": lib.etd_debug_dtrain_sumsq(dev, 0, C.byref(C.c_double()), None),
        "sumsq: no result": lib.etd_debug_dtrain_sumsq(dev, 4, None, None),
    }
    assert {k: v for k, v in calls.items() if v != -22} == {}
    assert b"etd_debug_dtrain_sumsq" in lib.etd_last_error()
