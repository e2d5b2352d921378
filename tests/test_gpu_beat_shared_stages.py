"""The claim the shared forward kernels of csrc/beat.hip rest on: on the same input and parameters, every non-GEMM forward stage that the inference engine
(etd_beat_*) and the trainer (etd_btrain_*) both run gives the same bits on either side.  One BeatDetector with stage taps on (etd_beat_debug_stage_taps) and one
BeatTrainer are made from the same synthetic state; each trainer-side tap (etd_debug_btrain_front_fwd, _dattn, _iattn, _means) is fed the ENGINE's tapped input
and the trainer's own copy of the parameters, and its output must equal the engine's tapped output bit for bit.  No comparison here has a tolerance.

  conv1     feat -> c1
  patch3    c2 -> x3.  The engine's conv2 runs over 42 columns, the trainer's over the 24 the model reads: the 24-column c2 is cut from the engine's tap on the host
  pool3     c3 -> front
  dattn     qkv, Er and the layer's input -> skip and x_attn, layers 0, 3 and 8 (the engine updates x in place, the trainer writes out of place and keeps prob)
  iattn     iqkv -> iao, the three instrument layers
  skipacc   skip of layers 0, 1, 2 -> tacc after each

The engine's taps expose the input of every one of these stages, so none is left out.  Shapes: songs of 1, 2, 7 and 37 frames in one ragged call (at dilation 256
every tap but the centre is masked; T = 1 and 2 mask taps at dilation 1), instr 5 and 1, and instr 5 once more with max_rows so low that the engine runs the call
in two chunks: the second starts at song 3, so its kernels see first > 0, row_base > 0 and frame_base > 0, which the trainer's whole-call table never has."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beat_stage_check as S
from etude_amd import _lib, synth
from etude_amd._engine import i64
from etude_amd.beat_train import BeatTrainer
from etude_amd.config import BeatDetectorModelConfig

pytestmark = pytest.mark.gpu
TS = [1, 2, 7, 37]
CASES = {"instr5": (5, 1 << 12), "instr1": (1, 1 << 12), "instr5-chunks": (5, 40)}      # (instr, the engine's max_rows); 40 < 5 x 37: chunks of songs 0 .. 2 and of song 3


@functools.lru_cache(maxsize=None)
def call(case):
    """(instr, the engine's taps of one call, the trainer's parameters); computed once per case and left unchanged"""
    instr, max_rows = CASES[case]
    dims = synth.beat_dims(instr=instr, d_hid=256)
    sd = synth.beat_state_dict(11, dims)
    feats = [synth.beat_features(900 + i, T, instr=instr) for i, T in enumerate(TS)]
    taps = S.device_taps(S.detector(dims, sd, max_rows), dims, feats, (1 << dims["nlayers"]) - 1, True)
    trainer = BeatTrainer(config=BeatDetectorModelConfig(**dims), state=sd, max_rows=instr * sum(TS), max_seqs=len(TS))
    params = trainer.state_dict()
    assert all(np.array_equal(np.asarray(params[k]), sd[k]) for k in sd)
    return instr, taps, params


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda().contiguous()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def out(*shape):
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    t.view(torch.uint8).fill_(0xFF)                      # NaN patterns: an output that was not written cannot pass
    return t


def same_bits(got, want, what):
    torch.cuda.synchronize()
    g, w = got.cpu().numpy().reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    assert g.shape == w.shape and np.isfinite(w).all(), what
    bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} floats differ, the first at {bad[0]}: trainer side {g[bad[0]]!r}, engine {w[bad[0]]!r}"


def front(which, instr, x, w=None, b=None, *shape):
    keep = [dev(x), None if w is None else dev(w), None if b is None else dev(b)]
    y = out(*shape)
    _lib.check(_lib.lib().etd_debug_btrain_front_fwd(which, len(TS), i64(TS), instr, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(y), None), "etd_debug_btrain_front_fwd")
    return y


@pytest.mark.parametrize("case", list(CASES))
def test_front_end(case):
    instr, t, p = call(case)
    R = instr * sum(TS)
    feat = np.concatenate([f.reshape(-1, 128) for f in t["feat"]])
    same_bits(front(0, instr, feat, np.asarray(p["conv1.weight"]).reshape(32, 15), p["conv1.bias"], R, 42, 32), t["c1"], "conv1")
    same_bits(front(2, instr, t["c2"].reshape(R, 42, 64)[:, :24], None, None, R * 3, 1152), t["x3"], "patch3")
    same_bits(front(3, instr, t["c3"], None, None, R, 256), t["front"], "pool3")


@pytest.mark.parametrize("layer", [0, 3, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_dilated_attention(case, layer):
    instr, t, p = call(case)
    R = instr * sum(TS)
    xin = t["front"] if layer == 0 else t[f"x_ffn.{layer - 1}"]          # layers 2 and 7 have no instrument layer behind them
    keep = [dev(t[f"qkv.{layer}"]), dev(p[f"Transformer_layers.time_attention_{layer}.self_attn.Er"]), dev(xin)]
    prob, skip, xout = out(R, 8, 5), out(R, 256), out(R, 256)
    _lib.check(_lib.lib().etd_debug_btrain_dattn(len(TS), i64(TS), instr, layer, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), None, ptr(prob), ptr(skip), ptr(xout),
                                                 None, None, None, None, None), "etd_debug_btrain_dattn")
    same_bits(skip, t[f"skip.{layer}"], f"skip.{layer}")
    same_bits(xout, t[f"x_attn.{layer}"], f"x_attn.{layer}")
    assert bool(torch.isfinite(prob).all())


@pytest.mark.parametrize("case", list(CASES))
def test_instrument_attention(case):
    instr, t, _ = call(case)
    for layer in (3, 4, 5):
        qkv, ao = dev(t[f"iqkv.{layer}"]), out(instr * sum(TS), 256)
        _lib.check(_lib.lib().etd_debug_btrain_iattn(len(TS), i64(TS), instr, ptr(qkv), None, ptr(ao), None, None), "etd_debug_btrain_iattn")
        same_bits(ao, t[f"iao.{layer}"], f"iao.{layer}")


@pytest.mark.parametrize("case", list(CASES))
def test_skip_accumulation(case):
    instr, t, _ = call(case)
    tacc = out(sum(TS), 256)
    for layer in (0, 1, 2):
        skip = dev(t[f"skip.{layer}"])
        _lib.check(_lib.lib().etd_debug_btrain_means(0, len(TS), i64(TS), instr, ptr(skip), None, 1 if layer == 0 else 0, ptr(tacc), None), "etd_debug_btrain_means")
        same_bits(tacc, t[f"tacc.{layer}"], f"tacc.{layer}")
