"""The create-time failures that never reach the GPU, with their exact texts: a null config, a config struct of another size (all three
engines), and for the beat engine a missing checkpoint key and a tensor of the wrong element count.  etd_beat_create checks every key
before its first HIP call, so these run (and must keep running) on a machine without a GPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from etude_amd import _lib
from etude_amd.beat import expected_keys

EINVAL = -22
CREATES = [("etd_extractor_create", "extractor_create", "etd_ext_cfg", _lib.ExtCfg),
           ("etd_decoder_create", "decoder_create", "etd_dec_cfg", _lib.DecCfg),
           ("etd_beat_create", "beat_create", "etd_beat_cfg", _lib.BeatCfg)]


def _one_weight():
    return _lib.weights_arrays({"w": np.zeros(4, np.float32)})


@pytest.mark.parametrize("fn,tag,struct,cfg_t", CREATES)
def test_null_cfg(fn, tag, struct, cfg_t):
    lib = _lib.lib()
    names, ptrs, nums, n, keep = _one_weight()
    h = C.c_void_p()
    assert getattr(lib, fn)(None, names, ptrs, nums, n, C.byref(h)) == EINVAL
    assert lib.etd_last_error().decode() == f"{tag}: null argument"
    assert not h.value


@pytest.mark.parametrize("fn,tag,struct,cfg_t", CREATES)
def test_wrong_struct_bytes(fn, tag, struct, cfg_t):
    lib = _lib.lib()
    names, ptrs, nums, n, keep = _one_weight()
    cfg = cfg_t()
    want = C.sizeof(cfg_t)
    cfg.struct_bytes = want - 4
    h = C.c_void_p()
    assert getattr(lib, fn)(C.byref(cfg), names, ptrs, nums, n, C.byref(h)) == EINVAL
    assert lib.etd_last_error().decode() == (f"{tag}: {struct} of {want - 4} bytes, this library (ABI {_lib.ABI_VERSION}) expects {want} "
                                             "-- caller built against another etude_hip.h")
    assert not h.value


def _beat_cfg_and_weights():
    m = SimpleNamespace(attn_len=5, instr=5, ntoken=2, dmodel=256, nhead=8, d_hid=256, nlayers=4)
    cfg = _lib.BeatCfg(attn_len=m.attn_len, instr=m.instr, ntoken=m.ntoken, dmodel=m.dmodel, nhead=m.nhead, d_hid=m.d_hid, nlayers=m.nlayers,
                       norm_first=1, n_mels=128, tempo_out=300, max_rows=1024)
    return cfg, {k: np.zeros(s, np.float32) for k, s in expected_keys(m).items()}


# the last key etd_beat_create looks at for a 4-layer model: everything before it has passed, nothing has touched the GPU
LAST_KEY = "Transformer_layers.instr_attention_3.norm2.bias"


def _beat_create(cfg, sd):
    lib = _lib.lib()
    names, ptrs, nums, n, keep = _lib.weights_arrays(sd)
    h = C.c_void_p()
    rc = lib.etd_beat_create(C.byref(cfg), names, ptrs, nums, n, C.byref(h))
    return rc, lib.etd_last_error().decode(), h


@pytest.mark.parametrize("key", ["conv1.weight", "Transformer_layers.time_attention_2.self_attn.Er", LAST_KEY])
def test_beat_missing_weight(key):
    cfg, sd = _beat_cfg_and_weights()
    del sd[key]
    rc, msg, h = _beat_create(cfg, sd)
    assert rc == EINVAL and not h.value
    assert msg == f"beat_create: missing weight '{key}'"


@pytest.mark.parametrize("key", ["conv2.bias", LAST_KEY])
def test_beat_wrong_element_count(key):
    cfg, sd = _beat_cfg_and_weights()
    want = sd[key].size
    sd[key] = np.zeros(want - 1, np.float32)
    rc, msg, h = _beat_create(cfg, sd)
    assert rc == EINVAL and not h.value
    assert msg == f"beat_create: weight '{key}' has {want - 1} elements, expected {want}"
