"""Beat-Transformer engine, CPU side: the numpy restatement (tests/beat_np.py) against the reference's goldens, the config mirror, the loader's key contract and
etd_beat_create's refusals (which happen before any HIP call)."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_np  # noqa: E402

from etude_amd import _lib, synth  # noqa: E402
from etude_amd.beat import check_state_dict, expected_keys, load_state_dict  # noqa: E402
from etude_amd.config import BeatDetectorConfig, BeatDetectorModelConfig  # noqa: E402

WEIGHT_SEED = 7


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def sd():
    return synth.beat_state_dict(WEIGHT_SEED)


@pytest.mark.parametrize("T", [1, 5, 37, 300])
def test_restatement_matches_reference_goldens(golden_dir, sd, T):
    g = np.load(golden_dir / f"beat_T{T}.npz")
    assert int(g["weight_seed"]) == WEIGHT_SEED
    feat = synth.beat_features(int(g["seed"]), T)
    assert _sha(feat) == str(g["feat_sha256"]), "synth.beat_features drifted from the goldens"
    r = beat_np.forward(sd, feat)
    m = max(1.0, float(np.abs(g["logits"]).max()))
    assert np.abs(r["logits"] - g["logits"]).max() <= 1e-5 * m
    assert np.abs(r["tempo"] - g["tempo"]).max() <= 1e-5 * max(1.0, float(np.abs(g["tempo"]).max()))
    if T == 37:
        for k in ("front", "layer0"):
            assert np.abs(r[k] - g[k]).max() <= 1e-5 * float(np.abs(g[k]).max()), k


def test_restatement_matches_batch_golden(golden_dir, sd):
    g = np.load(golden_dir / "beat_B2.npz")
    T = int(g["T"])
    for b, seed in enumerate(g["seeds"]):
        feat = synth.beat_features(int(seed), T)
        assert _sha(feat) == str(g["feat_sha256"][b])
        r = beat_np.forward(sd, feat)
        assert np.abs(r["logits"] - g["logits"][b]).max() <= 1e-5 * max(1.0, float(np.abs(g["logits"][b]).max()))
        assert np.abs(r["tempo"] - g["tempo"][b]).max() <= 1e-5 * max(1.0, float(np.abs(g["tempo"][b]).max()))


@pytest.mark.parametrize("name", ["archA", "archB"])
def test_restatement_matches_reference_goldens_of_other_architectures(golden_dir, name):
    """archA: instr 3, nlayers 5 (instrument layers 3 and 4 only), d_hid 512, ntoken 3 at T = 70; archB: instr 8, nlayers 11 at T = 40 (tests/golden/make_golden_beat.py)"""
    g = np.load(golden_dir / f"beat_{name}.npz")
    over = {k: int(g[k]) for k in ("instr", "nlayers", "d_hid", "ntoken") if k in g}
    assert over == (dict(instr=3, nlayers=5, d_hid=512, ntoken=3) if name == "archA" else dict(instr=8, nlayers=11))
    dims = synth.beat_dims(**over)
    T = int(g["T"])
    feat = synth.beat_features(int(g["seed"]), T, instr=dims["instr"])
    assert _sha(feat) == str(g["feat_sha256"]), "synth.beat_features drifted from the goldens"
    r = beat_np.forward(synth.beat_state_dict(int(g["weight_seed"]), dims), feat, nlayers=dims["nlayers"])
    assert r["logits"].shape == g["logits"].shape == (T, dims["ntoken"])
    assert np.abs(r["logits"] - g["logits"]).max() <= 1e-5 * max(1.0, float(np.abs(g["logits"]).max()))
    assert np.abs(r["tempo"] - g["tempo"]).max() <= 1e-5 * max(1.0, float(np.abs(g["tempo"]).max()))


def test_goldens_are_small_and_nondegenerate(golden_dir):
    for p in sorted(golden_dir.glob("beat_*.npz")):
        assert p.stat().st_size < 512 * 1024, p.name
    g = np.load(golden_dir / "beat_T1100.npz")
    lg = g["logits"]
    assert lg.std(0).min() > 0.05 and (lg > 0).any() and (lg < 0).any()


def test_features_in_range():
    f = synth.beat_features(3, 500)
    assert f.shape == (5, 500, 128) and f.dtype == np.float32
    assert f.min() >= -80.0 and f.max() <= 0.0


def test_config_mirror_defaults():
    c = BeatDetectorConfig()
    assert (c.min_bpm, c.max_bpm, c.fps_divisor, c.threshold, c.beats_per_bar) == (70.0, 250.0, 1024, 0.2, [3, 4])
    m = c.model
    assert isinstance(m, BeatDetectorModelConfig)
    assert (m.attn_len, m.instr, m.ntoken, m.dmodel, m.nhead, m.d_hid, m.nlayers, m.norm_first) == (5, 5, 2, 256, 8, 1024, 9, True)


def test_loader_key_contract(tmp_path, sd):
    cfg = BeatDetectorModelConfig()
    assert len(expected_keys(cfg)) == 181 and set(expected_keys(cfg)) == set(sd)
    t = {k: torch.from_numpy(v) for k, v in sd.items()}
    torch.save(t, tmp_path / "flat.pt")
    torch.save({"state_dict": t, "epoch": 3}, tmp_path / "nested.pt")
    for name in ("flat.pt", "nested.pt"):
        got = load_state_dict(tmp_path / name)
        check_state_dict(got, cfg)
        assert set(got) == set(sd)
    missing = dict(t); missing.pop("conv2.bias")
    with pytest.raises(RuntimeError, match="missing"):
        check_state_dict(missing, cfg)
    extra = dict(t); extra["module.extra"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="unexpected"):
        check_state_dict(extra, cfg)
    prefixed = {"module." + k: v for k, v in t.items()}              # no prefix stripping (beat_detector.py:95)
    with pytest.raises(RuntimeError):
        check_state_dict(prefixed, cfg)
    bad = dict(t); bad["Transformer_layers.time_attention_2.self_attn.Er"] = torch.zeros(8, 32, 4)
    with pytest.raises(RuntimeError, match="size mismatch"):
        check_state_dict(bad, cfg)


def _create(sd, **over):
    m = dict(attn_len=5, instr=5, ntoken=2, dmodel=256, nhead=8, d_hid=1024, nlayers=9, norm_first=1, n_mels=128, tempo_out=300, max_rows=4096)
    m.update({k: v for k, v in over.items() if k != "struct_bytes"})
    cfg = _lib.BeatCfg(**m)
    if "struct_bytes" in over:
        cfg.struct_bytes = over["struct_bytes"]
    names, ptrs, nums, n, keep = _lib.weights_arrays(sd)
    h = C.c_void_p()
    rc = _lib.lib().etd_beat_create(C.byref(cfg), names, ptrs, nums, n, C.byref(h))
    return rc, _lib.lib().etd_last_error().decode()


@pytest.mark.parametrize("over,word", [(dict(nhead=4), "nhead"), (dict(attn_len=3), "attn_len"), (dict(norm_first=0), "norm_first"),
                                       (dict(struct_bytes=12), "etd_beat_cfg"), (dict(dmodel=128), "dmodel")])
def test_create_refusals_without_gpu(sd, over, word):
    rc, msg = _create(sd, **over)
    assert rc == -22 and word in msg, (rc, msg)


def test_create_refuses_missing_key_and_wrong_count(sd):
    d = dict(sd); d.pop("Transformer_layers.instr_attention_4.linear2.bias")
    rc, msg = _create(d)
    assert rc == -22 and "instr_attention_4.linear2.bias" in msg
    d = dict(sd); d["out_linear_t.bias"] = np.zeros(299, np.float32)
    rc, msg = _create(d)
    assert rc == -22 and "out_linear_t.bias" in msg
