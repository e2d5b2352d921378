#!/usr/bin/env python3
"""Generate tests/golden/beat_*.npz by RUNNING THE REFERENCE's Demixed_DilatedTransformerModel (etude/models/beat_transformer.py) on CPU torch, fp32, eval().

Runs only where the reference checkout is available (never on the GPU box).  Weights are ``etude_amd.synth.beat_state_dict`` loaded with ``strict=True`` (the key
names and shapes are checked against the reference class as a side effect); inputs are ``synth.beat_features``, regenerated from their seeds by the tests, and each
fixture stores the input's sha256 so that drift in ``synth`` is caught.  Outputs are data only: logits, tempo head and, for T = 37, the conv front-end and
layer-0 activations (captured by forward hooks); ARCHS adds two other architectures (logits and tempo only).  No weights are written.

Usage:  python tests/golden/make_golden_beat.py --reference DIR
"""
from __future__ import annotations

import argparse
import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
from etude_amd import synth  # noqa: E402

WEIGHT_SEED = 7
CASES = [(1, 101), (5, 102), (37, 103), (300, 104), (1100, 105)]        # (T, feature seed), B = 1
BATCH = (2, 64, (201, 202))                                             # B = 2 forward: T, feature seeds
# other architectures (logits and tempo only): name, the constructor arguments that differ, T, feature seed, weight seed
ARCHS = [("archA", dict(instr=3, nlayers=5, d_hid=512, ntoken=3), 70, 301, 11), ("archB", dict(instr=8, nlayers=11), 40, 302, 12)]


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from etude.models.beat_transformer import Demixed_DilatedTransformerModel
    torch.manual_seed(0)
    dims = synth.beat_dims()
    model = Demixed_DilatedTransformerModel(attn_len=5, instr=5, ntoken=2, dmodel=256, nhead=8, d_hid=1024, nlayers=9, norm_first=True)
    sd = synth.beat_state_dict(WEIGHT_SEED, dims)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.eval()
    assert len(sd) == 181

    taps = {}
    model.dropout3.register_forward_hook(lambda m, i, o: taps.__setitem__("front", o.detach().clone()))
    model.Transformer_layers["time_attention_0"].register_forward_hook(lambda m, i, o: taps.__setitem__("layer0", o[0].detach().clone()))

    for T, seed in CASES:
        feat = synth.beat_features(seed, T)
        with torch.no_grad():
            logits, tempo = model(torch.from_numpy(feat)[None])
        lg = logits[0].numpy()
        if T >= 37:      # non-degenerate: logits vary over frames and take both signs
            assert lg.std(0).min() > 1e-2 * max(1.0, np.abs(lg).max()), (T, lg.std(0))
            assert (lg > 0).any() and (lg < 0).any(), T
        out = dict(T=np.int64(T), seed=np.int64(seed), weight_seed=np.int64(WEIGHT_SEED), feat_sha256=np.array(sha(feat)), logits=lg.astype(np.float32),
                   tempo=tempo[0].numpy().astype(np.float32))
        if T == 37:
            out["front"] = taps["front"].reshape(5, 256, T).numpy().transpose(0, 2, 1).astype(np.float32)       # [instr][T][D]
            out["layer0"] = taps["layer0"].numpy().astype(np.float32)                                          # [instr][T][D]
        np.savez_compressed(HERE / f"beat_T{T}.npz", **out)
        print(f"beat_T{T}.npz  max|logit| {np.abs(lg).max():.3f}  std over frames {lg.std(0) if T > 1 else 0}")

    B, T, seeds = BATCH
    feats = np.stack([synth.beat_features(s, T) for s in seeds])
    with torch.no_grad():
        logits, tempo = model(torch.from_numpy(feats))
    np.savez_compressed(HERE / "beat_B2.npz", T=np.int64(T), seeds=np.array(seeds, np.int64), weight_seed=np.int64(WEIGHT_SEED),
                        feat_sha256=np.array([sha(f) for f in feats]), logits=logits.numpy().astype(np.float32), tempo=tempo.numpy().astype(np.float32))
    print("beat_B2.npz")
    arch_goldens(Demixed_DilatedTransformerModel)


def arch_goldens(Model):
    for name, over, T, seed, wseed in ARCHS:
        dims = synth.beat_dims(**over)
        model = Model(attn_len=5, instr=dims["instr"], ntoken=dims["ntoken"], dmodel=256, nhead=8, d_hid=dims["d_hid"], nlayers=dims["nlayers"], norm_first=True)
        sd = synth.beat_state_dict(wseed, dims)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.eval()
        feat = synth.beat_features(seed, T, instr=dims["instr"])
        with torch.no_grad():
            logits, tempo = model(torch.from_numpy(feat)[None])
        lg = logits[0].numpy()
        assert lg.shape == (T, dims["ntoken"]) and lg.std(0).min() > 1e-2 * max(1.0, np.abs(lg).max()), (name, lg.std(0))
        np.savez_compressed(HERE / f"beat_{name}.npz", T=np.int64(T), seed=np.int64(seed), weight_seed=np.int64(wseed), feat_sha256=np.array(sha(feat)),
                            logits=lg.astype(np.float32), tempo=tempo[0].numpy().astype(np.float32), **{k: np.int64(v) for k, v in over.items()})
        print(f"beat_{name}.npz  {over}  max|logit| {np.abs(lg).max():.3f}  std over frames {lg.std(0)}")


if __name__ == "__main__":
    main()
