#!/usr/bin/env python3
"""Generate tests/golden/beat_train_*.npz by RUNNING THE REFERENCE's Demixed_DilatedTransformerModel (etude/models/beat_transformer.py) on CPU torch in fp64 and
eval() (no dropout), applying this project's beat / tempo loss to its outputs and letting autograd give every parameter's gradient.

Runs only where the reference checkout is available (never on the GPU box).  Weights are ``etude_amd.synth.beat_state_dict`` loaded with ``strict=True``; the batch
is ``tests/beat_train_np.make_batch``, regenerated from its seed by the tests (the fixture stores the features' sha256 so that drift is caught).  A full set of
gradients is 37 MB, so each fixture holds the loss, every tensor of at most SMALL elements in full (fp64) and, for every tensor, checksums: its sum, the sum and
maximum of its magnitudes and four projections onto seeded uniform(-1, 1) vectors (``checksums``).  No weights are written.

Usage:  python tests/golden/make_golden_beat_train.py --reference DIR
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
sys.path.insert(0, str(ROOT / "tests"))
from etude_amd import synth  # noqa: E402
from beat_train_np import make_batch  # noqa: E402

SMALL = 4096
POS_WEIGHT = {2: (3.0, 7.0), 3: (3.0, 7.0, 2.0)}
TEMPO_WEIGHT = 0.5
# name, the constructor arguments that differ from the default architecture, T, batch seed, weight seed
CASES = [("default", dict(), 37, 21, 7), ("archA", dict(instr=3, nlayers=5, d_hid=512, ntoken=3), 70, 22, 11)]


def checksums(name: str, g: np.ndarray) -> np.ndarray:
    """[7] fp64: sum, sum |g|, max |g|, and 4 projections onto uniform(-1, 1) vectors seeded by the tensor's name"""
    g = np.asarray(g, np.float64).reshape(-1)
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))
    return np.array([g.sum(), np.abs(g).sum(), np.abs(g).max()] + [float(g @ rng.uniform(-1.0, 1.0, g.size)) for _ in range(4)], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference repository (Xiugapurin/Etude)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from etude.models.beat_transformer import Demixed_DilatedTransformerModel
    for name, over, T, seed, wseed in CASES:
        dims = synth.beat_dims(**over)
        model = Demixed_DilatedTransformerModel(attn_len=5, instr=dims["instr"], ntoken=dims["ntoken"], dmodel=256, nhead=8, d_hid=dims["d_hid"],
                                                nlayers=dims["nlayers"], norm_first=True)
        sd = synth.beat_state_dict(wseed, dims)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.double().eval()
        b = make_batch(seed, [T], instr=dims["instr"], ntoken=dims["ntoken"])
        feat, y, p = (torch.from_numpy(np.asarray(a, np.float64)) for a in (b["feats"][0], b["beat"][0], b["tempo"][0]))
        z, t = model(feat[None])
        z, t = z[0], t[0]
        pw = torch.tensor(POS_WEIGHT[dims["ntoken"]], dtype=torch.float64)
        loss = 0.0
        for c in range(dims["ntoken"]):
            m = y[:, c] >= 0
            yc, zc = y[m, c], z[m, c]
            bce = torch.clamp(zc, min=0) - zc * yc + torch.log1p(torch.exp(-zc.abs()))
            loss = loss + ((1 + (pw[c] - 1) * yc) * bce).sum() / int(m.sum())
        loss = loss + TEMPO_WEIGHT * -(p * torch.log_softmax(t, -1)).sum()
        loss.backward()
        grads = {k: v.grad.numpy() for k, v in model.named_parameters()}
        assert set(grads) == set(sd), sorted(set(sd) ^ set(grads))
        out = {"T": np.int64(T), "seed": np.int64(seed), "weight_seed": np.int64(wseed), "loss": np.float64(loss.detach()),
               "feat_sha256": np.array(hashlib.sha256(np.ascontiguousarray(b["feats"][0], np.float32).tobytes()).hexdigest()),
               "pos_weight": np.array(POS_WEIGHT[dims["ntoken"]], np.float64), "tempo_weight": np.float64(TEMPO_WEIGHT)}
        out.update({k: np.int64(v) for k, v in over.items()})
        for k, g in grads.items():
            out["sum:" + k] = checksums(k, g)
            if g.size <= SMALL:
                out["grad:" + k] = g.astype(np.float64)
        np.savez_compressed(HERE / f"beat_train_{name}.npz", **out)
        print(f"beat_train_{name}.npz  loss {float(loss):.6f}  {len(grads)} tensors  {(HERE / f'beat_train_{name}.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
