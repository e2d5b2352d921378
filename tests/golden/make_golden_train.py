#!/usr/bin/env python3
"""Generate tests/golden/train_tiny.npz by RUNNING THE REFERENCE's EtudeDecoder (etude/models/etude_decoder.py over transformers' GPT-NeoX) in float64 on the tiny
training configuration of tests/train_np.py.

Runs only where the reference checkout, torch and transformers are available.  The weights and the batches come from tests/train_np.py (seeded_state, ragged_batch):
they are not stored.  Stored: results only --
  loss                      the reference's forward(..., labels=...).loss of the ragged batch
  grad_norm/<key>           L2 norm of each parameter's gradient
  grad_sample/<key>         64 entries of each gradient at seeded flat indices (sample_index/<key>; every entry where the tensor has fewer)
  param_sample/<key>        the same entries of the parameter after one clip_grad_norm_(1.0) + torch.optim.AdamW step
  loss_after_5_steps        the trajectory batch's loss after 5 such steps on it (gradient accumulation of the same batch twice is the batch's gradient in fp64)

Usage:  python tests/golden/make_golden_train.py --reference DIR
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

OPT = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)      # tests/test_gpu_train.py's
RAGGED = (1, 2, 63, 64, 65, 127, 128, 129, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    os.environ.setdefault("LOG_LEVEL", "ERROR")
    from etude.models.etude_decoder import EtudeDecoder, EtudeDecoderConfig
    import train_np as tn

    cfg = tn.tiny_config()
    state = tn.seeded_state(cfg, 3)
    fields = ("vocab_size", "pad_token_id", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "max_position_embeddings", "num_classes",
              "pad_class_id", "attribute_pad_id", "num_attribute_bins", "attribute_emb_dim")

    def model():
        m = EtudeDecoder(EtudeDecoderConfig(**{k: getattr(cfg, k) for k in fields})).double()
        sd = {k: torch.tensor(v, dtype=torch.float64) for k, v in state.items()}
        extra = {k: v for k, v in m.state_dict().items() if k not in sd}      # rotary buffers, if this transformers registers any
        m.load_state_dict({**sd, **extra}, strict=True)
        m.train()                                                               # dropout is 0 in the reference's configuration: train mode == eval mode
        return m

    def loss_of(m, b):
        t = lambda k: torch.as_tensor(b[k])      # noqa: E731
        return m(input_ids=t("input_ids"), attention_mask=t("attention_mask"), class_ids=t("class_ids"), labels=t("labels"), polyphony_bin_ids=t("polyphony_bin_ids"),
                 rhythm_intensity_bin_ids=t("rhythm_intensity_bin_ids"), note_sustain_bin_ids=t("sustain_bin_ids"), pitch_overlap_bin_ids=t("pitch_overlap_bin_ids"),
                 return_dict=True).loss

    out = {}
    m = model()
    batch = tn.ragged_batch(cfg, RAGGED, seed=5, ignore_all=(4,))
    opt = torch.optim.AdamW(m.parameters(), **OPT)
    loss = loss_of(m, batch)
    loss.backward()
    out["loss"] = np.float64(loss.item())
    rng = np.random.default_rng(2024)
    named = dict(m.named_parameters())
    idx = {}
    for k in state:
        p = named[k]
        n = p.numel()
        idx[k] = np.sort(rng.choice(n, size=min(64, n), replace=False))
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out["sample_index/" + k] = idx[k].astype(np.int64)
        out["grad_norm/" + k] = np.float64(g.norm().item())
        out["grad_sample/" + k] = g.reshape(-1)[idx[k]].numpy().copy()
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    for k in state:
        out["param_sample/" + k] = named[k].detach().reshape(-1)[idx[k]].numpy().copy()

    m = model()
    tb = tn.ragged_batch(cfg, (40, 64, 17), seed=21)
    opt = torch.optim.AdamW(m.parameters(), **OPT)
    for _ in range(5):
        opt.zero_grad()
        loss_of(m, tb).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
    out["loss_after_5_steps"] = np.float64(loss_of(m, tb).item())
    np.savez_compressed(HERE / "train_tiny.npz", **out)
    print("wrote", HERE / "train_tiny.npz", (HERE / "train_tiny.npz").stat().st_size, "bytes; loss", out["loss"], "after 5 steps", out["loss_after_5_steps"])


if __name__ == "__main__":
    main()
