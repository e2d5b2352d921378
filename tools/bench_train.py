#!/usr/bin/env python3
"""Measure one optimizer step of etude_amd.DecoderTrainer at the reference's default decoder (hidden 512, 8 layers, 2 048 intermediate, 1 024 positions, the goldens'
vocabulary) on batches of 8 full-length sequences.  Not a test and not bench.py.

Median of ``--repeats`` (5) after ``--warmup`` (2) optimizer steps of ``--accum`` (1) batches each.  Prints one JSON line and, with ``--out``, writes it:
  step_ms                                   wall time of loss_and_backward x accum + step, synchronised
  forward_ms / backward_ms / optimizer_ms   the library's event profiler (a profiled run of its own: the events serialise nothing but are not free)
  mfma_fraction                             model FLOPs of the linear layers (6 x rows x weights) + attention / step time / 157 TFLOP/s, the fp32-MFMA peak gemm3.h quotes
  workspace_bytes, state_bytes
  torch_autograd_ms                         for orientation only: fp32 torch-ROCm autograd of oracle/neox.py on the same batch and GPU (``--no-torch`` skips it)
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from etude_amd import _lib, synth  # noqa: E402
from etude_amd.decoder import EtudeDecoderConfig  # noqa: E402
from etude_amd.train import DecoderTrainer  # noqa: E402

PEAK_FP32_MFMA = 157e12


def make_batch(cfg, B, T, seed):
    rng = np.random.default_rng(seed)
    b = {"input_ids": rng.integers(1, cfg.vocab_size, (B, T)), "attention_mask": np.ones((B, T), np.int64), "class_ids": rng.integers(1, cfg.num_classes, (B, T)),
         "labels": rng.integers(0, cfg.vocab_size, (B, T))}
    b["labels"][:, : T // 4] = -100
    for k in ("polyphony_bin_ids", "rhythm_intensity_bin_ids", "sustain_bin_ids", "pitch_overlap_bin_ids"):
        b[k] = rng.integers(0, cfg.num_attribute_bins, (B, T))
    return b


def model_flops(cfg, B, T):
    H, I, L, V, E = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size, cfg.attribute_emb_dim
    weights = L * (4 * H * H + 2 * H * I) + V * H + 4 * E * H
    linear = 6.0 * B * T * weights                                   # forward + two backward products per weight
    attn = L * B * (T * (T + 1) / 2) * H * 2 * (2 + 5)               # causal pairs x (QK^T, PV) forward; 5 products backward (P recomputed twice: 7 in this engine)
    return linear, attn


def torch_autograd_ms(cfg, state, batch, repeats):
    from oracle import neox
    dev = torch.device("cuda")
    sd = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in state.items()}
    d = neox.NeoxDims(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                      intermediate_size=cfg.intermediate_size, max_position_embeddings=cfg.max_position_embeddings, attribute_emb_dim=cfg.attribute_emb_dim)
    t = {k: torch.as_tensor(v, device=dev) for k, v in batch.items()}
    times = []
    with torch.device(dev):                                          # the oracle builds its position / mask tensors on the default device
        for _ in range(repeats + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loss = 0
            for i in range(t["input_ids"].shape[0]):
                s = lambda k: t[k][i][None]                          # noqa: E731
                attrs = {"pitch_overlap": s("pitch_overlap_bin_ids"), "polyphony": s("polyphony_bin_ids"), "note_sustain": s("sustain_bin_ids"),
                         "rhythm_intensity": s("rhythm_intensity_bin_ids")}
                h, _ = neox.transformer(sd, neox.embed(sd, s("input_ids"), s("class_ids"), attrs), d)
                lg = torch.nn.functional.linear(h, sd["lm_head.weight"])[0]
                loss = loss + torch.nn.functional.cross_entropy(lg, t["labels"][i], reduction="sum")
            loss.backward()
            torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
            for p in sd.values():
                p.grad = None
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--accum", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    cfg = EtudeDecoderConfig(**synth.decoder_dims())
    B, T = a.batch, cfg.max_position_embeddings
    state = synth.decoder_state_dict(1, {})
    tr = DecoderTrainer(cfg, state, grad_accum_steps=a.accum, max_rows=B * T)
    batches = [make_batch(cfg, B, T, 100 + i) for i in range(a.accum)]

    def one():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        losses, norm = tr.train_step(batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, losses[0]
    for _ in range(a.warmup):
        one()
    runs = [one() for _ in range(a.repeats)]
    step_ms = statistics.median(r[0] for r in runs)
    _lib.prof_enable(True); _lib.prof_reset()
    one()
    prof = _lib.prof_report()
    _lib.prof_enable(False)
    linear, attn = model_flops(cfg, B * a.accum, T)
    res = dict(config=dict(hidden=cfg.hidden_size, layers=cfg.num_hidden_layers, intermediate=cfg.intermediate_size, positions=T, vocab=cfg.vocab_size, batch=B,
                           accum=a.accum), step_ms=step_ms, step_ms_runs=[r[0] for r in runs], loss_first=runs[0][1], loss_last=runs[-1][1],
               forward_ms=prof.get("dtrain_forward", {}).get("ms"), backward_ms=prof.get("dtrain_backward", {}).get("ms"),
               optimizer_ms=prof.get("dtrain_optimizer", {}).get("ms"), linear_flops=linear, attention_flops=attn,
               mfma_fraction=linear / (step_ms * 1e-3) / PEAK_FP32_MFMA, workspace_bytes=tr.workspace_bytes(), state_bytes=int(_lib.lib().etd_dtrain_bytes(tr._h, 1)))
    tr.close()
    if not a.no_torch:
        res["torch_autograd_ms"] = torch_autograd_ms(cfg, state, batches[0], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
