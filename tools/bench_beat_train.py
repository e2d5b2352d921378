#!/usr/bin/env python3
"""Measure one optimizer step of etude_amd.BeatTrainer at the default Beat-Transformer (instr 5, 9 layers, d_hid 1024) on ``--batch`` (8) excerpts of ``--frames``
(1024) frames: 40 960 rows.  Not a test and not bench.py.

Median of ``--repeats`` (5) after ``--warmup`` (2) optimizer steps.  Prints one JSON line and, with ``--out``, writes it:
  step_ms                                   wall time of loss_and_backward + step, synchronised (the host-side packing and upload of the batch included)
  forward_ms / backward_ms / optimizer_ms   the library's event profiler (a profiled run of its own)
  workspace_bytes, state_bytes
  torch_autograd_ms                         for orientation only: fp32 torch-ROCm autograd of tests/beat_train_np.py on the same batch and GPU, the same loss at the
                                            trainer's defaults used here (pos_weight 1, tempo_weight 1; every class has scored cells), median of 2 runs after 1
                                            (``--no-torch`` skips it)
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from etude_amd import _lib, synth  # noqa: E402
from etude_amd.beat_train import BeatTrainer  # noqa: E402
from etude_amd.config import BeatDetectorModelConfig  # noqa: E402


def torch_autograd_ms(state, cfg, batch, repeats):
    import beat_train_np as bt
    dev = torch.device("cuda")
    p = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in state.items()}
    b = dict(feats=[torch.as_tensor(f, device=dev) for f in batch["feats"]], beat=[torch.as_tensor(y, device=dev) for y in batch["beat"]],
             tempo=[torch.as_tensor(t, device=dev) for t in batch["tempo"]])
    times = []
    with torch.device(dev):
        for _ in range(repeats + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            outs = [bt.forward(p, f, cfg.nlayers) for f in b["feats"]]
            z, y = torch.cat([o[0] for o in outs]), torch.cat(b["beat"])
            m = y >= 0
            loss = (torch.nn.functional.binary_cross_entropy_with_logits(z, y.clamp(min=0), reduction="none") * m).sum(0).div(m.sum(0)).sum()
            loss = loss + sum(-(t * torch.log_softmax(o[1], -1)).sum() for o, t in zip(outs, b["tempo"])) / len(outs)
            loss.backward()
            torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
            for v in p.values():
                v.grad = None
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import beat_train_np as bt
    cfg = BeatDetectorModelConfig()
    state = synth.beat_state_dict(7, synth.beat_dims())
    batch = bt.make_batch(5, [a.frames] * a.batch, instr=cfg.instr, ntoken=cfg.ntoken)
    tr = BeatTrainer(cfg, state, max_rows=cfg.instr * a.frames * a.batch, max_seqs=a.batch)
    args = (batch["feats"], batch["beat"], batch["tempo"])

    def one():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        losses, norm = tr.train_step([args])
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
    res = dict(config=dict(instr=cfg.instr, layers=cfg.nlayers, d_hid=cfg.d_hid, batch=a.batch, frames=a.frames, rows=cfg.instr * a.frames * a.batch), step_ms=step_ms,
               step_ms_runs=[r[0] for r in runs], loss_first=runs[0][1], loss_last=runs[-1][1], forward_ms=prof.get("btrain_forward", {}).get("ms"),
               backward_ms=prof.get("btrain_backward", {}).get("ms"), optimizer_ms=prof.get("btrain_optimizer", {}).get("ms"), workspace_bytes=tr.workspace_bytes(),
               state_bytes=int(_lib.lib().etd_btrain_bytes(tr.h, 1)))
    tr.close()
    if not a.no_torch:
        res["torch_autograd_ms"] = torch_autograd_ms(state, cfg, batch, 2)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
