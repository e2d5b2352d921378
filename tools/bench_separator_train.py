"""One optimizer step of SeparatorTrainer at the default config (5 instruments, T = 512, F = 1024, stereo), 8 units per instrument: the median of 5 after 2 warm-ups,
split by events into forward (a forward-only call), backward (the forward + backward call minus the forward) and optimizer (Adam + zero_grad).  Prints one JSON line;
the figure beside the time is the fraction of the 157 TFLOP/s fp32-MFMA peak over the convolution FLOPs (forward, input and weight gradients).

    python tools/bench_separator_train.py [--units 8] [--out profiles/separator_train_device.json]

Not measured here: fp32 torch-ROCm autograd of the restatement on the same batch (tests/separator_train_np.py builds its tensors on the host), and any data loading."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from etude_amd.separator import SeparatorConfig  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer  # noqa: E402

PEAK = 157.3e12


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = SeparatorConfig()
    B = args.units
    tr = SeparatorTrainer(cfg, seed=0, max_units=B, workspace_bytes=64 << 30)
    g = torch.Generator().manual_seed(0)
    mix = (torch.rand(B, cfg.T, cfg.F, cfg.n_channels, generator=g) * 2.0).cuda()
    target = (torch.rand(len(cfg.instruments), B, cfg.T, cfg.F, cfg.n_channels, generator=g)).cuda() * mix[None]
    fwd, fb, opt = [], [], []
    for it in range(7):
        f = _timed(lambda: tr.loss(mix, target, frozen_stats=False))
        t = _timed(lambda: tr.loss_and_backward(mix, target))
        o = _timed(tr.step)
        if it >= 2:
            fwd.append(f); fb.append(t); opt.append(o)
    med = statistics.median
    step_ms = med(fb) + med(opt)
    flops = tr.step_flops(B)
    res = {"config": "default", "instruments": len(cfg.instruments), "units_per_instrument": B, "workspace_bytes": tr.workspace_total_bytes(B),
           "forward_ms": round(med(fwd), 3), "backward_ms": round(med(fb) - med(fwd), 3), "optimizer_ms": round(med(opt), 3), "step_ms": round(step_ms, 3),
           "conv_flops": flops, "fraction_of_fp32_mfma_peak": round(flops / (step_ms * 1e-3) / PEAK, 4),
           "not_measured": "fp32 torch-ROCm autograd of the restatement on the same batch; data loading"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    tr.close()


if __name__ == "__main__":
    main()
