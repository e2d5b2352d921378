"""The segment sampler and dropout at the default config (5 instruments, T = 512, F = 1024, stereo), 8 units per batch: the gather kernel's time (the median of 5
after 2 warm-ups, by events), beside one optimizer step of SeparatorTrainer at p = 0 and at p = 0.5 on a gathered batch, measured as tools/bench_separator_train.py
measures it (forward + backward call, then Adam + zero_grad).  Prints one JSON line.

    python tools/bench_separator_data.py [--units 8] [--tracks 2] [--seconds 30] [--out profiles/separator_data_device.json]

The tracks are synthetic noise: the gather's time does not depend on the values.  Not measured here: reading and decoding audio files."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from etude_amd.separator import SeparatorConfig  # noqa: E402
from etude_amd.separator_data import SegmentSampler  # noqa: E402
from etude_amd.separator_train import SeparatorTrainer  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _median(fn, n=5, warm=2):
    return statistics.median([_timed(fn) for _ in range(warm + n)][warm:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=8)
    ap.add_argument("--tracks", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = SeparatorConfig()
    B, I = args.units, len(cfg.instruments)
    sm = SegmentSampler(cfg, seed=0)
    g = torch.Generator().manual_seed(0)
    N = int(args.seconds * cfg.sample_rate)
    add_ms = []
    for _ in range(args.tracks):
        stems = [torch.randn(cfg.n_channels, N, generator=g).cuda() * 0.1 for _ in range(I)]
        add_ms.append(_timed(lambda: sm.add_track(stems)))
    draws = sm.draw(B, 0, 0)
    gather_ms = _median(lambda: sm.batch(draws))
    mix, target = sm.batch(draws)
    out_bytes = (I + 1) * B * cfg.T * cfg.F * cfg.n_channels * 4
    steps = {}
    for p in (0.0, 0.5):
        tr = SeparatorTrainer(cfg, seed=0, max_units=B, workspace_bytes=64 << 30, dropout=p)
        fb, opt = [], []
        for it in range(7):
            t = _timed(lambda: tr.loss_and_backward(mix, target))
            o = _timed(tr.step)
            if it >= 2:
                fb.append(t); opt.append(o)
        steps[p] = round(statistics.median(fb) + statistics.median(opt), 3)
        tr.close()
    res = {"config": "default", "instruments": I, "units": B, "tracks": args.tracks, "track_seconds": args.seconds, "held_bytes": sm.held_bytes,
           "add_track_ms": round(statistics.median(add_ms), 3), "gather_ms": round(gather_ms, 4), "gather_output_bytes": out_bytes,
           "gather_output_GBps": round(out_bytes / (gather_ms * 1e-3) / 1e9, 1), "step_ms_p0": steps[0.0], "step_ms_p05": steps[0.5],
           "gather_share_of_step_p0": round(gather_ms / steps[0.0], 5),
           "not_measured": "reading and decoding audio files"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    sm.close()


if __name__ == "__main__":
    main()
