"""BSS Eval on one track: 5 stereo stems of 3 minutes at 44.1 kHz, 512-tap filters, 1-second windows.  The whole call (the median of 5 after 2
warm-ups, by events) and, in a second set of timed runs, its stages by the library's own events (correlations, factorisations, substitutions, projections, energies),
with the achieved fp64 TFLOP/s of the two GEMM stages from their flop counts: 4 S^2 L N for the correlations, 2 (W + L - 1) (S L) (2 S) per window for the
projections (the block-diagonal B counted as stored).  Prints one JSON line.

    python tools/bench_bss.py [--seconds 180] [--sources 5] [--taps 512] [--host-seconds 30 --host-taps 32] [--out profiles/bss_device.json]

The track is synthetic coloured noise: the times do not depend on the values.  As information only: the wall time of the fp64 numpy restatement (tests/bss_np.py) on
a --host-seconds track at --host-taps taps (0 skips it).  No fp64 matrix-core peak is measured here, so no fraction of peak is quoted."""
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
from etude_amd.bss import BSSEval, BSSEvalConfig  # noqa: E402


def _track(J, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(J, C, N, generator=g).cuda()
    ref[:, :, 1:] += 0.5 * ref[:, :, :-1]
    mix = torch.eye(J, device="cuda") + 0.2 * torch.randn(J, J, generator=g).cuda()
    est = torch.einsum("ij,jcn->icn", mix, ref) + 0.05 * torch.randn(J, C, N, generator=g).cuda()
    return (0.1 * ref).contiguous(), (0.1 * est).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sources", type=int, default=5)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--host-seconds", type=float, default=30.0)
    ap.add_argument("--host-taps", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    J, C, L, N = args.sources, args.channels, args.taps, int(args.seconds * args.rate)
    S = J * C
    eng = BSSEval(BSSEvalConfig(filters_len=L, window=args.rate, hop=args.rate))
    ref, est = _track(J, C, N, 0)
    whole = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = eng.energies_many([ref], [est])[0]
        b.record()
        b.synchronize()
        whole.append(a.elapsed_time(b))
    eng.timing(True)
    stages = []
    for _ in range(7):
        eng.energies_many([ref], [est])
        stages.append(eng.timing(True))
    eng.timing(False)
    st = np.median(np.array(stages[2:]), axis=0)
    bounds = eng.window_bounds(N)
    flop_corr = 4.0 * S * S * L * N
    flop_proj = sum(2.0 * (b - a + L - 1) * (S * L) * (2 * S) for a, b in bounds)
    m = eng.evaluate_many([ref], [est])[0]
    out = {"track": {"sources": J, "channels": C, "seconds": args.seconds, "rate": args.rate, "taps": L, "windows": len(bounds)},
           "workspace_bytes": eng.workspace_bytes(J, C, N), "status": res["status"], "call_ms": round(statistics.median(whole[2:]), 2),
           "stage_ms": dict(zip(("correlations", "factorisations", "substitutions", "projections", "energies"), [round(float(x), 3) for x in st])),
           "correlations_TFLOPs": round(flop_corr / (st[0] * 1e-3) / 1e12, 3), "projections_TFLOPs": round(flop_proj / (st[3] * 1e-3) / 1e12, 3),
           "flop": {"correlations": flop_corr, "projections": flop_proj, "cholesky": (S * L) ** 3 / 3.0 + J * (C * L) ** 3 / 3.0},
           "median_sdr_dB": [round(float(x), 3) for x in m["scores"]["sdr"]]}
    if args.host_seconds > 0:
        sys.path.insert(0, str(ROOT / "tests"))
        import bss_np
        n = int(args.host_seconds * args.rate)
        hr, he = ref[:, :, :n].cpu().numpy(), est[:, :, :n].cpu().numpy()
        t0 = time.time()
        bss_np.evaluate(hr, he, args.host_taps, args.rate, args.rate)
        out["host_restatement"] = {"seconds_of_audio": args.host_seconds, "taps": args.host_taps, "wall_s": round(time.time() - t0, 2)}
    print(json.dumps(out))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
