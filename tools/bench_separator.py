"""Time the source separator on one 3-minute stereo song at the default config and write profiles/separator_device.json.

    python tools/bench_separator.py [--seconds 180] [--runs 5] [--warmup 2] [--test-log LOG] [--out profiles/separator_device.json]
    python tools/bench_separator.py --mwf 1 [--out profiles/separator_mwf.json]

Median wall time of ``StemSeparator.separate_many`` (synchronised) over the runs, then one profiled run for the per-kernel split (the library's event profiler).
--test-log: the output of ``pytest tests/test_gpu_separator.py -s``; its SEP_ERR lines give the largest device / yardstick error ratio of every stage.
The weights are random (``init_separator_state``): the time does not depend on their values.
--mwf N: the same song with N passes of multichannel Wiener filtering against the same engine with the filter off, the two timed in alternation;
writes the added time per iteration, each k_mwf_* kernel's time and its algorithmic bytes over that time as a share of the 8 TB/s HBM peak."""
import argparse
import json
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_FP32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


def error_ratios(log: Path) -> dict:
    out = {}
    for m in re.finditer(r"SEP_ERR (\w+)[^:]*: device (\S+) yardstick (\S+) ratio (\S+)", log.read_text()):
        stage, ratio = m.group(1), float(m.group(4))
        out[stage] = max(out.get(stage, 0.0), ratio)
    return out


def timed(sep, wav, mwf=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sep.separate_many([wav], mwf_iterations=mwf) if mwf is not None else sep.separate_many([wav])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_mwf(a, sep, cfg, wav, N) -> dict:
    """off and on in alternation (one process, one engine, one song), then one profiled run with the filter on"""
    from etude_amd import _lib
    off, on = [], []
    for i in range(a.warmup + a.runs):
        t_off, _ = timed(sep, wav, 0)
        t_on, out = timed(sep, wav, a.mwf)
        if i >= a.warmup:
            off.append(t_off); on.append(t_on)
    assert bool(torch.isfinite(out[0]).all())
    _lib.prof_enable(True)
    _lib.prof_reset()
    timed(sep, wav, a.mwf)
    prof = _lib.prof_report()
    _lib.prof_enable(False)
    Tf, I, C, F = sep.num_frames(N), len(cfg.instruments), cfg.n_channels, cfg.F
    y_bytes, x_bytes = I * C * Tf * F * 8, C * Tf * F * 8
    chunks = -(-Tf // 64)
    # what each kernel must move, per launch: stats reads Y and writes the chunk partials; reduce reads them; apply reads X and Y and writes Y; scale reads X once per song
    algo = {"k_mwf_scale": x_bytes, "k_mwf_stats": y_bytes + chunks * I * F * (C * C + 1) * 8, "k_mwf_reduce": chunks * I * F * (C * C + 1) * 8 + I * F * C * C * 8,
            "k_mwf_apply": 2 * y_bytes + x_bytes}
    kernels = {}
    for k, v in sorted(prof.items()):
        if k.startswith("k_mwf"):
            per = v["ms"] / v["launches"]
            kernels[k] = {"ms": v["ms"], "launches": v["launches"], "ms_per_launch": per, "algorithmic_bytes_per_launch": algo[k],
                          "share_of_hbm_peak": algo[k] / (per * 1e-3) / PEAK_HBM}
    med_off, med_on = statistics.median(off), statistics.median(on)
    it_bytes = 3 * y_bytes + x_bytes
    kern_ms_it = sum(v["ms"] for k, v in kernels.items() if k != "k_mwf_scale") / a.mwf
    return {
        "what": f"StemSeparator.separate_many with mwf_iterations = {a.mwf} against 0, one stereo song, default config, random weights, timed in alternation",
        "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), "seconds_of_audio": a.seconds, "samples": N, "frames": Tf,
        "runs": a.runs, "warmup": a.warmup, "mwf_iterations": a.mwf, "median_off_s": med_off, "median_on_s": med_on, "all_off_s": off, "all_on_s": on,
        "added_ms_per_iteration_over_wall": (med_on - med_off) * 1e3 / a.mwf, "kernel_ms_per_iteration": kern_ms_it,
        "algorithmic_bytes_per_iteration": it_bytes, "iteration_share_of_hbm_peak_over_kernel_time": it_bytes / (kern_ms_it * 1e-3) / PEAK_HBM if kern_ms_it else None,
        "kernels": kernels, "workspace_bytes_off": sep.workspace_total_bytes([N]),
        "not_measured": ["hardware counters", "other song lengths, batches and instrument counts", "mono", "a trained checkpoint"],
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--test-log", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "separator_device.json")
    ap.add_argument("--mwf", type=int, default=0, help="time N passes of multichannel Wiener filtering against none (default --out: profiles/separator_mwf.json)")
    a = ap.parse_args()
    if a.mwf and a.out == ROOT / "profiles" / "separator_device.json":
        a.out = ROOT / "profiles" / "separator_mwf.json"
    from etude_amd import _lib
    from etude_amd.separator import SeparatorConfig, StemSeparator
    cfg = SeparatorConfig()
    sep = StemSeparator(cfg, seed=0)
    N = int(a.seconds * cfg.sample_rate)
    r = np.random.default_rng(0)
    t = np.arange(N) / cfg.sample_rate
    wav = torch.from_numpy(np.stack([0.3 * np.sin(2 * np.pi * 220.0 * (c + 1) * t) + 0.1 * r.standard_normal(N) for c in range(2)]).astype(np.float32)).cuda()
    if a.mwf:
        res = bench_mwf(a, sep, cfg, wav, N)
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
        return
    times = []
    for i in range(a.warmup + a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sep.separate_many([wav])
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(time.perf_counter() - t0)
    assert bool(torch.isfinite(out[0]).all())
    _lib.prof_enable(True)
    _lib.prof_reset()
    sep.separate_many([wav])
    torch.cuda.synchronize()
    prof = _lib.prof_report()
    _lib.prof_enable(False)
    Tf = sep.num_frames(N)
    segs = -(-Tf // cfg.T)
    flops = sep.segment_flops() * segs
    med = statistics.median(times)
    conv_ms = sum(v["ms"] for k, v in prof.items() if k in ("k_sep_conv", "k_sep_deconv", "k_sep_head"))
    res = {
        "what": "StemSeparator.separate_many, one stereo song, default config, random weights",
        "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), "seconds_of_audio": a.seconds, "samples": N, "frames": Tf, "segments": segs,
        "runs": a.runs, "warmup": a.warmup, "median_s": med, "all_s": times,
        "unet_flops": flops, "unet_tflops_over_wall": flops / med / 1e12, "share_of_fp32_mfma_peak_over_wall": flops / med / PEAK_FP32_MFMA,
        "unet_tflops_over_kernel_time": flops / (conv_ms * 1e-3) / 1e12 if conv_ms else None,
        "share_of_fp32_mfma_peak_over_kernel_time": flops / (conv_ms * 1e-3) / PEAK_FP32_MFMA if conv_ms else None,
        "unit_bytes": sep.unit_bytes, "workspace_bytes": sep.workspace_total_bytes([N]),
        "kernels_ms": {k: {"ms": v["ms"], "launches": v["launches"]} for k, v in sorted(prof.items()) if k.startswith("k_sep")},
        "not_measured": ["hardware counters", "other song lengths and batches", "a trained checkpoint"],
    }
    if a.test_log and a.test_log.exists():
        res["largest_error_ratio_device_over_fp32_yardstick"] = error_ratios(a.test_log)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
