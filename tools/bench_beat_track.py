#!/usr/bin/env python3
"""Time the native DBN trackers: 64 songs x 7 752 frames (3 min at 44100 / 1024 fps) at BeatDetector's default config.

Reports, per batch and per frame-step (one Viterbi step of every song and HMM = batch time / frames per song): tracking alone on device-resident activations
(etd_dbn_track: trimming + densities, Viterbi of the beat, 3-beat and 4-beat HMMs, backtracking, peak picking, one copy back), the Beat-Transformer forward pass of
the same batch, and detect_many end to end (features on the host -> beat times).  For context only: the numpy restatement's time on the host for ONE song.
Warm-up runs precede every timed window and each figure is the median of `--repeats` windows that end in a device synchronise.

Usage:  python tools/bench_beat_track.py [--songs 64] [--frames 7752] [--repeats 5] [--out profiles/beat_track.json]
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
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=7752)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-model", action="store_true", help="tracking only (no Beat-Transformer pass, no detect_many)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beat_track needs a ROCm GPU: there is no CPU path and no CPU timing stands in for it")
    from etude_amd import BeatDetector, dbn, synth
    fps = 44100 / 1024
    n, T = a.songs, a.frames
    acts = [synth.beat_activations(500 + i, T, ((None, 90.0 + 1.5 * i),), 3 + i % 2, jitter=0.004)[0] for i in range(n)]
    eng = dbn.DBNEngine(fps, 70.0, 250.0, 0.2, [3, 4])
    x = torch.from_numpy(np.concatenate(acts)).cuda()
    Ts = [T] * n
    res = {}
    out = eng.track(x, Ts)
    beats = sum(len(b) for b, _, _ in out)
    med, lo, hi = timed(lambda: eng.track(x, Ts), a.repeats)
    res["track_ms_per_batch"] = dict(median=med, min=lo, max=hi)
    res["track_us_per_frame_step"] = med * 1e3 / T
    res["beats_found"] = beats
    one = eng.track(x[:T].contiguous(), [T])
    med1, lo1, hi1 = timed(lambda: eng.track(x[:T].contiguous(), [T]), a.repeats)
    res["track_ms_one_song"] = dict(median=med1, min=lo1, max=hi1)
    if not a.skip_model:
        det = BeatDetector(state_dict=synth.beat_state_dict(7), tracker="native")
        feats = [synth.beat_features(900 + i % 4, T) for i in range(n)]
        feat_dev, _ = det._songs_to_device(feats)
        medf, lof, hif = timed(lambda: det._run(feat_dev, Ts, want_tempo=False), a.repeats, warmup=1)
        res["forward_ms_per_batch"] = dict(median=medf, min=lof, max=hif)
        logits, _ = det._run(feat_dev, Ts, want_tempo=False)
        act = torch.sigmoid(logits).contiguous()
        medm, lom, him = timed(lambda: det._native().track(act, Ts), a.repeats)
        res["track_model_activations_ms_per_batch"] = dict(median=medm, min=lom, max=him)
        mede, loe, hie = timed(lambda: det.detect_many(feats), max(2, a.repeats // 2), warmup=1)
        res["detect_many_ms_per_batch"] = dict(median=mede, min=loe, max=hie)
        res["tracking_not_slower_than_forward"] = bool(max(med, medm) <= medf)
    import dbn_np
    cfg = dbn_np.TrackerCfg(fps=fps, min_bpm=70.0, max_bpm=250.0, threshold=0.2, beats_per_bar=(3, 4))
    t0 = time.perf_counter()
    rb = dbn_np.track_beats(acts[0][:, 0], cfg)
    rr, _ = dbn_np.track_downbeats(dbn_np.combined(acts[0][:, 0], acts[0][:, 1]), cfg)
    res["host_restatement_s_one_song"] = time.perf_counter() - t0
    res["one_song_equals_restatement"] = bool(np.array_equal(one[0][0], rb) and np.array_equal(one[0][1], rr))
    res.update(songs=n, frames=T, device=torch.cuda.get_device_name(0), barriers_per_frame_step=1)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
