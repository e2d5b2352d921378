"""Warping Path Deviation, the audio-based metric of evaluate.py: ``WPDCalculator`` stands in for etude.evaluation.metrics.wpd.WPDCalculator
(etude/evaluation/metrics/wpd.py; EvaluationRunner calls it once per (song, version), etude/evaluation/runner.py:73-87).

The metric is host arithmetic on a warping path: a line fitted to (cover time, origin time) along the path, and the standard deviation of the path's distance from
it.  The path comes from ``etude_amd.aligner`` (csrc/dtw.hip); ``wpd_many`` scores a batch of its results.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np


class WPDCalculator:
    def __init__(self, subsample_step: int = 1, trim_seconds: float = 0, **kwargs):
        if not isinstance(subsample_step, int) or subsample_step < 1:
            raise ValueError("subsample_step must be an integer >= 1.")
        if not isinstance(trim_seconds, (int, float)) or trim_seconds < 0:
            raise ValueError("trim_seconds must be a number >= 0.")
        self.subsample_step = subsample_step
        self.trim_seconds = trim_seconds

    def calculate(self, align_result: Dict, feature_rate: int = 50) -> Dict:
        """-> {"wpd_score": sigma} or {"error": message}, as wpd.py:32-95"""
        try:
            wp = align_result.get("wp")
            n_cover = align_result.get("num_frames_cover")
            n_origin = align_result.get("num_frames_origin")
            if wp is None or n_cover is None or n_origin is None:
                return {"error": "Alignment result is missing required keys ('wp', 'num_frames_cover', 'num_frames_origin')."}
            t_cover = np.arange(n_cover) / feature_rate
            t_origin = np.arange(n_origin) / feature_rate
            sub = wp[:, ::self.subsample_step]
            if sub.shape[1] < 10:
                return {"error": "Not enough points after subsampling."}
            x = t_cover[np.clip(sub[0], 0, n_cover - 1)]
            y = t_origin[np.clip(sub[1], 0, n_origin - 1)]
            if self.trim_seconds > 0 and y[-1] > (2 * self.trim_seconds):
                mask = (y >= self.trim_seconds) & (y <= y[-1] - self.trim_seconds)
                if np.sum(mask) > 10:
                    x, y = x[mask], y[mask]
            a, b = np.polyfit(x, y, 1)[:2]
            return {"wpd_score": np.std(y - (a * x + b))}
        except Exception as e:      # noqa: BLE001  (the reference reports any failure as an error dict)
            return {"error": str(e)}


def wpd_many(align_results: Sequence[Optional[Dict]], subsample_step: int = 1, trim_seconds: float = 0, feature_rate: int = 50) -> List[Dict]:
    """One WPD dict per alignment result (None -> the missing-keys error dict), e.g. over ``align_features_many``'s output for the covers of ``generate_many``."""
    calc = WPDCalculator(subsample_step=subsample_step, trim_seconds=trim_seconds)
    return [calc.calculate(r if r is not None else {}, feature_rate) for r in align_results]
