"""beat_pred.json -> tempo.json: ``BeatAnalyzer`` <- etude.data.beat_analyzer.BeatAnalyzer, ``structuralize_many`` (detect_many + analyze_data) and
``structuralize_stems_many`` (the same from separated stems).

Host Python with no hot path (a few hundred beats per song).  The behaviour is the reference class's, restated: the same float operations in the same order (numpy's
diff / mean / std on the same lists), so that the regions agree to the last bit (tests/test_beat_analyzer_cpu.py against the reference's own output).  The steps,
with the reference's defaults:

  1. drop every beat closer than 0.1 s to a downbeat;
  2. a measure per pair of consecutive downbeats: its beats (the downbeat + the beats strictly inside), uniform when std / mean of their spacing is below 0.1;
  3. the song's time signature: the most common beat count of the uniform measures (first seen wins ties), 4 when fewer than 10 are uniform, and 2 reads as 4;
  4. stable regions: a window of 4 measures whose 3 spacings have a standard deviation below 0.1 s, extended while the next downbeat falls within 0.1 s of the
     prediction from the window's mean spacing;
  5. per region the mean measure duration and bpm = 60 * time_sig / duration;
  6. the gap between two regions is filled with N copies of a measure when it is within 0.25 of N >= 1 measures, or N measures and a 2-beat half measure when
     within 0.25 of N + 0.5; then neighbours with the same time signature and less than 1 bpm apart merge.
"""
from __future__ import annotations

import json
import logging
import math
from collections import Counter
from pathlib import Path
from typing import Dict, List, Sequence, Union

import numpy as np

log = logging.getLogger(__name__)

CLOSE_BEAT_S = 0.1
UNIFORMITY = 0.1
WINDOW = 4
STABLE_S = 0.1
GAP_TOLERANCE = 0.25
MERGE_BPM = 1.0
MIN_UNIFORM_MEASURES = 10


class BeatAnalyzer:
    def __init__(self):
        self.beat_pred: List[float] = []
        self.downbeat_pred: List[float] = []

    # ------------------------------------------------------------------ entry points
    def analyze(self, beat_file_path: Union[str, Path]) -> List[Dict]:
        with open(beat_file_path, "r", encoding="utf-8") as f:
            return self.analyze_data(json.load(f))

    def analyze_data(self, data: Dict) -> List[Dict]:
        """{"beat_pred": [...], "downbeat_pred": [...]} (what BeatDetector.detect returns) -> tempo.json content"""
        self.beat_pred = data.get("beat_pred", [])
        self.downbeat_pred = data.get("downbeat_pred", [])
        if not self.downbeat_pred:
            log.warning("no downbeats: no tempo analysis")
            return []
        measures = self._measures(self._beats_away_from_downbeats())
        if not measures:
            log.warning("no measures")
            return []
        time_sig = self._time_signature(measures)
        regions = []
        for lo, hi in self._stable_spans(measures):
            downbeats = [m["start"] for m in measures[lo:hi + 1]]
            if hi + 1 < len(measures):
                downbeats.append(measures[hi + 1]["start"])
            durations = [downbeats[k + 1] - downbeats[k] for k in range(len(downbeats) - 1)]
            if not durations:
                continue
            mean_duration = sum(durations) / len(durations)
            regions.append({"start_time": downbeats[0], "downbeats": downbeats[:-1], "avg_duration": mean_duration,
                            "bpm": (60 * time_sig) / mean_duration if mean_duration > 0 else 0, "time_sig": time_sig})
        if not regions:
            log.warning("no stable tempo region")
            return []
        return [{"time_sig": r["time_sig"], "bpm": r["bpm"], "start": r["start_time"], "downbeats": r["downbeats"]} for r in self._fill_gaps_and_merge(regions)]

    def save_tempo_data(self, tempo_data: List[Dict], output_path: Union[str, Path]) -> None:
        output_path = Path(output_path)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        with open(output_path, "w", encoding="utf-8") as f:
            json.dump(tempo_data, f, indent=4)

    # ------------------------------------------------------------------ steps
    def _beats_away_from_downbeats(self) -> List[float]:
        return [b for b in self.beat_pred if not any(abs(b - d) < CLOSE_BEAT_S for d in self.downbeat_pred)]

    def _measures(self, beats: Sequence[float]) -> List[Dict]:
        out = []
        for start, end in zip(self.downbeat_pred[:-1], self.downbeat_pred[1:]):
            inside = [start] + [b for b in beats if start < b < end]
            uniform = True
            if len(inside) > 1:
                spacing = np.diff(inside)
                mean = np.mean(spacing)
                if mean > 0:
                    uniform = bool(np.std(spacing) / mean < UNIFORMITY)
            out.append({"start": start, "raw_beats": len(inside), "duration": end - start, "uniform": uniform})
        return out

    @staticmethod
    def _time_signature(measures: Sequence[Dict]) -> int:
        counts = [m["raw_beats"] for m in measures if m["uniform"]]
        if len(counts) < MIN_UNIFORM_MEASURES:
            return 4
        most = Counter(counts).most_common(1)[0][0]          # (first seen wins ties, as statistics.mode)
        return 4 if most == 2 else most

    @staticmethod
    def _stable_spans(measures: Sequence[Dict]) -> List[tuple]:
        starts = [m["start"] for m in measures]
        spans, i = [], 0
        while i <= len(starts) - WINDOW:
            spacing = [starts[j + 1] - starts[j] for j in range(i, i + WINDOW - 1)]
            if not spacing or np.std(spacing) >= STABLE_S:
                i += 1
                continue
            ideal = np.mean(spacing)
            end = i + WINDOW - 1
            while end + 1 < len(starts) and abs(starts[end + 1] - (starts[end] + ideal)) < STABLE_S:
                end += 1
            spans.append((i, end))
            i = end + 1
        return spans

    @staticmethod
    def _fill_gaps_and_merge(regions: List[Dict]) -> List[Dict]:
        if len(regions) < 2:
            return regions
        filled = []
        for cur, nxt in zip(regions[:-1], regions[1:]):
            filled.append(cur)
            duration = cur["avg_duration"]
            expected_end = cur["downbeats"][-1] + duration
            gap = nxt["downbeats"][0] - expected_end
            if duration <= 0 or gap < 0:
                continue
            ratio = gap / duration
            whole, half = 0, False
            if abs(ratio - round(ratio)) < GAP_TOLERANCE and round(ratio) >= 1:
                whole = round(ratio)
            elif abs(ratio - (math.floor(ratio) + 0.5)) < GAP_TOLERANCE:
                whole, half = math.floor(ratio), True
            at = expected_end
            for _ in range(whole):
                filled.append({"time_sig": cur["time_sig"], "bpm": cur["bpm"], "start_time": at, "downbeats": [at], "avg_duration": duration})
                at += duration
            if half:
                filled.append({"time_sig": 2, "bpm": cur["bpm"], "start_time": at, "downbeats": [at], "avg_duration": duration / 2})
        filled.append(regions[-1])
        merged: List[Dict] = []
        for r in filled:
            if merged and merged[-1]["time_sig"] == r["time_sig"] and abs(merged[-1]["bpm"] - r["bpm"]) < MERGE_BPM:
                merged[-1]["downbeats"].extend(r["downbeats"])
            else:
                merged.append(r)
        return merged


def structuralize_many(detector, features_list: Sequence) -> List[List[Dict]]:
    """stage 2 of infer.py for many songs: ``detector.detect_many`` (native trackers) then ``BeatAnalyzer.analyze_data`` -> one tempo.json content per song"""
    return [BeatAnalyzer().analyze_data(r) for r in detector.detect_many(features_list)]


def structuralize_stems_many(detector, stems_list: Sequence, stem_features=None) -> List[List[Dict]]:
    """the same from the songs' separated stems [instr][channels][N]: ``detector.detect_stems_many`` (features, model and trackers on the device) then ``analyze_data``"""
    return [BeatAnalyzer().analyze_data(r) for r in detector.detect_stems_many(stems_list, stem_features=stem_features)]


def structuralize_audio_many(detector, separator, wavs: Sequence) -> List[List[Dict]]:
    """the same from the songs' audio [channels][N]: ``detector.detect_audio_many`` (separator, features, model and trackers on the device) then ``analyze_data``"""
    return [BeatAnalyzer().analyze_data(r) for r in detector.detect_audio_many(separator, wavs)]


def structuralize_files_many(detector, separator, paths: Sequence, loader=None) -> List[List[Dict]]:
    """the same from WAV files of any rate: loaded on the device at the separator's rate (``etude_amd.audio``), as the mean of their channels for a
    1-channel separator, else with the channels they have (the separator duplicates a mono file).  loader: an ``AudioLoader`` (default: one per device, made once)"""
    if loader is None:
        from .audio import default_audio_loader
        loader = default_audio_loader(separator.device)
    wavs = loader.load_many(paths, separator.config.sample_rate, mono=separator.config.n_channels == 1)
    return structuralize_audio_many(detector, separator, wavs)
