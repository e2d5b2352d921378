"""Volume contour of stage 1 (infer.py:99-104) -- drop-in for etude/utils/preprocess.py:116-166.

``analyze_volume`` = librosa.load(sr=22050, mono) + librosa.feature.rms(frame = 2 * hop, hop = sr // resolution, zero-padded
centre frames) + min-max normalisation.  Here: the clip is averaged to mono and resampled on the GPU by the Extract stage's
polyphase sinc resampler (csrc/frontend.hip), the frame energies come from ``k_rms_frames``.

PARITY UNPINNED: librosa resamples with the third-party soxr library ("soxr_hq"), which is neither in /root/reference nor in
this image; a different band-limited resampler changes individual samples in the 4th digit and a 2 204-sample RMS far
less.  The oracle (oracle/mel.py: volume_contour) restates the same steps with the torchaudio-style resampler.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Union

import numpy as np
import torch

from . import _lib
from .extractor import read_wav
from .frontend import FrontEnd


class VolumeAnalyzer:
    """`volume_contour_tensor` for many clips of one sample rate: the resampler tables are built once (batch serving)."""

    def __init__(self, sr_in: int, sr: int = 22050, resolution: int = 20, device="cuda"):
        self.dev = torch.device(device)
        self.sr, self.resolution = int(sr), int(resolution)
        with torch.cuda.device(self.dev):
            self.fe = FrontEnd(int(sr_in), sr_out=int(sr), pad_mode="constant")

    def __call__(self, wave: Union[np.ndarray, torch.Tensor]) -> np.ndarray:
        w = torch.as_tensor(wave, dtype=torch.float32)
        if w.dim() == 1:
            w = w[None]
        w = w.to(self.dev).contiguous()
        with torch.cuda.device(self.dev):
            y = self.fe.resample(w)                         # mono mean + resample (no spectrogram: librosa.load does neither)
            hop = self.sr // self.resolution
            T = 1 + y.numel() // hop
            out = torch.empty(T, dtype=torch.float32, device=self.dev)
            st = torch.cuda.current_stream(self.dev).cuda_stream
            _lib.check(_lib.lib().etd_rms_frames(y.data_ptr(), y.numel(), 2 * hop, hop, out.data_ptr(), T, C.c_void_p(st)), "etd_rms_frames")
            rms = out.cpu().numpy()
        if rms.size and rms.max() > rms.min():
            return (rms - rms.min()) / (rms.max() - rms.min())
        return np.zeros_like(rms)

    def close(self):
        self.fe.close()


def volume_contour_tensor(wave: Union[np.ndarray, torch.Tensor], sr_in: int, sr: int = 22050, resolution: int = 20, device="cuda") -> np.ndarray:
    """[C, L] (or [L]) float32 audio -> normalised RMS contour, float32 [1 + L_resampled // hop]."""
    dev = torch.device(device)
    w = torch.as_tensor(wave, dtype=torch.float32)
    if w.dim() == 1:
        w = w[None]
    w = w.to(dev).contiguous()
    with torch.cuda.device(dev):
        fe = FrontEnd(int(sr_in), sr_out=int(sr), pad_mode="constant")
        y = fe.resample(w)                                  # mono mean + resample (no spectrogram)
        hop = int(sr) // int(resolution)
        frame = 2 * hop
        T = 1 + y.numel() // hop
        out = torch.empty(T, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().etd_rms_frames(y.data_ptr(), y.numel(), frame, hop, out.data_ptr(), T, C.c_void_p(st)), "etd_rms_frames")
        rms = out.cpu().numpy()
        fe.close()
    if rms.size and rms.max() > rms.min():
        return (rms - rms.min()) / (rms.max() - rms.min())
    return np.zeros_like(rms)


def analyze_volume(audio_path: Union[str, Path], sr: int = 22050, resolution: int = 20) -> np.ndarray:
    """Signature of etude/utils/preprocess.py:116-120."""
    if not Path(audio_path).exists():
        raise FileNotFoundError(f"Audio file not found at: {audio_path}")
    wave, sr_in = read_wav(audio_path)
    return volume_contour_tensor(wave, sr_in, sr, resolution)


def save_volume_map(volume_map: np.ndarray, output_path: Union[str, Path]):
    """etude/utils/preprocess.py:154-166."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "w") as f:
        json.dump(np.asarray(volume_map).tolist(), f)


# ---- stage 3 host functions (etude/utils/preprocess.py:14-114): the reference's float operations in the same order, scipy's interp1d restated with numpy

def compute_wp_std(time_map: list) -> float:
    """etude/utils/preprocess.py:14-19 (WP-Std of Music2MIDI): the standard deviation of origin time - cover time over the map; inf for an empty map."""
    if not time_map:
        return float("inf")
    return np.std([pair[0] - pair[1] for pair in time_map])


def _interp_linear(x: np.ndarray, y: np.ndarray, x_new: float, below: float, above: float) -> float:
    """scipy.interpolate.interp1d(x, y, kind="linear", bounds_error=False, fill_value=(below, above)) at one point: x sorted first (stable), the bracket from
    searchsorted clipped to 1 .. len - 1, slope * (x_new - x_lo) + y_lo; the fill values strictly outside [x[0], x[-1]]."""
    if x.shape[0] < 2:
        raise ValueError("x and y arrays must have at least 2 entries")
    order = np.argsort(x, kind="mergesort")
    x, y = x[order], y[order]
    hi = int(np.clip(np.searchsorted(x, x_new), 1, len(x) - 1))
    lo = hi - 1
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
    v = slope * (x_new - x[lo]) + y[lo]
    if x_new < x[0]:
        v = below
    if x_new > x[-1]:
        v = above
    return v


def create_time_map_from_downbeats(downbeats, align_result: dict, feature_rate: int = 50) -> list:
    """etude/utils/preprocess.py:21-58: [origin downbeat time, cover time on the warping path] for every downbeat not past the path's end."""
    wp = align_result["wp"]
    t_origin = wp[1] / feature_rate
    t_cover = wp[0] / feature_rate
    if t_origin.shape[0] < 2:
        raise ValueError("x and y arrays must have at least 2 entries")      # (interp1d's own refusal, raised where the reference builds the interpolator)
    time_map = []
    for db_time in downbeats:
        if db_time <= t_origin[-1]:
            time_map.append([float(db_time), float(_interp_linear(t_origin, t_cover, db_time, t_cover[0], t_cover[-1]))])
    return time_map


def weakly_align(transcription_notes: list, time_map: list) -> list:
    """etude/utils/preprocess.py:60-114: every note's onset moves from the cover's timeline to the origin's, linearly inside its segment of the time map (sorted in
    place by cover time, as the reference does); the duration is kept.  A note before the first anchor, or in a segment shorter than 1e-6 s, is dropped; the last
    anchor opens a segment of 10 s."""
    if not time_map or not transcription_notes:
        return []
    out = []
    time_map.sort(key=lambda p: p[1])
    k = 0
    for note in sorted(transcription_notes, key=lambda n: n["onset"]):
        t_on = note["onset"]
        dur = note["offset"] - t_on
        while k + 1 < len(time_map) and t_on >= time_map[k + 1][1]:
            k += 1
        s1, p1 = time_map[k]
        if k + 1 < len(time_map):
            s2, p2 = time_map[k + 1]
        else:
            s2, p2 = s1 + 10, p1 + 10
        seg = p2 - p1
        if seg < 1e-6:
            continue
        if p1 <= t_on < p2:
            rel = (t_on - p1) / seg
            onset = s1 + rel * (s2 - s1)
            out.append({"pitch": note["pitch"], "onset": onset, "offset": onset + dur, "velocity": note["velocity"]})
    return out
