"""The stem mel-dB feature contract of DESIGN.md 4d, restated in numpy: the oracle of tests/test_stemfeat_cpu.py and tests/test_gpu_stemfeat.py.

``features(stems, ...)`` is the fp64 restatement ([instr][channels][N] float32 -> [instr][T][n_mels] float64); ``features(..., dtype=np.float32)`` runs the same
steps in float32 (scipy.fft.rfft on float32 frames, a float32 filterbank product): the arithmetic librosa itself uses, which the GPU test takes as the yardstick of
what float32 costs.  librosa is not a dependency: parity with it is unpinned.
"""
from __future__ import annotations

import numpy as np

FRAMINGS = ("librosa", "librosa_reflect", "spleeter")


def lead_of(framing: str, n_fft: int) -> int:
    if framing not in FRAMINGS:
        raise ValueError(f"framing must be one of {FRAMINGS}, got {framing!r}")
    return n_fft if framing == "spleeter" else n_fft // 2


def num_frames(N: int, n_fft: int = 4096, hop: int = 1024, framing: str = "librosa") -> int:
    return 1 + (N + 2 * lead_of(framing, n_fft) - n_fft) // hop


def hz_to_mel(f):
    """Slaney scale: linear below 1 kHz, logarithmic above"""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sr: int = 44100, n_fft: int = 4096, n_mels: int = 128, fmin: float = 30.0, fmax: float = 11000.0) -> np.ndarray:
    """librosa.filters.mel(htk=False, norm="slaney") -> [n_mels][n_fft/2 + 1] float32, formed in fp64"""
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)          # rfftfreq
    pts = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    fdiff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    fb = np.zeros((n_mels, freqs.size), np.float64)
    for m in range(n_mels):
        lower = -ramps[m] / fdiff[m]
        upper = ramps[m + 2] / fdiff[m + 1]
        fb[m] = np.maximum(0.0, np.minimum(lower, upper))
    fb *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb.astype(np.float32)


def hann(n_fft: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


def mono_of(stems: np.ndarray) -> np.ndarray:
    """[instr][channels][N] float32 -> [instr][N] float32: the channel mean in fp32 (channels summed in order, then divided)"""
    x = np.asarray(stems, np.float32)
    acc = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        acc = acc + x[:, c]
    return acc / np.float32(x.shape[1])


def frames_of(mono: np.ndarray, n_fft: int, hop: int, framing: str) -> np.ndarray:
    """[N] -> [T][n_fft]: frame t covers samples [t * hop - lead, + n_fft), zeros or reflection outside [0, N)"""
    N = mono.shape[0]
    lead = lead_of(framing, n_fft)
    if framing == "librosa_reflect":
        if N <= n_fft // 2:
            raise ValueError(f"librosa_reflect needs N > n_fft / 2 = {n_fft // 2}, got {N}")
        padded = np.pad(mono, (lead, lead), mode="reflect")
    else:
        padded = np.pad(mono, (lead, lead))
    T = num_frames(N, n_fft, hop, framing)
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return padded[idx]


def features(stems, sr: int = 44100, n_fft: int = 4096, hop: int = 1024, n_mels: int = 128, fmin: float = 30.0, fmax: float = 11000.0,
             top_db: float = 80.0, amin: float = 1e-10, framing: str = "librosa", dtype=np.float64) -> np.ndarray:
    stems = np.asarray(stems)
    if stems.ndim != 3 or stems.shape[1] < 1 or stems.shape[2] < 1:
        raise ValueError(f"stems must be [instr][channels >= 1][N >= 1], got {stems.shape}")
    dtype = np.dtype(dtype)
    mono = mono_of(stems)
    fb = mel_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(dtype)
    win = hann(n_fft).astype(dtype)
    out = []
    for i in range(mono.shape[0]):
        fr = frames_of(mono[i].astype(dtype), n_fft, hop, framing) * win
        if dtype == np.float32:
            import scipy.fft
            spec = scipy.fft.rfft(fr, axis=1)
            assert spec.dtype == np.complex64
        else:
            spec = np.fft.rfft(fr, axis=1)
        power = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
        S = power @ fb.T
        ref = S.max()
        ten, a = dtype.type(10.0), dtype.type(amin)
        y = ten * np.log10(np.maximum(a, S)) - ten * np.log10(np.maximum(a, ref))
        y = np.maximum(y, y.max() - dtype.type(top_db))
        out.append(y)
    return np.stack(out)


def synthetic_stems(seed: int, instr: int = 5, channels: int = 2, N: int = 1024 * 40 + 517, sr: int = 44100, silent_stem: int = 3,
                    zero_frames=(1, 12, 20), hop: int = 1024) -> np.ndarray:
    """The seeded test input: six Gaussian-enveloped sinusoids (40 .. 9 000 Hz, amplitudes 1e-3 .. 0.3) and white noise (1e-5 .. 1e-3) per stem; stem `silent_stem`
    all zeros; samples of frames zero_frames[1] .. zero_frames[2] (with a frame's whole support) of stem zero_frames[0] zeroed."""
    rng = np.random.default_rng(seed)
    t = np.arange(N, dtype=np.float64) / sr
    x = np.zeros((instr, channels, N), np.float64)
    for i in range(instr):
        for c in range(channels):
            for _ in range(6):
                f = np.exp(rng.uniform(np.log(40.0), np.log(9000.0)))
                a = np.exp(rng.uniform(np.log(1e-3), np.log(0.3)))
                mid, wid = rng.uniform(0, N / sr), rng.uniform(0.05, 0.5) * max(N / sr, 1e-3)
                x[i, c] += a * np.exp(-0.5 * ((t - mid) / wid) ** 2) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
            x[i, c] += np.exp(rng.uniform(np.log(1e-5), np.log(1e-3))) * rng.standard_normal(N)
    if 0 <= silent_stem < instr:
        x[silent_stem] = 0.0
    if zero_frames is not None and zero_frames[0] < instr:
        s, a, b = zero_frames
        lo, hi = max(0, a * hop - 4096), min(N, (b - 1) * hop + 4096)          # every sample a zero frame can see, for every framing at n_fft <= 4096
        if lo < hi:
            x[s, :, lo:hi] = 0.0
    return x.astype(np.float32)
