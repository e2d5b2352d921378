"""The audio front end restated in float64, stage by stage, and the shapes its tests share.  TEST INFRASTRUCTURE ONLY.

Written from the algorithm (channel mean; polyphase sinc resampling ``y[j*new + p] = sum_k kern[p][k] x[j*orig + k - width]``; centred framing, window,
DFT, ``|X|^2``; filterbank; log; centred RMS frames), not from csrc/frontend.hip: no LDS span, no bit reversal, no CSR.  The tables (resampling kernel,
window, dense filterbank) are arguments -- the fp32 ones the device was given, cast up -- so a figure measured against this file is the error of the
arithmetic alone.  ``stft_mel_f32_radix2`` is the one exception: an fp32 numpy run of a radix-2 decimation-in-time schedule, a second yardstick for the
STFT stage beside fp32 torch (whose FFT is another algorithm with another error constant).

tests/test_frontend_cpu.py holds this file to oracle/mel.py in float64 and to torch.stft(float64); tests/test_gpu_frontend_stages.py holds the device to it.
"""
from __future__ import annotations

import math

import numpy as np

RB = 8                      # input blocks per workgroup of the device's resampler: lengths are placed around nw * RB outputs
LOG_OFFSET = np.float32(1e-8)

# (sr_in, sr_out): orig 441 / nw 160 / K 475; orig 3 / nw 1; orig 1 / nw 2; nw 441 (second trip of a 256-wide phase loop); nw 640 (third trip);
# orig 2 / nw 1; equal rates (channel mean only)
RATE_PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (16000, 22050), (11025, 16000), (44100, 22050), (16000, 16000)]

# (n_fft, hop, n_mels, win_length)
SETTINGS = [(2048, 256, 256, 2048),
            (2048, 256, 256, 1024),
            (64, 16, 8, 64),
            (64, 16, 256, 64),          # 33 bins for 256 bands: empty and single-bin bands
            (256, 100, 40, 255),        # odd window, a hop that divides nothing
            (512, 512, 128, 512),       # no overlap
            (4096, 256, 1024, 4096)]    # the largest accepted
PAD_MODES = ["reflect", "constant"]
CHANNELS = [1, 2, 3, 6]

RMS_FRAMES = [2, 63, 64, 65, 2204]
RMS_HOPS = [1, 1102]
RMS_QUOTIENTS = [6, 7, 8]   # n // hop: 7, 8, 9 frames -- four frames share a workgroup


def pair_dims(sr_in: int, sr_out: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(orig, new, width, K) of a rate pair: orig / new = the rates over their gcd, width = the one-sided reach of the windowed sinc in input samples"""
    g = math.gcd(int(sr_in), int(sr_out))
    orig, new = int(sr_in) // g, int(sr_out) // g
    width = math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))
    return orig, new, width, 2 * width + orig


def resampled_len(L: int, sr_in: int, sr_out: int) -> int:
    orig, new, _, _ = pair_dims(sr_in, sr_out)
    return -((-new * int(L)) // orig)          # ceil(new * L / orig) in integers


def num_frames(n: int, hop: int) -> int:
    return 1 + int(n) // int(hop)


def lengths_around(sr_in: int, sr_out: int, target: int):
    """The three input lengths around an output count: the longest clip that resamples to fewer than `target` samples, the shortest that reaches `target`,
    the shortest that exceeds it.  When downsampling the output grows by at most one per input sample, so these give target - 1, target, target + 1 exactly."""
    orig, new, _, _ = pair_dims(sr_in, sr_out)
    at = (target * orig) // new
    while resampled_len(at, sr_in, sr_out) >= target:
        at -= 1
    while resampled_len(at, sr_in, sr_out) < target:
        at += 1
    above = at
    while resampled_len(above, sr_in, sr_out) <= target:
        above += 1
    return [L for L in (at - 1, at, above) if L >= 1]


def resample_lengths(sr_in: int, sr_out: int):
    """Input lengths at which the resampler can go wrong: one sample; around one input block and one filter span (zero fill on both sides of a clip shorter than
    the span); outputs one below, at and one above a whole workgroup (nw * RB) and, for the extractor's pair, a whole block (nw) that is no whole workgroup."""
    if sr_in == sr_out:
        return [1, 255, 256, 257]
    orig, new, width, K = pair_dims(sr_in, sr_out)
    out = [1] + lengths_around(sr_in, sr_out, new * RB)
    if (sr_in, sr_out) == (44100, 16000):
        out += [orig - 1, orig, orig + 1, K - 1, K, K + 1] + lengths_around(sr_in, sr_out, 2 * new * RB) + lengths_around(sr_in, sr_out, 11 * new)
    return sorted(set(out))


RESAMPLE_CASES = [(a, b, L) for a, b in RATE_PAIRS for L in resample_lengths(a, b)]


def clip_len(n_fft: int, hop: int) -> int:
    """A clip of a few frames for a transform setting: two windows and a bit, odd, no multiple of the hop"""
    n = 2 * n_fft + hop // 2 + 3
    return n + (n % hop == 0)


# ------------------------------------------------------------------------------------------------ inputs
def noisy_clip(seed: int, channels: int, L: int, sr: int) -> np.ndarray:
    """[channels, L] fp32: synth.clip_audio (decaying sinusoids) plus white noise 40 dB below its peak, so that no mel band sits at a level set by cancellation,
    where a log-domain figure would measure luck.  Every channel has its own content: pairs come from clips of different seeds, each scaled differently."""
    from etude_amd import synth
    out = np.zeros((channels, L), np.float32)
    seconds = (L + 1) / sr + 0.01
    for c0 in range(0, channels, 2):
        a = synth.clip_audio(seed=1000 * seed + c0, seconds=seconds, sr=sr)[:, :L]
        n = min(2, channels - c0)
        out[c0:c0 + n] = a[:n] * np.float32(1.0 - 0.11 * c0)
    rng = np.random.default_rng(77 + seed)
    out += (0.5 * 10 ** (-40 / 20) * rng.standard_normal(out.shape)).astype(np.float32)
    return np.ascontiguousarray(out)


def ramp(L: int) -> np.ndarray:
    """[L] fp32, deterministic, non-periodic, no two windows alike: a chirp under a slow ramp"""
    i = np.arange(L, dtype=np.float64)
    return ((0.25 + 0.5 * (i % 977) / 977.0) * np.sin(0.05 * i + 3e-5 * i * i) + 0.1 * np.cos(1.7 * i)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ tables
def window_table(n_fft: int, win_length: int) -> np.ndarray:
    """torch.stft's window: a periodic Hann of win_length samples centred in n_fft (fp32, as the device is given it)"""
    import torch
    win = np.zeros(n_fft, np.float32)
    lpad = (n_fft - win_length) // 2
    win[lpad:lpad + win_length] = torch.hann_window(win_length, periodic=True).numpy()
    return win


def csr_to_dense(start, length, w, n_freqs: int) -> np.ndarray:
    fb = np.zeros((n_freqs, len(start)), np.float32)
    o = 0
    for m, (s, n) in enumerate(zip(start, length)):
        fb[s:s + n, m] = w[o:o + n]
        o += n
    return fb


# ------------------------------------------------------------------------------------------------ stages, float64
def mono(wav) -> np.ndarray:
    return np.asarray(wav, np.float64).mean(axis=0)


def resample(x, kern, width: int, orig: int, new: int) -> np.ndarray:
    """kern [new][K] (K = 2 * width + orig): y[j * new + p] = sum_k kern[p][k] * x[j * orig + k - width], zeros outside the clip, cut to ceil(new * L / orig)"""
    x = np.asarray(x, np.float64)
    kern = np.asarray(kern, np.float64)
    L, K = x.shape[0], kern.shape[1]
    target = -((-new * L) // orig)
    J = -(-target // new)
    xp = np.zeros(width + (J - 1) * orig + K + L, np.float64)
    xp[width:width + L] = x
    blocks = np.lib.stride_tricks.sliding_window_view(xp, K)[::orig][:J]       # [J, K]: block j starts at x[j * orig - width]
    return (blocks @ kern.T).reshape(-1)[:target]


def frames_of(x, n_fft: int, hop: int, pad_mode: str) -> np.ndarray:
    x = np.asarray(x, np.float64)
    half = n_fft // 2
    xp = np.pad(x, (half, half), mode="reflect") if pad_mode == "reflect" else np.pad(x, (half, half + n_fft))
    T = num_frames(x.shape[0], hop)
    return np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::hop][:T]      # [T, n_fft]: frame t starts at x[t * hop - n_fft / 2]


def power_frames(x, n_fft: int, hop: int, window, pad_mode: str) -> np.ndarray:
    """[T, n_fft / 2 + 1]: |rfft(window * frame)|^2, frame t centred on sample t * hop, the clip reflected (without repeating its end samples) or zero-padded"""
    f = frames_of(x, n_fft, hop, pad_mode) * np.asarray(window, np.float64)[None]
    X = np.fft.rfft(f, axis=1)
    return X.real ** 2 + X.imag ** 2


def log_mel(power, fb, log_offset=LOG_OFFSET) -> np.ndarray:
    """fb dense [n_freqs, n_mels] -> [T, n_mels]"""
    return np.log(np.asarray(power, np.float64) @ np.asarray(fb, np.float64) + np.float64(log_offset))


def rms_frames(x, frame: int, hop: int) -> np.ndarray:
    """frame t covers samples [t * hop - frame // 2, + frame), zeros outside the clip; 1 + n // hop frames"""
    x = np.asarray(x, np.float64)
    xp = np.pad(x, (frame // 2, frame + hop))
    f = np.lib.stride_tricks.sliding_window_view(xp, frame)[::hop][:num_frames(x.shape[0], hop)]
    return np.sqrt((f * f).sum(axis=1) / frame)


# ------------------------------------------------------------------------------------------------ fp32 yardstick of the radix-2 schedule
def stft_mel_f32_radix2(x32, n_fft: int, hop: int, window32, pad_mode: str, fb32, log_offset=LOG_OFFSET) -> np.ndarray:
    """The STFT / mel / log stage in fp32 numpy with a radix-2 decimation-in-time FFT (bit-reversed input, lg(n_fft) butterfly passes, twiddles rounded once from
    float64): what fp32 loses on this stage when the transform is the plain radix-2 one."""
    x32 = np.asarray(x32, np.float32)
    half = n_fft // 2
    xp = np.pad(x32, (half, half), mode="reflect") if pad_mode == "reflect" else np.pad(x32, (half, half + n_fft))
    T = num_frames(x32.shape[0], hop)
    f = np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::hop][:T] * np.asarray(window32, np.float32)[None]
    lg = n_fft.bit_length() - 1
    i = np.arange(n_fft)
    rev = np.zeros(n_fft, np.int64)
    for b in range(lg):
        rev |= ((i >> b) & 1) << (lg - 1 - b)
    re = np.ascontiguousarray(f[:, rev]).astype(np.float32)
    im = np.zeros_like(re)
    ang = -2.0 * np.pi * np.arange(half) / n_fft
    twr, twi = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    for s in range(lg):
        hl = 1 << s
        re = re.reshape(T, -1, 2, hl)
        im = im.reshape(T, -1, 2, hl)
        wr, wi = twr[:: half // hl][None, None], twi[:: half // hl][None, None]
        xr, xi = re[:, :, 1], im[:, :, 1]
        tr, ti = wr * xr - wi * xi, wr * xi + wi * xr
        ur, ui = re[:, :, 0], im[:, :, 0]
        re = np.stack([ur + tr, ur - tr], axis=2).reshape(T, n_fft)
        im = np.stack([ui + ti, ui - ti], axis=2).reshape(T, n_fft)
    pw = re[:, :half + 1] ** 2 + im[:, :half + 1] ** 2
    acc = np.zeros((T, fb32.shape[1]), np.float32)
    for k in range(half + 1):                                  # bins in ascending order, one fp32 addition per bin
        acc += pw[:, k:k + 1] * np.asarray(fb32[k], np.float32)[None]
    return np.log(acc + np.float32(log_offset))
