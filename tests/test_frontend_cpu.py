"""Keeps tests/frontend_np.py (the float64 restatement the device is held to) and the host tables of etude_amd/frontend.py honest.  No GPU.

The restatement is compared with oracle/mel.py run in float64 on the same fp32 tables cast up (so the difference is float64 rounding, nothing else), with
torch.stft(float64) directly, and with signals whose answer is known in closed form.  The two tables the host layer builds for the device are bit-identical to
the oracle's.  etd_frontend_resampled_len / etd_frontend_num_frames need a handle, which needs a device: they are checked in test_gpu_frontend_stages.py.
"""
import math

import numpy as np
import pytest
import torch

import frontend_np as fnp
from etude_amd.frontend import _dense_to_csr, _mel_csr, _resample_table
from oracle import mel

RESAMPLING_PAIRS = [p for p in fnp.RATE_PAIRS if p[0] != p[1]]
F64 = 1e-12          # relative to the largest value: float64 sums of a few thousand fp32-sized terms in two orders lose 1e-14 .. 1e-13


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    s = float(np.abs(ref).max())
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / (s if s > 0 else 1.0)


def mono64(seed, L, sr, channels=2):
    return fnp.mono(fnp.noisy_clip(seed, channels, L, sr))


# ---------------------------------------------------------------------------------------------------- shape lists
def test_shape_lists_sit_on_the_edges():
    orig, new, width, K = fnp.pair_dims(44100, 16000)
    assert (orig, new, width, K) == (441, 160, 17, 475)
    assert [fnp.pair_dims(a, b)[:2] for a, b in fnp.RATE_PAIRS] == [(441, 160), (3, 1), (1, 2), (320, 441), (441, 640), (2, 1), (1, 1)]
    Ls = fnp.resample_lengths(44100, 16000)
    assert {1, 440, 441, 442, 474, 475, 476} <= set(Ls)
    n_out = {fnp.resampled_len(L, 44100, 16000) for L in Ls}
    for target in (new * fnp.RB, 2 * new * fnp.RB, 11 * new):
        assert {target - 1, target, target + 1} <= n_out
    for a, b in RESAMPLING_PAIRS:                                  # every pair: a last workgroup that is short by one, full, and one output into the next
        new = fnp.pair_dims(a, b)[1]
        lo, at, hi = [fnp.resampled_len(L, a, b) for L in fnp.lengths_around(a, b, new * fnp.RB)]
        assert lo < new * fnp.RB <= at < hi and (a < b or (lo, at, hi) == (new * fnp.RB - 1, new * fnp.RB, new * fnp.RB + 1))
    assert len(fnp.RESAMPLE_CASES) == len(set(fnp.RESAMPLE_CASES))
    for n_fft, hop, n_mels, win in fnp.SETTINGS:
        assert fnp.clip_len(n_fft, hop) % hop and fnp.clip_len(n_fft, hop) > n_fft // 2


@pytest.mark.parametrize("sr_in,sr_out", RESAMPLING_PAIRS)
def test_length_formulas_match_the_oracle(sr_in, sr_out):
    orig, new, _, _ = fnp.pair_dims(sr_in, sr_out)
    for L in list(range(1, 40)) + fnp.resample_lengths(sr_in, sr_out) + [orig * 7 + 3]:
        n = fnp.resampled_len(L, sr_in, sr_out)
        assert n == int(math.ceil(new * L / orig)) == mel.resample(torch.zeros(L), sr_in, sr_out).numel()
        assert fnp.num_frames(n, 256) == mel.feature_frames(L, sr_in, sr_out, 256)


# ---------------------------------------------------------------------------------------------------- host tables
@pytest.mark.parametrize("sr_in,sr_out", RESAMPLING_PAIRS)
def test_resample_table_is_the_oracles(sr_in, sr_out):
    kt, width, orig, new = _resample_table(sr_in, sr_out)
    k, w2, o2, n2 = mel.sinc_resample_kernel(sr_in, sr_out)
    assert (width, orig, new) == (w2, o2, n2) == fnp.pair_dims(sr_in, sr_out)[2:3] + fnp.pair_dims(sr_in, sr_out)[:2]
    assert kt.dtype == np.float32 and kt.shape == (2 * width + orig, new) and kt.flags.c_contiguous
    assert kt.tobytes() == np.ascontiguousarray(k.numpy().T).tobytes()


MEL_CONFIGS = sorted({(n_fft, n_mels, sr) for n_fft, _, n_mels, _ in fnp.SETTINGS for sr in (16000, 22050)} | {(64, 1024, 16000), (4096, 8, 22050)})


@pytest.mark.parametrize("n_fft,n_mels,sr", MEL_CONFIGS)
def test_mel_csr_scatters_back_to_the_oracles_filterbank(n_fft, n_mels, sr):
    n_freqs = n_fft // 2 + 1
    start, length, w = _mel_csr(n_freqs, float(sr // 2), n_mels, sr)
    want = mel.melscale_fbanks(n_freqs, 0.0, float(sr // 2), n_mels, sr).numpy()
    assert start.dtype == length.dtype == np.int32 and w.dtype == np.float32
    assert (length >= 0).all() and (start >= 0).all() and (start + length <= n_freqs).all()
    assert w.size == max(1, int(length.sum()))
    # the same value in every cell, hence the same bits in every non-zero cell; the oracle's max(0, min(down, up)) leaves some zeros signed (-0.0), which
    # carry no weight and which the CSR form does not store
    assert np.array_equal(fnp.csr_to_dense(start, length, w, n_freqs), want)
    assert fnp.csr_to_dense(start, length, w, n_freqs).tobytes() == (want + np.float32(0.0)).tobytes()
    for m in range(n_mels):                                        # a span is tight: it starts and ends on a non-zero weight, an empty band has length 0
        nz = np.flatnonzero(want[:, m])
        assert length[m] == (nz[-1] - nz[0] + 1 if nz.size else 0)


def _interior_zero_fb():
    """A filterbank whose band 1 has a zero inside its span and whose band 2 is empty, as fp32 rounding can make them"""
    fb = np.zeros((9, 4), np.float32)
    fb[1:3, 0] = (0.5, 0.25)
    fb[2:7, 1] = (0.1, 0.0, 0.3, 0.0, 0.2)
    fb[8, 3] = 1.0
    return fb


def test_mel_csr_keeps_interior_zeros_and_empty_bands():
    """No triangular filter of the configurations above has a zero strictly inside its span, so that case is planted: the CSR step must store the span from
    the first to the last non-zero weight, zeros included, and give an empty band length 0."""
    assert (_mel_csr(33, 8000.0, 256, 16000)[1] == 0).any()                  # the (64, 16, 256, 64) setting really has empty bands
    fb = _interior_zero_fb()
    start, length, w = _dense_to_csr(fb)
    assert start.tolist() == [1, 2, 0, 8] and length.tolist() == [2, 5, 0, 1]
    assert w.dtype == np.float32 and w.tobytes() == np.array([0.5, 0.25, 0.1, 0.0, 0.3, 0.0, 0.2, 1.0], np.float32).tobytes()
    assert fnp.csr_to_dense(start, length, w, 9).tobytes() == fb.tobytes()
    s0, l0, w0 = _dense_to_csr(np.zeros((9, 3), np.float32))                 # nothing but empty bands: one placeholder weight, never read
    assert not l0.any() and w0.size == 1


# ---------------------------------------------------------------------------------------------------- the restatement against the oracle in float64
@pytest.mark.parametrize("sr_in,sr_out,L", [c for c in fnp.RESAMPLE_CASES if c[0] != c[1]])
def test_resample_restatement_matches_oracle_f64(monkeypatch, sr_in, sr_out, L):
    k32, width, orig, new = mel.sinc_resample_kernel(sr_in, sr_out)
    monkeypatch.setattr(mel, "sinc_resample_kernel", lambda *a, **kw: (k32.double(), width, orig, new))     # the oracle's own path on the fp32 table cast up
    x = mono64(L % 13, L, sr_in)
    want = mel.resample(torch.from_numpy(x), sr_in, sr_out).numpy()
    got = fnp.resample(x, k32.numpy(), width, orig, new)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (fnp.resampled_len(L, sr_in, sr_out),)
    assert rel(got, want) <= F64


def _clip_for(setting, pad_mode, seed=3):
    n_fft, hop, n_mels, win = setting
    return mono64(seed, fnp.clip_len(n_fft, hop), 16000)


@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_power_frames_match_torch_stft_f64(setting, pad_mode):
    n_fft, hop, n_mels, win = setting
    x = _clip_for(setting, pad_mode)
    window = fnp.window_table(n_fft, win)
    want = torch.stft(torch.from_numpy(x), n_fft=n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True).double(), center=True,
                      pad_mode=pad_mode, normalized=False, onesided=True, return_complex=True).abs().pow(2.0).numpy().T
    got = fnp.power_frames(x, n_fft, hop, window, pad_mode)
    assert got.shape == want.shape == (fnp.num_frames(x.size, hop), n_fft // 2 + 1)
    assert rel(got, want) <= F64


@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_log_mel_restatement_matches_oracle_f64(monkeypatch, setting, pad_mode):
    n_fft, hop, n_mels, win = setting
    x = _clip_for(setting, pad_mode, seed=4)
    fb = mel.melscale_fbanks(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000)
    hann = torch.hann_window
    monkeypatch.setattr(torch, "hann_window", lambda n, periodic=True: hann(n, periodic=periodic).double())   # the oracle in float64 on its fp32 tables cast up
    monkeypatch.setattr(mel, "melscale_fbanks", lambda *a, **k: fb.double())
    want = mel.log_mel(torch.from_numpy(x), 16000, n_fft, win, hop, n_mels, float(fnp.LOG_OFFSET), pad_mode).numpy()
    monkeypatch.undo()
    got = fnp.log_mel(fnp.power_frames(x, n_fft, hop, fnp.window_table(n_fft, win), pad_mode), fb.numpy())
    assert want.dtype == np.float64 and got.shape == want.shape
    # in the log domain: an absolute 1e-12 is a relative 1e-12 of the band's power (offset included)
    assert float(np.abs(got - want).max()) <= 1e-11


@pytest.mark.parametrize("n,N", [(2048, 1025), (64, 33), (256, 129)])
def test_smallest_reflect_clip_matches_torch(n, N):
    """N = n_fft / 2 + 1, the shortest clip reflect padding is defined for: the last frame reflects about sample N - 1 all the way back to sample 1"""
    x = fnp.ramp(N).astype(np.float64)
    hop = n // 8
    want = torch.stft(torch.from_numpy(x), n_fft=n, hop_length=hop, window=torch.hann_window(n).double(), center=True, pad_mode="reflect",
                      return_complex=True).abs().pow(2.0).numpy().T
    assert rel(fnp.power_frames(x, n, hop, fnp.window_table(n, n), "reflect"), want) <= F64
    f = fnp.frames_of(x, n, hop, "reflect")
    assert f[0, 0] == x[n // 2] and f[0, n // 2] == x[0] and f[-1, -1] == x[2 * (N - 1) - ((f.shape[0] - 1) * hop + n - 1 - n // 2)]


def test_rms_restatement_matches_oracle_f64():
    for frame, hop, n in [(2204, 1102, 7000), (2, 1, 9), (65, 7, 300), (63, 1102, 2 * 1102)]:
        x = torch.from_numpy(fnp.ramp(n).astype(np.float64))
        yp = torch.nn.functional.pad(x, (frame // 2, frame))
        want = torch.sqrt(torch.mean(yp.unfold(0, frame, hop)[:1 + n // hop] ** 2, dim=1)).numpy()
        got = fnp.rms_frames(x.numpy(), frame, hop)
        assert got.shape == want.shape == (1 + n // hop,) and rel(got, want) <= F64


# ---------------------------------------------------------------------------------------------------- analytic
def test_sinusoid_at_a_bin_centre():
    n_fft, hop, b = 256, 64, 37
    x = np.cos(2 * np.pi * b * np.arange(4 * n_fft) / n_fft)
    p = fnp.power_frames(x, n_fft, hop, np.ones(n_fft), "reflect")
    t = p.shape[0] // 2                                        # an interior frame holds whole periods: all power in bin b, (n/2)^2 of it
    assert abs(p[t, b] - (n_fft / 2) ** 2) <= 1e-9 * (n_fft / 2) ** 2 and np.delete(p[t], b).max() <= 1e-18 * (n_fft / 2) ** 2
    ph = fnp.power_frames(x, n_fft, hop, fnp.window_table(n_fft, n_fft), "reflect")       # Hann: (n/4)^2 at b, a quarter of that at b +- 1, nothing else
    assert abs(ph[t, b] - (n_fft / 4) ** 2) <= 1e-6 * (n_fft / 4) ** 2
    assert abs(ph[t, b - 1] - (n_fft / 8) ** 2) <= 1e-6 * (n_fft / 8) ** 2 and abs(ph[t, b + 1] - (n_fft / 8) ** 2) <= 1e-6 * (n_fft / 8) ** 2
    assert np.delete(ph[t], [b - 1, b, b + 1]).max() <= 1e-10 * (n_fft / 4) ** 2
    fb = np.zeros((n_fft // 2 + 1, 2))
    fb[b, 0] = 0.5
    assert np.allclose(fnp.log_mel(p[t:t + 1], fb)[0], [np.log(0.5 * (n_fft / 2) ** 2 + 1e-8), np.log(np.float64(fnp.LOG_OFFSET))], rtol=1e-12, atol=0)


@pytest.mark.parametrize("sr_in,sr_out", RESAMPLING_PAIRS)
def test_constant_resamples_to_the_constant(sr_in, sr_out):
    """Away from the ends every phase of the windowed sinc sums to 1 up to its stop-band ripple (a few 1e-4 at width 6) -- a dropped tap or a phase read from the
    wrong row is 1e-2 or more"""
    kt, width, orig, new = _resample_table(sr_in, sr_out)
    L = 6 * (orig + 2 * width)
    y = fnp.resample(np.full(L, 0.75), kt.T, width, orig, new)
    lo = -(-width * new // orig) + new
    inner = y[lo:y.size - lo - new]
    assert inner.size >= new and np.abs(inner - 0.75).max() < 2e-3 * 0.75
    if orig >= 2 * new:                                             # a low-pass below the input's Nyquist: the first output sees half the filter, about half the step
        assert abs(y[0] - 0.75) > 0.1


def test_rms_of_a_constant():
    for frame, hop in [(2204, 1102), (64, 1), (63, 5)]:
        r = fnp.rms_frames(np.full(20 * frame, -0.3), frame, hop)
        inner = r[frame // hop + 1: r.size - frame // hop - 1]
        assert inner.size and np.abs(inner - 0.3).max() <= 1e-15
        assert r[0] < 0.3 * 0.8                                    # the first frame is half padding


@pytest.mark.parametrize("setting", [fnp.SETTINGS[1], fnp.SETTINGS[3], fnp.SETTINGS[4]], ids=lambda s: "-".join(map(str, s)))
def test_radix2_yardstick_is_the_same_transform(setting):
    """frontend_np.stft_mel_f32_radix2 (the fp32 radix-2 yardstick of the STFT stage) computes what the float64 restatement computes, to fp32 accuracy"""
    n_fft, hop, n_mels, win = setting
    x = mono64(6, fnp.clip_len(n_fft, hop), 16000).astype(np.float32)
    fb = mel.melscale_fbanks(n_fft // 2 + 1, 0.0, 8000.0, n_mels, 16000).numpy()
    window = fnp.window_table(n_fft, win)
    for pad_mode in fnp.PAD_MODES:
        want = fnp.log_mel(fnp.power_frames(x, n_fft, hop, window, pad_mode), fb)
        got = fnp.stft_mel_f32_radix2(x, n_fft, hop, window, pad_mode, fb)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.abs(got - want).max() < 1e-3 and np.abs(got - want).mean() < 1e-5
