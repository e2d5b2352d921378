"""The audio front end on the device (csrc/frontend.hip: k_resample, k_mono, k_stft_mel, k_rms_frames), stage by stage, against the float64 restatement
tests/frontend_np.py at every length, rate and frame edge.

etd_frontend_run and etd_rms_frames are driven through ctypes so that the test owns the output buffers: each has 64 guard floats on either side holding a NaN
bit pattern, and is pre-filled with it.  After every call the guards must be untouched and no float inside may still hold the pattern.

Each stage is fed its own tapped input: the resampler (or channel mean) gets the clip; the STFT / mel / log stage and the RMS stage are compared with the
restatement applied to the device's own resampled buffer.  The yardstick is not a constant.  A figure is ``err = max|dev - f64| / max|f64|`` (resampler, channel
mean, RMS) or the largest and the mean absolute difference in the log domain (log-mel), and is held to 4 x the same figure of fp32 torch on the CPU for the same
stage on the same input (oracle.mel.resample, torch.mean, oracle.mel.log_mel, an fp32 unfold), with a floor of 4 * 2^-24 (relative to max|f64|) where fp32 torch
happens to be exact: two fp32 chains over the same terms in different orders.  A dropped tap, a shifted band or a wrong reflection shows at 1e-3 or more.  The
log-mel rows also carry the figures of an fp32 numpy radix-2 FFT (frontend_np.stft_mel_f32_radix2), the device's own kind of transform, for comparison.

The exact tests (run to run, shifts, zero-pad linearity, silence) carry no tolerance.  Every figure is printed; with ETD_FRONTEND_REPORT=dir they are also kept as
dir/frontend_device.json (how profiles/frontend_device.json is made).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import frontend_np as fnp
from etude_amd import _lib
from oracle import mel

pytestmark = pytest.mark.gpu

FLOOR = 4.0 * 2.0 ** -24
GUARD = 64
NAN_BITS = 0x7FC5A5A5                      # a quiet NaN no kernel produces
DEFAULT = fnp.SETTINGS[0]
ROWS = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield torch.device("cuda:0")
    for f in _FE.values():
        f.close()
    _FE.clear()
    out = os.environ.get("ETD_FRONTEND_REPORT")
    if out and ROWS:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "frontend_device.json"), "w") as f:
            json.dump(ROWS, f, indent=1)


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    s = float(np.abs(ref).max())
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / (s if s > 0 else 1.0)


def held(err_dev, err32, floor=FLOOR):
    return err_dev <= max(4.0 * err32, floor)


def record(**row):
    print(row)
    ROWS.append(row)
    return row


class Guarded:
    """n floats on the device between two guards, all holding NAN_BITS until a kernel writes them"""

    def __init__(self, n, dev):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == NAN_BITS).all(), "written below the buffer"
        assert (b[GUARD + self.n:] == NAN_BITS).all(), "written beyond the buffer"
        inner = b[GUARD:GUARD + self.n]
        assert not (inner == NAN_BITS).any(), f"{int((inner == NAN_BITS).sum())} of {self.n} floats never written"
        return inner.view(np.float32).copy()


_FE = {}


def front_end(sr_in, sr_out, setting=DEFAULT, pad_mode="reflect"):
    from etude_amd.frontend import FrontEnd
    key = (sr_in, sr_out, setting, pad_mode)
    if key not in _FE:
        n_fft, hop, n_mels, win = setting
        _FE[key] = FrontEnd(sr_in, sr_out, n_fft=n_fft, hop=hop, n_mels=n_mels, log_offset=float(fnp.LOG_OFFSET), pad_mode=pad_mode, win_length=win)
    return _FE[key]


def run(fe, wav, dev, features=True):
    """etd_frontend_run on guarded buffers -> (resampled [n], features [T, n_mels] or None)"""
    lib = _lib.lib()
    wav = np.ascontiguousarray(wav, np.float32)
    c, L = wav.shape
    w = torch.from_numpy(wav).to(dev)
    n = int(lib.etd_frontend_resampled_len(fe.h, L))
    T = int(lib.etd_frontend_num_frames(fe.h, L))
    assert n == fnp.resampled_len(L, fe.sr_in, fe.sr_out) and T == fnp.num_frames(n, fe.hop)
    res = Guarded(n, dev)
    feat = Guarded(T * fe.n_mels, dev) if features else None
    out_t = C.c_longlong(-1)
    _lib.check(lib.etd_frontend_run(fe.h, w.data_ptr(), c, L, res.ptr, feat.ptr if features else None, T if features else 0, C.byref(out_t), None), "etd_frontend_run")
    r = res.read()
    assert out_t.value == (T if features else 0)
    return r, (feat.read().reshape(T, fe.n_mels) if features else None)


def rms(x, frame, hop, dev, x_dev=None):
    lib = _lib.lib()
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev) if x_dev is None else x_dev
    n = xd.numel()
    T = fnp.num_frames(n, hop)
    out = Guarded(T, dev)
    _lib.check(lib.etd_rms_frames(xd.data_ptr(), n, frame, hop, out.ptr, T, None), "etd_rms_frames")
    return out.read()


def filterbank(fe, n_fft):
    return mel.melscale_fbanks(n_fft // 2 + 1, 0.0, float(fe.sr_out // 2), fe.n_mels, fe.sr_out).numpy()


# ---------------------------------------------------------------------------------------------------- stage checks
def check_first_stage(wav, sr_in, sr_out, res, tag):
    """channel mean (+ resampler) against float64 and fp32 torch"""
    from etude_amd.frontend import _resample_table
    x64 = fnp.mono(wav)
    m32 = torch.mean(torch.from_numpy(wav), dim=0)
    if sr_in == sr_out:
        want, y32, stage = x64, m32.numpy(), "mono"
    else:
        kt, width, orig, new = _resample_table(sr_in, sr_out)
        want, y32, stage = fnp.resample(x64, kt.T, width, orig, new), mel.resample(m32, sr_in, sr_out).numpy(), "resample"
    assert res.shape == want.shape == y32.shape
    row = record(stage=stage, case=tag, sr_in=sr_in, sr_out=sr_out, channels=int(wav.shape[0]), L=int(wav.shape[1]), n=int(res.size), err_dev=rel(res, want), err_f32=rel(y32, want))
    assert held(row["err_dev"], row["err_f32"]), row


def check_logmel(fe, setting, pad_mode, res, feat, tag):
    """the STFT / mel / log stage on the device's own resampled buffer"""
    n_fft, hop, n_mels, win = setting
    window, fb = fnp.window_table(n_fft, win), filterbank(fe, n_fft)
    want = fnp.log_mel(fnp.power_frames(res, n_fft, hop, window, pad_mode), fb)
    y32 = mel.log_mel(torch.from_numpy(res), fe.sr_out, n_fft, win, hop, n_mels, float(fnp.LOG_OFFSET), pad_mode).numpy()
    r2 = fnp.stft_mel_f32_radix2(res, n_fft, hop, window, pad_mode, fb)
    assert feat.shape == want.shape == y32.shape == r2.shape == (fnp.num_frames(res.size, hop), n_mels)
    assert np.isfinite(feat).all()
    d, d32, dr2 = np.abs(feat - want), np.abs(y32 - want), np.abs(r2 - want)
    row = record(stage="logmel", case=tag, setting=list(setting), pad_mode=pad_mode, n=int(res.size), frames=int(feat.shape[0]), max_dev=float(d.max()), max_f32=float(d32.max()),
                 max_radix2=float(dr2.max()), mean_dev=float(d.mean()), mean_f32=float(d32.mean()), mean_radix2=float(dr2.mean()), scale=float(np.abs(want).max()))
    floor = FLOOR * row["scale"]
    assert held(row["max_dev"], row["max_f32"], floor) and held(row["mean_dev"], row["mean_f32"], floor), row
    return want


def check_rms(x, frame, hop, got, tag):
    want = fnp.rms_frames(x, frame, hop)
    xp = torch.nn.functional.pad(torch.from_numpy(np.asarray(x, np.float32)), (frame // 2, frame + hop))
    f = xp.unfold(0, frame, hop)[:want.size]
    y32 = torch.sqrt(torch.mean(f * f, dim=1)).numpy()
    assert got.shape == want.shape == y32.shape
    row = record(stage="rms", case=tag, frame=frame, hop=hop, n=int(len(x)), frames=int(want.size), err_dev=rel(got, want), err_f32=rel(y32, want))
    assert held(row["err_dev"], row["err_f32"]), row
    return want


# ---------------------------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("sr_in,sr_out", fnp.RATE_PAIRS)
def test_length_formulas(dev, sr_in, sr_out):
    lib, fe = _lib.lib(), front_end(sr_in, sr_out)
    orig, new, _, _ = fnp.pair_dims(sr_in, sr_out)
    for L in list(range(0, 50)) + fnp.resample_lengths(sr_in, sr_out) + [orig * 1000 + 1, 2 ** 33 + 7]:
        n = -((-new * L) // orig)
        assert lib.etd_frontend_resampled_len(fe.h, L) == n and lib.etd_frontend_num_frames(fe.h, L) == 1 + n // 256 == fe.num_frames(L)


# ---------------------------------------------------------------------------------------------------- resampler and channel mean
@pytest.mark.parametrize("sr_in,sr_out,L", fnp.RESAMPLE_CASES)
def test_resample_stage(dev, sr_in, sr_out, L):
    """every rate pair at one sample, around its block, its filter span and its workgroup (frontend_np.resample_lengths); stereo"""
    wav = fnp.noisy_clip(L % 11, 2, L, sr_in)
    res, _ = run(front_end(sr_in, sr_out), wav, dev, features=False)
    check_first_stage(wav, sr_in, sr_out, res, "lengths")


@pytest.mark.parametrize("channels", fnp.CHANNELS)
@pytest.mark.parametrize("sr_in,sr_out,L", [(44100, 16000, 3529), (16000, 22050, 700), (16000, 16000, 1031)])
def test_channel_mean(dev, sr_in, sr_out, L, channels):
    """every channel has its own content: one read twice, or left out, is an error of the size of the signal"""
    wav = fnp.noisy_clip(5, channels, L, sr_in)
    assert all(np.abs(wav[a] - wav[b]).max() > 0.05 for a in range(channels) for b in range(a))
    res, _ = run(front_end(sr_in, sr_out), wav, dev, features=False)
    check_first_stage(wav, sr_in, sr_out, res, "channels")


# ---------------------------------------------------------------------------------------------------- STFT / mel / log
@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_logmel_stage_every_setting(dev, setting, pad_mode):
    """equal rates (k_mono in front): lg 6 .. 12, fewer butterflies than threads, one to four trips of the band loop, a window shorter than the frame"""
    n_fft, hop, n_mels, win = setting
    fe = front_end(16000, 16000, setting, pad_mode)
    wav = fnp.noisy_clip(2, 2, fnp.clip_len(n_fft, hop), 16000)
    res, feat = run(fe, wav, dev)
    check_first_stage(wav, 16000, 16000, res, "settings")
    check_logmel(fe, setting, pad_mode, res, feat, "settings")


@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("sr_in,sr_out,L", [(a, b, L) for a, b in [(44100, 16000), (16000, 16000), (16000, 22050)] for L in fnp.lengths_around(a, b, 1536)])
def test_logmel_stage_frame_count_steps(dev, sr_in, sr_out, L, pad_mode):
    """resampled lengths one below, at and one above a multiple of the hop (6, 7, 7 frames when downsampling), through the resampler and through k_mono"""
    fe = front_end(sr_in, sr_out, DEFAULT, pad_mode)
    wav = fnp.noisy_clip(7, 2, L, sr_in)
    res, feat = run(fe, wav, dev)
    assert feat.shape[0] == 1 + res.size // 256
    if sr_in >= sr_out:
        assert res.size in (1535, 1536, 1537)
    check_first_stage(wav, sr_in, sr_out, res, "frame-count")
    check_logmel(fe, DEFAULT, pad_mode, res, feat, "frame-count")


@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_smallest_reflect_clip(dev, setting):
    """N = n_fft / 2 + 1: the last frame reflects about sample N - 1 all the way back to sample 1"""
    n_fft, hop, n_mels, win = setting
    fe = front_end(16000, 16000, setting, "reflect")
    wav = fnp.noisy_clip(9, 1, n_fft // 2 + 1, 16000)
    res, feat = run(fe, wav, dev)
    assert res.tobytes() == wav[0].tobytes()                                   # the mean of one channel is the channel
    check_logmel(fe, setting, "reflect", res, feat, "smallest-reflect")
    with pytest.raises(_lib.EtudeHipError, match="reflect pad undefined"):
        run(fe, wav[:, :-1], dev)


def test_smallest_reflect_clip_after_resampling(dev):
    L = fnp.lengths_around(44100, 16000, 1025)[1]
    fe = front_end(44100, 16000)
    wav = fnp.noisy_clip(10, 2, L, 44100)
    res, feat = run(fe, wav, dev)
    assert res.size == 1025 and feat.shape[0] == 5
    check_first_stage(wav, 44100, 16000, res, "smallest-reflect")
    check_logmel(fe, DEFAULT, "reflect", res, feat, "smallest-reflect")
    with pytest.raises(_lib.EtudeHipError, match="reflect pad undefined"):
        run(fe, wav[:, :L - 3], dev)


@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_smallest_constant_clips(dev, setting):
    """zero padding has no shortest clip: one sample, one short of a hop (one frame), a whole hop (two frames)"""
    n_fft, hop, n_mels, win = setting
    fe = front_end(16000, 16000, setting, "constant")
    for N in (1, hop - 1, hop):
        wav = fnp.noisy_clip(N % 7, 1, N, 16000)
        res, feat = run(fe, wav, dev)
        assert feat.shape[0] == (2 if N == hop else 1)
        check_logmel(fe, setting, "constant", res, feat, "smallest-constant")


def test_empty_bands_read_the_log_offset(dev):
    setting = (64, 16, 256, 64)
    assert setting in fnp.SETTINGS
    from etude_amd.frontend import _mel_csr
    start, length, w = _mel_csr(33, 8000.0, 256, 16000)
    empty = np.flatnonzero(length == 0)
    assert empty.size >= 1 and (length == 1).any()
    for pad_mode in fnp.PAD_MODES:
        fe = front_end(16000, 16000, setting, pad_mode)
        _, feat = run(fe, fnp.noisy_clip(2, 2, fnp.clip_len(64, 16), 16000), dev)
        _, quiet = run(fe, np.zeros((1, 40), np.float32), dev)
        assert len(set(quiet.reshape(-1).view(np.int32).tolist())) == 1
        assert (feat[:, empty].view(np.int32) == quiet.view(np.int32)[0, 0]).all()


# ---------------------------------------------------------------------------------------------------- exact tests
@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_silence_is_exactly_the_log_offset(dev, setting, pad_mode):
    n_fft, hop, n_mels, win = setting
    _, feat = run(front_end(16000, 16000, setting, pad_mode), np.zeros((2, fnp.clip_len(n_fft, hop)), np.float32), dev)
    want = np.float32(np.log(np.float64(fnp.LOG_OFFSET)))                      # log(fp32(1e-8)) correctly rounded to fp32
    assert feat.view(np.int32).min() == feat.view(np.int32).max() == want.view(np.int32), (feat.min(), feat.max(), want)


def test_silence_through_the_resampler(dev):
    res, feat = run(front_end(44100, 16000), np.zeros((2, 3000), np.float32), dev)
    assert not res.view(np.int32).any()                                          # +0.0 everywhere: fmaf(w, +0, +0) cannot make a -0
    assert (feat.view(np.int32) == np.float32(np.log(np.float64(fnp.LOG_OFFSET))).view(np.int32)).all()


@pytest.mark.parametrize("sr_in,sr_out,L,setting,pad_mode", [(44100, 16000, 3529, DEFAULT, "reflect"), (16000, 22050, 1500, fnp.SETTINGS[4], "constant"),
                                                            (16000, 16000, 8500, fnp.SETTINGS[6], "reflect")])
def test_run_to_run(dev, sr_in, sr_out, L, setting, pad_mode):
    fe = front_end(sr_in, sr_out, setting, pad_mode)
    wav = fnp.noisy_clip(1, 3, L, sr_in)
    a, b = run(fe, wav, dev), run(fe, wav, dev)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    r = rms(a[0], 65, 7, dev)
    assert r.tobytes() == rms(a[0], 65, 7, dev).tobytes()


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (16000, 22050), (48000, 16000)])
@pytest.mark.parametrize("j", [3, 13])
def test_resampler_shift_invariance(dev, sr_in, sr_out, j):
    """A clip delayed by j input blocks (j no multiple of the 8 blocks a workgroup shares, so every output moves to another slot of another workgroup) gives the
    same output delayed by j * new samples, bit for bit: an output is one fmaf chain over its K taps in tap order, wherever it sits.

    Zeros prepended: samples before the clip count as zeros anyway, so EVERY output from j * new on is identical; of the j * new outputs before, block b (outputs
    b * new ..) reads inputs up to b * orig + orig + width - 1 of the delayed clip and is exactly zero while that stays below j * orig.
    Arbitrary samples prepended: output block b of the original reads inputs from b * orig - width, so blocks b >= ceil(width / orig) never saw the seam and are
    identical; the blocks before read up to `width` samples that were zeros in one run and are not in the other."""
    orig, new, width, K = fnp.pair_dims(sr_in, sr_out)
    fe = front_end(sr_in, sr_out)
    L = 10 * orig + 17 if orig > 8 else 40 * orig + 1
    x = fnp.ramp(L)[None]
    y, _ = run(fe, x, dev, features=False)
    z, _ = run(fe, np.concatenate([np.zeros((1, j * orig), np.float32), x], axis=1), dev, features=False)
    assert z.size == y.size + j * new and z[j * new:].tobytes() == y.tobytes()
    quiet_blocks = max(0, (j * orig - width) // orig)                            # blocks b with (b + 1) * orig + width - 1 < j * orig
    assert not z[:quiet_blocks * new].view(np.int32).any()
    if width < j * orig:
        assert z[:j * new].any()                                                # the filter's pre-ringing is there
    pre = (fnp.ramp(j * orig + 5)[5:] * np.float32(0.7) + np.float32(0.2))[None]
    a, _ = run(fe, np.concatenate([pre, x], axis=1), dev, features=False)
    b0 = -(-width // orig)                                                       # first block whose taps all lie inside the original clip
    assert a[(j + b0) * new:].tobytes() == y[b0 * new:].tobytes()
    assert a[j * new:(j + b0) * new].tobytes() != y[:b0 * new].tobytes()         # and the seam is where it is stated to be


@pytest.mark.parametrize("pad_mode", fnp.PAD_MODES)
@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_frame_shift_invariance(dev, setting, pad_mode):
    """Interior frames -- t * hop - n_fft / 2 >= 0 and t * hop + n_fft / 2 <= N, the window touches neither end -- do not know where they are: frame t of x is
    frame t + 1 of x with one hop of other samples in front, bit for bit."""
    n_fft, hop, n_mels, win = setting
    fe = front_end(16000, 16000, setting, pad_mode)
    N = 3 * n_fft + hop + 5
    x = fnp.ramp(N)
    _, f0 = run(fe, x[None], dev)
    _, f1 = run(fe, np.concatenate([fnp.ramp(hop + 9)[9:] * np.float32(0.5), x])[None], dev)
    interior = [t for t in range(f0.shape[0]) if t * hop - n_fft // 2 >= 0 and t * hop + n_fft // 2 <= N]
    assert len(interior) >= 2 and interior[0] > 0 and interior[-1] < f0.shape[0] - 1
    assert f1[[t + 1 for t in interior]].tobytes() == f0[interior].tobytes()
    assert f1[1].tobytes() != f0[0].tobytes()                                  # the first frame is not interior: it saw padding


@pytest.mark.parametrize("setting", fnp.SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_zero_pad_first_frame_ignores_what_follows(dev, setting):
    """constant mode: the first frame covers samples [-n_fft / 2, n_fft / 2); whatever comes after them does not change a bit of it"""
    n_fft, hop, n_mels, win = setting
    fe = front_end(16000, 16000, setting, "constant")
    x = fnp.ramp(n_fft // 2)
    _, f0 = run(fe, x[None], dev)
    _, f1 = run(fe, np.concatenate([x, fnp.ramp(2 * n_fft + 3) + np.float32(0.3)])[None], dev)
    assert f1[0].tobytes() == f0[0].tobytes()
    assert f0.shape[0] == 1 or f1[:f0.shape[0]].tobytes() != f0.tobytes()      # a later frame does reach them


@pytest.mark.parametrize("setting", [fnp.SETTINGS[0], fnp.SETTINGS[2], fnp.SETTINGS[4]], ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("where", ["0", "1", "N-2", "N-1"])
def test_single_tap_reflection(dev, setting, where):
    """A clip of zeros with one sample set, in reflect mode.  Samples 0 and N - 1 are the mirrors themselves and appear once in the padded signal, samples 1 and
    N - 2 twice; the restatement (numpy's reflect padding) says at which window positions.  Frames the tap does not reach are exactly the log offset."""
    n_fft, hop, n_mels, win = setting
    N = n_fft + 3 * hop + 1
    p = {"0": 0, "1": 1, "N-2": N - 2, "N-1": N - 1}[where]
    x = np.zeros((1, N), np.float32)
    x[0, p] = 0.5
    fe = front_end(16000, 16000, setting, "reflect")
    res, feat = run(fe, x, dev)
    assert res.tobytes() == x[0].tobytes()
    fr = fnp.frames_of(x[0], n_fft, hop, "reflect")
    assert int((fr[0] != 0).sum()) == {"0": 1, "1": 2}.get(where, 0) and int((fr[-1] != 0).sum()) == {"N-1": 1, "N-2": 2}.get(where, 0)
    check_logmel(fe, setting, "reflect", res, feat, "single-tap-" + where)
    silent = ~(fr * fnp.window_table(n_fft, win)[None] != 0).any(axis=1)
    assert silent.any() and not silent.all()
    assert (feat[silent].view(np.int32) == np.float32(np.log(np.float64(fnp.LOG_OFFSET))).view(np.int32)).all()


# ---------------------------------------------------------------------------------------------------- RMS frames
@pytest.mark.parametrize("hop", fnp.RMS_HOPS)
@pytest.mark.parametrize("frame", fnp.RMS_FRAMES)
def test_rms_frames(dev, frame, hop):
    """frames shorter than, equal to and longer than a wave (one wave sums a frame), 7 / 8 / 9 frames (four share a workgroup), lengths that are and are not
    multiples of the hop"""
    for q in fnp.RMS_QUOTIENTS:
        for n in (q * hop, q * hop + min(hop - 1, 5)):
            x = fnp.noisy_clip(q, 1, n, 22050)[0]
            got = rms(x, frame, hop, dev)
            assert got.size == q + 1
            check_rms(x, frame, hop, got, "direct")


def test_rms_last_frame_with_one_sample(dev):
    """frame 2, n a multiple of the hop: the last frame covers [n - 1, n + 1), all padding but the last sample"""
    for hop in fnp.RMS_HOPS:
        n = 7 * hop
        x = fnp.ramp(n) + np.float32(0.5)
        got = rms(x, 2, hop, dev)
        want = check_rms(x, 2, hop, got, "last-frame")
        # one square, one division, one square root in fp32: each within an ulp or so of the exact value, 4 * 2^-24 in all
        assert abs(want[-1] - abs(float(x[-1])) / np.sqrt(2.0)) <= 1e-15 and abs(got[-1] - want[-1]) <= FLOOR * want[-1]
    got = rms(np.array([0.25], np.float32), 2204, 1102, dev)                      # one sample, one frame, 2203 zeros
    assert got.shape == (1,) and abs(got[0] - 0.25 / np.sqrt(2204.0)) <= FLOOR * 0.25 / np.sqrt(2204.0)


@pytest.mark.parametrize("channels", [2, 3])
def test_rms_on_the_devices_resampled_buffer(dev, channels):
    """analyze_volume's chain: FrontEnd(sr, 22050, pad_mode="constant") without features, then frame 2204 / hop 1102 on that buffer where it lies"""
    fe = front_end(44100, 22050, DEFAULT, "constant")
    L = 2 * 8 * 1102 + 3
    wav = fnp.noisy_clip(4, channels, L, 44100) * np.linspace(0.1, 1.0, L, dtype=np.float32)[None]
    lib = _lib.lib()
    n = int(lib.etd_frontend_resampled_len(fe.h, L))
    res = Guarded(n, dev)
    w = torch.from_numpy(np.ascontiguousarray(wav)).to(dev)
    _lib.check(lib.etd_frontend_run(fe.h, w.data_ptr(), channels, L, res.ptr, None, 0, None, None), "etd_frontend_run")
    r = res.read()
    check_first_stage(wav, 44100, 22050, r, "volume")
    got = rms(None, 2204, 1102, dev, x_dev=res.buf[GUARD:GUARD + n].view(torch.float32))
    want = check_rms(r, 2204, 1102, got, "volume")
    assert want[-2] > 2 * want[1]                                              # the crescendo is there


# ---------------------------------------------------------------------------------------------------- the resampler's LDS request
def test_rate_pair_beyond_the_lds_limit_is_refused(dev):
    """k_resample keeps 7 * orig + K input samples in dynamic LDS.  A pair with a large orig asks for more than a workgroup may have; etd_frontend_create refuses
    it against the limit the device reports (160 KiB on an MI355X), naming the pair, before anything is uploaded or launched.  The pairs are orig -> 1 Hz (one
    phase, K = 2 * ceil(6 * orig / 0.99) + orig, a table of K floats): the smallest orig beyond the limit is refused, the one before it -- the largest request
    the library accepts -- runs and is right.  Nothing is ever launched with an oversized request."""
    from etude_amd.frontend import FrontEnd
    limit = int(torch.cuda.get_device_properties(0).shared_memory_per_block)
    assert limit >= 16 * 1024

    def lds_bytes(a, b):
        orig, new, width, K = fnp.pair_dims(a, b)
        return 4 * ((fnp.RB - 1) * orig + K)

    sr = next(s for s in range(2, 1 << 20) if lds_bytes(s, 1) > limit)
    assert lds_bytes(sr - 1, 1) <= limit < lds_bytes(sr, 1)
    with pytest.raises(_lib.EtudeHipError) as e:
        FrontEnd(sr, 1)
    msg = str(e.value)
    assert "rc=-22" in msg and f"resampling {sr} -> 1 Hz" in msg and f"needs {lds_bytes(sr, 1)} bytes of LDS" in msg and f"allows {limit}" in msg
    with pytest.raises(_lib.EtudeHipError, match="bytes of LDS"):                  # and a pair with a common factor, far beyond
        FrontEnd(3 * (sr + 500), 3)
    # the largest accepted request launches and is right (two workgroups, the second one short)
    fe = FrontEnd(sr - 1, 1)
    wav = fnp.noisy_clip(3, 2, 11 * (sr - 1) + 5, sr - 1)
    res, _ = run(fe, wav, dev, features=False)
    fe.close()
    assert res.size == 12
    check_first_stage(wav, sr - 1, 1, res, "largest-lds")
    # the library is unharmed: an ordinary pair created afterwards runs and is right
    fe = FrontEnd(44100, 16000)
    wav = fnp.noisy_clip(3, 2, 3000, 44100)
    res, feat = run(fe, wav, dev)
    fe.close()
    check_first_stage(wav, 44100, 16000, res, "after-refusal")
    assert np.isfinite(feat).all()
