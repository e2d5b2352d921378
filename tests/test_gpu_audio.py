"""Audio loading on the MI355X (csrc/resample.hip, etude_amd.AudioLoader) against the fp64 restatement of DESIGN.md 4q (tests/audio_np.py).

Decoding is exact: a file loaded at its own rate equals ``extractor.read_wav`` bit for bit.  Indexing is exact: a unit impulse reads the fp32 table back, entry by
entry.  Accuracy, on the kernel's own decoded input, for EVERY output n:  |y_dev[n] - y_ref64[n]| <= (K + 2) 2^-24 A[n],  A[n] = sum_k |h_k| |x_k|  -- one 2^-24 for
the table's rounding to fp32, K for the fmaf chain (each step rounds a partial sum no larger than A[n]), one for slack in the last rounding; nothing measured.
Then the plan's edges (a song is bit-identical alone, in a ragged batch, from run to run, and between neighbours of constant 1.0), the grouping by source rate,
and the chains that start from paths."""
import json
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import audio_np as au  # noqa: E402

from etude_amd.extractor import read_wav  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def _loader(quality="best"):
    from etude_amd.audio import AudioLoader
    if quality not in _cache:
        _cache[quality] = AudioLoader(quality=quality)
    return _cache[quality]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _write_s16(path, x, sr):
    """float [C][N] in [-1, 1) -> 16-bit PCM through the stdlib wave module"""
    x = np.atleast_2d(np.asarray(x))
    v = np.clip(np.round(x.T * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[0]); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(v.tobytes())


def _write_f32(path, x, sr):
    x = np.atleast_2d(np.asarray(x, np.float32))
    path.write_bytes(au._riff([au._fmt(3, x.shape[0], sr, 32), au._chunk(b"data", np.ascontiguousarray(x.T).astype("<f4").tobytes())]))


# ---------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_a_file_at_its_own_rate_equals_read_wav_bit_for_bit(tmp_path, ch):
    rng = np.random.default_rng(40 + ch)
    paths = []
    for kind in au.KINDS:
        for frames in (301, 1):
            p = tmp_path / f"{kind}_{frames}.wav"
            au.write_case(p, kind, frames, ch, 32000, rng)
            paths.append(p)
    full = _loader().load_many(paths, 32000)
    mono = _loader().load_many(paths, 32000, mono=True)
    for p, a, m in zip(paths, full, mono):
        x, _ = read_wav(p)
        assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == x.shape and tuple(m.shape) == x.shape[1:], p.name
        assert np.array_equal(_bits(a), x.view(np.uint32)), p.name
        assert np.array_equal(_bits(m), au.mono_mean(x).view(np.uint32)), p.name


# ---------------------------------------------------------------------------------------------------------------- indexing
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 22050), (22050, 44100)])
def test_a_unit_impulse_reads_the_table_back_entry_by_entry(tmp_path, sr_in, sr_out):
    tab, up, down, half = au.filter_table(sr_in, sr_out)
    tab32 = tab.astype(np.float32)
    N = 700
    where = (0, N - 1, 333)
    paths = []
    for j in where:
        x = np.zeros(N, np.float32)
        x[j] = 1.0
        paths.append(tmp_path / f"imp{j}.wav")
        _write_f32(paths[-1], x, sr_in)
    n = np.arange(au.out_len(N, sr_in, sr_out), dtype=np.int64)
    i0, p = (n * down) // up, (n * down) % up
    for j, y in zip(where, _loader().load_many(paths, sr_out, mono=True)):
        k = j - (i0 - half + 1)                              # the tap of output n that meets sample j
        inside = (k >= 0) & (k < 2 * half)
        want = np.where(inside, tab32[p, np.clip(k, 0, 2 * half - 1)], np.float32(0))
        assert tuple(y.shape) == (n.size,) and inside.any() and not inside.all()
        assert np.array_equal(_bits(y), want.view(np.uint32)), j
        assert (_bits(y)[~inside] == 0).all()                # +0.0f outside the window


# ---------------------------------------------------------------------------------------------------------------- accuracy
def _noise_s16(tmp_path, N, sr, seed, ch=2):
    rng = np.random.default_rng(seed)
    p = tmp_path / f"noise_{N}_{sr}.wav"
    _write_s16(p, rng.random((ch, N)) * 2 - 1, sr)
    return p


def _check_bound(y, x, sr_in, sr_out, quality, what):
    ref, A = au.resample_ref(x, sr_in, sr_out, quality)
    K = 2 * au.shape(sr_in, sr_out, quality)[2]
    y = y.cpu().numpy().astype(np.float64)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    err, bound = np.abs(y - ref), (K + 2) * 2.0 ** -24 * A
    worst = int(np.argmax(err - bound))
    print(f"AUDIO_ERR {what}: {y.size} outputs, K {K}, max err/bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f} (output {worst}: err {err[worst]:.3e}, bound {bound[worst]:.3e})")
    assert (err <= bound).all(), (what, worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("sr_in,sr_out,quality", [(44100, 22050, "best"), (48000, 22050, "best"), (44100, 16000, "best"), (8000, 22050, "best"), (48000, 44100, "fast")])
def test_every_output_is_within_the_derived_bound_of_fp64(tmp_path, sr_in, sr_out, quality):
    K = 2 * au.shape(sr_in, sr_out, quality)[2]
    paths = [_noise_s16(tmp_path, N, sr_in, 100 + N) for N in (4099, 1, 2, K - 1)]
    ld = _loader(quality)
    full, mono = ld.load_many(paths, sr_out), ld.load_many(paths, sr_out, mono=True)
    for p, a, m in zip(paths, full, mono):
        x, _ = read_wav(p)                                   # (what the kernel decodes, bit for bit: the test above)
        for c in range(2):
            _check_bound(a[c], x[c], sr_in, sr_out, quality, f"{sr_in}->{sr_out} {quality} N {x.shape[1]} channel {c}")
        _check_bound(m, au.mono_mean(x), sr_in, sr_out, quality, f"{sr_in}->{sr_out} {quality} N {x.shape[1]} mono")


# ---------------------------------------------------------------------------------------------------------------- the plan's edges
def test_a_song_is_bit_identical_alone_in_a_ragged_batch_and_again(tmp_path):
    rng = np.random.default_rng(5)
    paths = []
    for i, N in enumerate((1, 255, 256, 257, 513, 4099)):
        for ch in (1, 2, 3):
            p = tmp_path / f"s{N}_{ch}.wav"
            au.write_case(p, au.KINDS[(i + ch) % len(au.KINDS)], N, ch, 48000, rng)
            paths.append(p)
    ld = _loader()
    for sr, mono in ((22050, False), (22050, True), (48000, False)):
        batch = ld.load_many(paths, sr, mono)
        again = ld.load_many(paths[::-1], sr, mono)[::-1]
        for p, b, a in zip(paths, batch, again):
            alone = ld.load(p, sr, mono)
            assert torch.equal(alone, b) and torch.equal(alone, a), (p.name, sr, mono)


def test_no_read_crosses_into_a_neighbours_samples():
    """three songs back to back in ONE device buffer, the outer two constant 1.0: the middle one's outputs are those of the song in a buffer of its own"""
    rs = _loader().resampler(48000, 22050)
    rng = np.random.default_rng(9)
    for N, ch in ((257, 1), (300, 2)):
        x = (rng.random((ch, N)) * 2 - 1).astype(np.float32)
        inter = np.ascontiguousarray(x.T).reshape(-1)
        ones = np.ones(512 * ch, np.float32)
        buf = torch.from_numpy(np.concatenate([ones, inter, ones])).cuda()
        a, b = ones.size, ones.size + inter.size
        srcs = [buf[:a].view(torch.uint8), buf[a:b].view(torch.uint8), buf[b:].view(torch.uint8)]
        got = rs.run_many(srcs, [512, N, 512], [ch] * 3, ["F32"] * 3, [False] * 3)
        alone = rs.run_many([torch.from_numpy(inter).cuda().view(torch.uint8)], [N], [ch], ["F32"], [False])[0]
        planar = _loader().resample_many([x], 48000, 22050)[0]
        assert torch.equal(got[1], alone) and torch.equal(planar, alone)
        for c in range(ch):
            _check_bound(alone[c], x[c], 48000, 22050, "best", f"sandwich N {N} channel {c}")


def test_refusals_come_before_any_launch():
    from etude_amd._lib import EtudeHipError
    rs = _loader().resampler(48000, 22050)
    src = torch.zeros(400, dtype=torch.uint8, device="cuda")
    for frames, ch, fmt, what in ((100, 2, "S16", None), (99, 2, "S16", "bytes"), (50, 9, "U8", "channels"), (50, 0, "U8", "channels")):
        if what is None:
            assert tuple(rs.run_many([src], [frames], [ch], [fmt], [False])[0].shape) == (2, au.out_len(100, 48000, 22050))
            continue
        with pytest.raises(EtudeHipError, match=what):
            rs.run_many([src], [frames], [ch], [fmt], [False])
    with pytest.raises(ValueError, match="non-finite"):
        _loader().resample_many([np.array([0.0, np.nan], np.float32)], 48000, 22050)
    from etude_amd.audio import AudioLoader
    with pytest.raises(EtudeHipError, match="no CPU path"):
        AudioLoader(device="cpu").resample_many([np.zeros(8, np.float32)], 48000, 22050)


# ---------------------------------------------------------------------------------------------------------------- grouping
def test_files_of_three_rates_come_back_in_input_order(tmp_path):
    rates = (44100, 48000, 22050, 48000, 44100, 22050, 44100)
    paths = [_noise_s16(tmp_path, 900 + 37 * i, sr, 300 + i, ch=1 + i % 2) for i, sr in enumerate(rates)]
    ld = _loader()
    got = ld.load_many(paths, 22050, mono=True)
    assert set(ld._resamplers) >= {(44100, 22050), (48000, 22050), (22050, 22050)}
    for i, (p, sr, y) in enumerate(zip(paths, rates, got)):
        assert tuple(y.shape) == (au.out_len(900 + 37 * i, sr, 22050),)
        assert torch.equal(y, ld.load(p, 22050, mono=True)), p.name
    fn = ld.as_load_fn()
    assert torch.equal(fn(paths[1]), got[1])


# ---------------------------------------------------------------------------------------------------------------- chains
def _music(sr, seconds, seed, channels=2):
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * seconds)) / sr
    notes = rng.choice([220.0, 261.63, 329.63, 392.0, 440.0, 523.25], size=8)
    x = sum(0.08 * np.sin(2 * np.pi * f * t + i) * (1.0 + np.sin(2 * np.pi * (0.5 + 0.25 * i) * t)) for i, f in enumerate(notes))
    return np.stack([x * (1.0 - 0.1 * c) + 0.01 * rng.standard_normal(t.size) for c in range(channels)])


def test_tuning_and_alignment_from_files_equal_the_chains_on_the_loaders_output(tmp_path):
    from etude_amd.aligner import align_audio_many, align_files_many
    from etude_amd.tuning import TuningEstimator
    cover, origin = tmp_path / "cover.wav", tmp_path / "origin.wav"
    _write_s16(cover, _music(48000, 1.6, 1), 48000)          # 76 800 frames -> 35 280 samples at 22 050 Hz: above the estimator's two windows
    _write_s16(origin, _music(48000, 1.7, 2), 48000)
    ld = _loader()
    wavs = [ld.load(p, 22050, mono=True) for p in (cover, origin)]
    est = TuningEstimator()
    assert np.array_equal(est.estimate_files_many([cover, origin], ld), est.estimate_many(wavs))
    assert np.array_equal(est.estimate_files_many([cover, origin]), est.estimate_many(wavs))       # (the default loader)
    got, want = align_files_many([(cover, origin)], ld)[0], align_audio_many([(wavs[0], wavs[1])], "estimate")[0]
    assert np.array_equal(got["wp"], want["wp"]) and got["pitch_shift"] == want["pitch_shift"]
    assert (got["num_frames_cover"], got["num_frames_origin"]) == (want["num_frames_cover"], want["num_frames_origin"])


def test_structuralize_files_many_equals_structuralize_audio_many_on_the_loaders_output(tmp_path):
    from etude_amd import structuralize_audio_many, structuralize_files_many, synth
    from etude_amd.beat import BeatDetector
    from etude_amd.separator import SeparatorConfig, StemSeparator, init_separator_state
    det = BeatDetector(state_dict=synth.beat_state_dict(20240607), tracker="native")
    cfg = SeparatorConfig(instruments=("vocals", "piano", "drums", "bass", "other"), n_fft=1024, hop=256, T=64, F=64, conv_n_filters=(16, 32, 64, 128, 256, 512))
    sep = StemSeparator(cfg, init_separator_state(cfg, 4))
    paths = [tmp_path / "stereo48.wav", tmp_path / "mono44.wav"]
    _write_s16(paths[0], _music(48000, 3.0, 5), 48000)
    _write_s16(paths[1], _music(44100, 3.0, 6, channels=1), 44100)
    ld = _loader()
    wavs = ld.load_many(paths, cfg.sample_rate)
    assert [tuple(w.shape) for w in wavs] == [(2, 132300), (1, 132300)]
    got = structuralize_files_many(det, sep, paths, ld)
    assert got == structuralize_audio_many(det, sep, wavs) and len(got) == 2


def test_evaluate_many_loads_an_origin_of_any_rate_with_a_loader(tmp_path):
    from etude_amd.render import NOTE_DTYPE, NoteRenderer, PianoVoice
    from etude_amd.rhythm import evaluate_many
    rng = np.random.default_rng(21)
    on = np.sort(rng.random(40) * 8.0)
    piece = np.array([(o, o + 0.15 + float(rng.random()) * 0.6, int(rng.integers(36, 97)), int(rng.integers(50, 120))) for o in on], NOTE_DTYPE)
    r = NoteRenderer(22050, PianoVoice())
    moved = piece.copy()
    moved["onset"], moved["offset"] = 1.05 * piece["onset"] + 0.25, 1.05 * piece["offset"] + 0.25
    origin = r.render(moved).cpu().numpy().astype(np.float64)
    origin = 0.5 * origin / max(1.0, float(np.abs(origin).max()))
    d = tmp_path / "song"
    d.mkdir()
    _write_s16(d / "origin.wav", np.stack([np.repeat(origin, 2), 0.5 * np.repeat(origin, 2)]), 44100)      # stereo at 44.1 kHz
    (d / "a.json").write_text(json.dumps([dict(onset=float(n["onset"]), offset=float(n["offset"]), pitch=int(n["pitch"]), velocity=int(n["velocity"])) for n in piece]))
    meta = [{"dir_name": "song"}]
    with pytest.raises(ValueError, match="22050"):
        evaluate_many(tmp_path, meta, ["a"], renderer=r)
    rows = evaluate_many(tmp_path, meta, ["a"], renderer=r, loader=_loader())
    assert [row["version"] for row in rows] == ["a"] and np.isfinite(rows[0]["wpd_score"]) and rows[0]["wpd_score"] >= 0
