"""Audio loading without a GPU (etude_amd.audio, csrc/resample.hip's host side) against the fp64 restatement of DESIGN.md 4q (tests/audio_np.py): the filter design,
N', the walk over a WAV's chunks with the decode rules against ``extractor.read_wav`` bit for bit, the refusals, and the C ABI's plan of a ragged batch."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import audio_np as au  # noqa: E402

from etude_amd import audio  # noqa: E402
from etude_amd._lib import EtudeHipError  # noqa: E402
from etude_amd.extractor import read_wav  # noqa: E402

PAIRS = [(44100, 22050, "best"), (48000, 22050, "best"), (44100, 16000, "best"), (22050, 44100, "best"), (8000, 22050, "best"), (48000, 44100, "fast")]


@pytest.mark.parametrize("sr_in,sr_out,quality", PAIRS)
def test_filter_matches_restatement_and_is_symmetric(sr_in, sr_out, quality):
    tab, up, down, half = audio.resample_filter(sr_in, sr_out, quality)
    ref, rup, rdown, rhalf = au.filter_table(sr_in, sr_out, quality)
    assert (up, down, half) == (rup, rdown, rhalf) and tab.shape == ref.shape == (up, 2 * half) and tab.dtype == np.float64
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    assert (np.abs(tab - ref) <= 1e-14 * rowmax).all(), float((np.abs(tab - ref) / rowmax).max())
    # h(-t) = h(t): row p reversed is row up - p; row 0 reversed is itself one tap later (its last tap is t = half, outside or at the edge of the window)
    for p in range(1, up):
        assert np.array_equal(tab[p][::-1], tab[up - p]), p
    assert np.array_equal(tab[0][:-1][::-1], tab[0][:-1])
    # the pass band has unit gain: every phase's taps sum to about 1 (the residue is the stop-band leakage of the window)
    assert np.abs(tab.sum(axis=1) - 1.0).max() < 2e-3


def test_resampled_len_is_the_exact_ceiling():
    for sr_in, sr_out, _ in PAIRS:
        up, down, _ = au.shape(sr_in, sr_out)
        for n in (1, 2, 319, 320, 321, 10 ** 9 + 7):
            want = (n * up + down - 1) // down
            assert audio.resampled_len(n, sr_in, sr_out) == want == au.out_len(n, sr_in, sr_out)
            r = audio.Resampler(sr_in, sr_out)
            assert r.out_len(n) == want
            r.close()


# ---------------------------------------------------------------------------------------------------------------- files
_chunk, _riff, _fmt, _pcm_bytes, write_case, KINDS = au._chunk, au._riff, au._fmt, au._pcm_bytes, au.write_case, au.KINDS


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_read_wav_raw_and_the_decode_rules_equal_read_wav(tmp_path, kind, ch):
    rng = np.random.default_rng(7 * ch + len(kind))
    p = tmp_path / f"{kind}_{ch}.wav"
    want_fmt = write_case(p, kind, 301, ch, 32000, rng)
    raw, fmt, C, sr, frames = audio.read_wav_raw(p)
    assert (fmt, C, sr, frames) == (want_fmt, ch, 32000, 301) and raw.dtype == np.uint8 and raw.size == 301 * ch * audio.WIDTH[fmt]
    x, sr0 = read_wav(p)
    got = au.decode(raw, fmt, C)
    assert sr0 == sr and got.dtype == x.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_read_wav_raw_clips_a_data_size_past_the_end_to_whole_frames(tmp_path):
    rng = np.random.default_rng(3)
    body = _pcm_bytes(rng, 16, 50, 2)
    whole = _riff([_fmt(1, 2, 44100, 16), _chunk(b"data", body)])
    p = tmp_path / "cut.wav"
    p.write_bytes(whole[:-7])                                   # the header still promises 200 bytes; 193 are there: 48 whole frames
    raw, fmt, C, sr, frames = audio.read_wav_raw(p)
    assert (fmt, C, sr, frames) == ("S16", 2, 44100, 48) and raw.tobytes() == body[:192]


def test_read_wav_raw_refusals_name_the_path(tmp_path):
    data = _chunk(b"data", b"\0" * 16)
    cases = {
        "notriff": b"RIFX" + _riff([_fmt(1, 1, 8000, 16), data])[4:],
        "datafirst": _riff([data, _fmt(1, 1, 8000, 16)]),
        "compressed": _riff([_fmt(2, 1, 8000, 4), data]),          # ADPCM
        "mulaw": _riff([_fmt(7, 1, 8000, 8), data]),
        "nochannels": _riff([_fmt(1, 0, 8000, 16), data]),
        "nodata": _riff([_fmt(1, 1, 8000, 16)]),
    }
    for name, blob in cases.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=name):
            audio.read_wav_raw(p)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_create_needs_no_gpu_and_refuses_a_table_above_the_budget():
    for sr_in, sr_out, quality in PAIRS + [(22050, 22050, "best")]:
        r = audio.Resampler(sr_in, sr_out, quality)
        assert r.h.value and (r.up, r.down, r.half) == au.shape(sr_in, sr_out, quality)
        r.close()
        r.close()
    with pytest.raises(EtudeHipError, match="22051.*entries"):
        audio.Resampler(44100, 22051)
    with pytest.raises(ValueError):
        audio.Resampler(44100, 22050, "medium")


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 22050), (22050, 44100), (44100, 44100)])
def test_plan_tiles_every_output_exactly_once(sr_in, sr_out):
    r = audio.Resampler(sr_in, sr_out)
    lengths = [1, 255, 256, 257, 1000]
    frames = [n for n in lengths for _ in (1, 2)]
    channels = [c for _ in lengths for c in (1, 2)]
    for mono in (False, True):
        plan = r.plan(frames, channels, [mono] * len(frames))
        seen = {}
        for song, ch, n0, cnt in plan.tolist():
            nout = au.out_len(frames[song], sr_in, sr_out)
            assert 0 <= ch < (1 if mono else channels[song]) and n0 % 256 == 0 and 1 <= cnt <= 256 and n0 + cnt <= nout      # one (song, channel) per tile
            cover = seen.setdefault((song, ch), np.zeros(nout, np.int64))
            cover[n0: n0 + cnt] += 1
        assert set(seen) == {(s, c) for s in range(len(frames)) for c in range(1 if mono else channels[s])}
        assert all((v == 1).all() for v in seen.values())
        assert r.workspace_bytes(frames, channels, [mono] * len(frames)) >= 16 * len(plan)
    r.close()


def test_plan_refuses_bad_shapes():
    r = audio.Resampler(48000, 22050)
    for frames, channels in (([10], [0]), ([10], [9]), ([0], [1])):
        with pytest.raises(EtudeHipError):
            r.workspace_bytes(frames, channels, [False])
    r.close()
