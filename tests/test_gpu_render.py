"""The note renderer on the MI355X (csrc/render.hip, etude_amd.NoteRenderer) against the fp64 restatement of DESIGN.md 4l (tests/render_np.py).

The bound.  err = max_n |x_dev[n] - x64[n]| / max_n envsum[n], against the float64 restatement.  err32 is the same figure of the restatement's float32 variant on the
same input, computed here, never hard-coded: the phase is formed and reduced in fp64 in both, and behind that step both are fp32 -- the kernel adds the same terms in
another association and with fused multiply-adds, and evaluates its sine and exponentials differently.  The device is allowed 4 err32, the margin DESIGN.md 4j uses
against fp32 torch.  Every case prints its figures; with ETD_RENDER_REPORT=dir they are also kept as dir/render_accuracy.json (how profiles/render_device.json is
made).  Batch invariance and the peaks are bitwise."""
import json
import math
import os
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import render_np as rn  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 22050
BLK = 1024
_cache = {}
_report = {}


def arr(rows):
    from etude_amd.render import NOTE_DTYPE
    return np.array([tuple(r) for r in rows], NOTE_DTYPE)


def _renderer(sr=SR, voice=None, budget=None):
    from etude_amd.render import NoteRenderer, PianoVoice
    key = (sr, voice, budget)
    if key not in _cache:
        kw = {} if budget is None else {"workspace_budget": budget}
        _cache[key] = NoteRenderer(sr, voice or PianoVoice(), **kw)
    return _cache[key]


def _keep(name, **figures):
    _report[name] = figures
    print(name, figures)
    out = os.environ.get("ETD_RENDER_REPORT")
    if out:
        with open(os.path.join(out, "render_accuracy.json"), "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


def _check(name, notes, sr=SR, cents=0.0, voice=None, num_samples=None, dev=None):
    """one cover against the restatement under the bound -> the device's samples (numpy)"""
    from etude_amd.render import PianoVoice
    v = voice or PianoVoice()
    x64, env = rn.render_np(notes, sr, cents, v, num_samples)
    x32, _ = rn.render_np(notes, sr, cents, v, num_samples, dtype=np.float32)
    if dev is None:
        dev = _renderer(sr, voice).render(arr(notes), cents, num_samples).cpu().numpy()
    assert dev.dtype == np.float32 and dev.shape == x64.shape, (name, dev.shape, x64.shape)
    scale = float(env.max()) if len(env) else 0.0
    if scale == 0.0:
        _keep(name, silent=True, samples=len(dev))
        assert (dev == 0).all(), name
        return dev
    err = float(np.abs(dev - x64).max()) / scale
    err32 = float(np.abs(x32 - x64).max()) / scale
    _keep(name, err=err, err32=err32, ratio=err / err32, samples=len(dev))
    assert np.abs(x64).max() > 0.05 * scale                      # the case is not silent by accident
    assert err <= 4.0 * err32, (name, err, err32)
    return dev


R = 0.48
EDGES = {
    "onset_off_grid": dict(notes=[(0.1003, 0.7, 60, 100)]),
    "onset_zero": dict(notes=[(0.0, 0.6, 57, 100)]),
    "onset_on_block_boundary": dict(notes=[(2 * BLK / SR, 0.5, 64, 100)]),
    "onset_one_sample_before_boundary": dict(notes=[((2 * BLK - 1) / SR, 0.5, 64, 100)]),
    "onset_one_sample_behind_boundary": dict(notes=[((2 * BLK + 1) / SR, 0.5, 64, 100)]),
    "release_ends_at_block_end": dict(notes=[(0.02, 20 * BLK / SR - R, 55, 100)]),
    "shorter_than_attack": dict(notes=[(0.05, 0.052, 72, 100)]),
    "spans_four_blocks_release_off": dict(notes=[(1000 / SR, 4000 / SR, 50, 100)], release=False),
    "velocity_1": dict(notes=[(0.01, 0.5, 60, 1)]),
    "velocity_127": dict(notes=[(0.01, 0.5, 60, 127)]),
    "pitch_21": dict(notes=[(0.01, 1.0, 21, 100)]),
    "pitch_108": dict(notes=[(0.01, 0.5, 108, 100)]),
    "cents_minus_50": dict(notes=[(0.01, 0.5, 69, 100)], cents=-50.0),
    "cents_plus_50": dict(notes=[(0.01, 0.5, 69, 100)], cents=50.0),
    "rate_8000": dict(notes=[(0.0131, 0.5, 60, 100)], sr=8000),
    "rate_8000_silent_note": dict(notes=[(0.01, 0.3, 108, 100)], sr=8000),
    "rate_16000": dict(notes=[(0.0131, 0.5, 60, 100)], sr=16000),
    "rate_44100": dict(notes=[(0.0131, 0.5, 96, 100)], sr=44100),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_one_note(name):
    from etude_amd.render import PianoVoice
    c = EDGES[name]
    voice = None if c.get("release", True) else replace(PianoVoice(), release=False)
    dev = _check("edge/" + name, c["notes"], c.get("sr", SR), c.get("cents", 0.0), voice)
    sr = c.get("sr", SR)
    onset, offset = c["notes"][0][:2]
    first, end = rn.first_end(onset, offset, sr, voice or PianoVoice())
    assert (dev[:first] == 0).all() and (dev[end:] == 0).all()            # exactly 0 outside the support
    if name == "release_ends_at_block_end":
        assert end in (20 * BLK, 20 * BLK + 1) and len(dev) > 20 * BLK
    if name == "pitch_108":
        assert len(rn.partials(108, 100, 0.0, SR)[0]) == 2


def test_chord_of_forty_notes():
    rng = np.random.default_rng(1)
    notes = [(0.1, 0.3 + float(rng.random()), 40 + i, int(rng.integers(30, 128))) for i in range(40)]
    _check("sum/chord_40", notes)


def test_two_onsets_less_than_a_sample_apart():
    a, b = [(0.2, 0.6, 60, 100), (0.2 + 1.0e-5, 0.6, 67, 100)], [(0.2, 0.6, 60, 100), (0.2, 0.6, 67, 100)]
    assert 1.0e-5 * SR < 0.25
    x = _check("sum/two_onsets_0.22_sample_apart", a)
    y = _check("sum/two_onsets_together", b)
    assert not np.array_equal(x, y)                                         # the phase is zero at the exact onset, not at the nearest sample


def test_gap_is_exactly_zero_and_every_sample_is_written():
    """the allocation is filled with a pattern first: a block the kernel does not write would keep it"""
    import torch
    r = _renderer()
    gap0 = 0.3 + R
    notes = [arr([(0.05, 0.3, 60, 100), (0.1, 0.25, 64, 90), (gap0 + 3.0, gap0 + 3.2, 62, 100)]), arr([(0.0, 0.1, 70, 80)]), arr([])]
    p = r.pack(notes, num_samples=[None, None, 3000])
    nn, off, cents, N, soff = r._sub(p, [0, 1, 2])
    flat = torch.full((int(soff[-1]) + 64,), 7.0, dtype=torch.float32, device="cuda")
    r.run_raw(nn, off, cents, N, soff, flat)
    host = flat.cpu().numpy()
    for c in range(3):
        x = host[soff[c]: soff[c] + N[c]]
        _check(f"sum/gap_cover_{c}", notes[c], num_samples=int(N[c]), dev=x)
        assert (host[soff[c] + N[c]: soff[c + 1]] == 7.0).all()            # what lies between two covers is not touched
    assert (host[soff[-1]:] == 7.0).all()
    x = host[: N[0]]
    g0, g1 = math.ceil(gap0 * SR) + 1, math.floor((gap0 + 3.0) * SR) - 1
    assert g1 - g0 > 2.9 * SR and (x[g0:g1] == 0.0).all() and np.abs(x[g1 + 200:]).max() > 1e-3
    assert (host[soff[2]: soff[2] + 3000] == 0.0).all()                     # a cover with no notes: num_samples zeros


def test_late_phase_at_ten_minutes():
    """what an fp32 time base loses: the same note at onset 600 s meets the bound it meets at onset 0"""
    early = _check("late/onset_0", [(0.0, 1.0, 72, 100)])
    late = _check("late/onset_600", [(600.0, 601.0, 72, 100)])
    assert len(late) == rn.length_of([(600.0, 601.0, 72, 100)], SR) > 13.2e6 and (late[: 600 * SR] == 0).all()
    assert np.array_equal(late[600 * SR: 600 * SR + len(early)], early)     # 600 s is a whole number of samples: the very same bits


def _ragged():
    rng = np.random.default_rng(11)
    covers = []
    for n in (0, 1, 7, 300):
        on = np.sort(rng.random(n) * 5.0) if n != 1 else np.array([4.9])      # (the three sounding covers are about as long: no two of them share a budget of one)
        covers.append(arr([(o, o + 0.03 + float(rng.random()) * 0.8, int(rng.integers(21, 109)), int(rng.integers(1, 128))) for o in on]))
    return covers, [0.0, 12.5, -50.0, 3.0]


@pytest.mark.parametrize("given", [False, True])
def test_ragged_batch_is_bit_identical_however_it_is_batched(given):
    import torch
    from etude_amd.render import PianoVoice
    covers, cents = _ragged()
    ns = [777, 120000, 100001, 95000] if given else [None] * 4
    r = _renderer()
    alone = [r.render(c, t, n) for c, t, n in zip(covers, cents, ns)]
    assert alone[0].numel() == (777 if given else 0) and not alone[0].any()
    for c, t, n, x in zip(covers[1:], cents[1:], ns[1:], alone[1:]):
        assert x.numel() == (n if given else rn.length_of(c, SR)) and float(x.abs().max()) > 0
    if not given:
        _check("ragged/300_notes", covers[3], cents=cents[3], dev=alone[3].cpu().numpy())
    together = r.render_many(covers, cents, ns)
    again = r.render_many(covers, cents, ns)
    rev = r.render_many(covers[::-1], cents[::-1], ns[::-1])[::-1]
    p = r.pack(covers, cents, ns)
    need = max(4 * (int(p.num_samples[i]) + 63) // 64 * 64 + r.bytes_for(np.array([0, len(covers[i])], np.int64), p.num_samples[i: i + 1].copy()) for i in range(4))
    small = _renderer(budget=need)                                          # what the largest cover needs alone
    assert len(small.batches(p)) >= 3
    split = small.render_many(covers, cents, ns)
    for i in range(4):
        for other in (together, again, rev, split):
            assert other[i].dtype == torch.float32 and other[i].dim() == 1 and torch.equal(other[i], alone[i]), i


def test_peaks_equal_the_maximum_exactly():
    import torch
    covers, cents = _ragged()
    r = _renderer()
    xs = r.render_many(covers, cents) + [r.render(covers[2], num_samples=1001)[1:], torch.zeros(5, device="cuda")]
    pk = r.peaks_many(xs)
    assert pk.dtype == np.float32 and pk.shape == (6,)
    want = [float(x.abs().max()) if x.numel() else 0.0 for x in xs]
    assert pk.tolist() == want and pk[0] == 0.0 and pk[5] == 0.0 and pk[3] > 0.01
    assert len(r.peaks_many([])) == 0


# ------------------------------------------------------------------------------------------------ through the aligner
def _piece():
    rng = np.random.default_rng(21)
    on = np.sort(rng.random(60) * 11.0)
    return arr([(o, o + 0.15 + float(rng.random()) * 0.6, int(rng.integers(36, 97)), int(rng.integers(50, 120))) for o in on])


def _mapped(notes, fn):
    out = notes.copy()
    out["onset"], out["offset"] = fn(notes["onset"]), fn(notes["offset"])
    return out


def _wpd(results):
    from etude_amd.evaluation import wpd_many
    return [float(d["wpd_score"]) for d in wpd_many(results)]


def test_features_of_device_audio_against_the_restatements():
    import torch
    from etude_amd.aligner import align_features_many
    from etude_amd.alignfeat import default_align_features
    piece = _piece()
    r, feats = _renderer(), default_align_features("cuda")
    x_dev = r.render(piece)
    x64, _ = rn.render_np(piece, SR)
    origin = r.render(_mapped(piece, lambda t: 1.1 * t + 0.5))
    f_dev, f_np, f_org = feats.features_many([x_dev, torch.from_numpy(x64.astype(np.float32)), origin])
    cells = float((f_dev[0] != f_np[0]).float().mean())
    w_dev, w_np = _wpd(align_features_many([(f_dev, f_org), (f_np, f_org)]))
    _keep("aligner/device_vs_restatement", wpd_device=w_dev, wpd_restatement=w_np, difference=abs(w_dev - w_np), differing_chroma_cells=cells)
    assert abs(w_dev - w_np) <= 1.0 / 50.0                                  # one feature frame: a warping path is not defined below that


def test_wpd_tells_a_linear_map_from_a_wobbling_one():
    from etude_amd.aligner import align_notes_many
    piece = _piece()
    r = _renderer()
    lin = lambda t: 1.1 * t + 0.5                                            # noqa: E731
    wob = lambda t: 1.1 * t + 0.5 + 0.3 * np.sin(2.0 * np.pi * t / 6.0)     # noqa: E731  (monotone: the slope stays above 1.1 - 0.1 pi)
    o_lin, o_wob = r.render_many([_mapped(piece, lin), _mapped(piece, wob)])
    from etude_amd.alignfeat import default_align_features
    f_lin = default_align_features("cuda").features(o_lin)
    res = align_notes_many([(piece, f_lin), (piece, o_wob)], renderer=r)   # an origin as features and one as samples
    w_lin, w_wob = _wpd(res)
    _keep("aligner/linear_vs_wobble", wpd_linear=w_lin, wpd_wobble=w_wob, wobble_std=0.3 / math.sqrt(2.0))
    assert w_lin < w_wob


def test_evaluate_many_scores_covers_that_exist_as_notes_only(tmp_path):
    from etude_amd.extractor import save_wav
    from etude_amd.rhythm import evaluate_many
    from etude_amd.tokenizer import TinyREMITokenizer
    piece = _piece()
    r = _renderer()
    d = tmp_path / "song"
    d.mkdir()
    origin = r.render(_mapped(piece, lambda t: 1.05 * t + 0.25))
    save_wav(d / "origin.wav", origin, SR, peak=float(r.peaks_many([origin])[0]))
    (d / "a.json").write_text(json.dumps([dict(onset=float(n["onset"]), offset=float(n["offset"]), pitch=int(n["pitch"]), velocity=int(n["velocity"])) for n in piece]))
    TinyREMITokenizer.note_to_midi(piece, d / "b.mid")
    meta = [{"dir_name": "song"}]
    before = evaluate_many(tmp_path, meta, ["a", "b", "c"])
    assert [row["version"] for row in before] == ["a", "b"] and all("wpd_score" not in row and "rgc_score" in row for row in before)
    rows = evaluate_many(tmp_path, meta, ["a", "b", "c"], renderer=r)
    assert [row["version"] for row in rows] == ["a", "b"]
    for row, old in zip(rows, before):
        assert np.isfinite(row["wpd_score"]) and row["wpd_score"] >= 0 and {k: v for k, v in row.items() if k != "wpd_score"} == old
    _keep("aligner/evaluate_many", wpd_json=float(rows[0]["wpd_score"]), wpd_mid=float(rows[1]["wpd_score"]))
    save_wav(d / "origin.wav", origin, 16000)
    with pytest.raises(ValueError, match="22050"):
        evaluate_many(tmp_path, meta, ["a"], renderer=r)
