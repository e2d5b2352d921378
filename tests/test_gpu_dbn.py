"""DBN beat / downbeat tracking on the MI355X (csrc/dbn.hip) against the fp64 numpy restatement (tests/dbn_np.py): the Viterbi kernel bit for bit on supplied
densities, the trackers on fixtures that tests/test_dbn_cpu.py proves robust to an ulp in the densities, batch invariance, the BeatDetector surface and the workspace.

Kernel exactness uses the restatement's dense [S][S] recursion where S^2 T <= 2e9 and its block-sparse recursion beyond (the dense step costs 7 M operations per
frame at the 4-beat bar); tests/test_dbn_cpu.py holds the two bitwise equal."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dbn_fixtures as fx  # noqa: E402
import dbn_np  # noqa: E402

from etude_amd import dbn, synth  # noqa: E402

pytestmark = pytest.mark.gpu
FPS = fx.FPS


@pytest.fixture(scope="module")
def engine():
    return dbn.DBNEngine(FPS, 70.0, 250.0, 0.2, [3, 4])


@pytest.fixture(scope="module")
def engine0():
    return dbn.DBNEngine(FPS, 70.0, 250.0, 0.0, [3, 4])


def _densities(seed, T, K, kind):
    rng = np.random.default_rng(seed)
    d = np.log(rng.random((T, K)))
    if kind == "some_ninf":
        d[rng.random((T, K)) < 0.15] = -math.inf
    elif kind == "all_ninf":
        d[:] = -math.inf
    return d


@pytest.mark.parametrize("T", [1, 2, 9, 37, 1000, 7752])
@pytest.mark.parametrize("hmm", [0, 1, 2])
def test_viterbi_kernel_is_bitwise_the_restatement(engine, hmm, T):
    h = fx.hmms()[hmm]
    kinds = ["finite", "some_ninf"] + (["all_ninf"] if T in (9, 37) else [])
    for kind in kinds:
        d = _densities(1000 * hmm + T, T, h.K, kind)
        path, lp = engine.debug_viterbi(hmm, d)
        ref_path, ref_lp = dbn_np.viterbi(h, d, dense=h.S * h.S * T <= 2e9)
        assert lp == ref_lp, (hmm, T, kind, lp, ref_lp)
        assert np.array_equal(path, ref_path), (hmm, T, kind)
        if kind == "all_ninf":
            assert lp == -math.inf


def _track(eng, names):
    acts = [fx.fixtures()[n][0] for n in names]
    return eng.track_arrays(acts, dbn.IN_ACTIVATIONS)


@pytest.mark.parametrize("name", list(fx.fixtures()))
def test_trackers_match_the_restatement(engine, engine0, name):
    act, cfg, planted, per_bar = fx.fixtures()[name]
    eng = engine if cfg.threshold else engine0
    beats, rows, choice = _track(eng, [name])[0]
    rb, rr, rc = fx.restated(name)
    assert np.array_equal(beats, rb), name
    assert np.array_equal(rows, rr.reshape(-1, 2)), name
    assert choice == rc, name
    if per_bar is not None:
        assert cfg.beats_per_bar[choice] == per_bar, name          # 3/4 against 4/4 material
    if planted is not None:
        assert len(beats) == len(planted) and np.abs(beats - planted[:, 0]).max() <= 2


def test_madmom_style_processors(engine):
    act = fx.fixtures()["steady_3_4"][0]
    bt = dbn.DBNBeatTracker(min_bpm=70.0, max_bpm=250.0, fps=FPS, threshold=0.2)
    dt = dbn.DBNDownBeatTracker(beats_per_bar=[3, 4], min_bpm=70.0, max_bpm=250.0, fps=FPS, threshold=0.2)
    rb, rr, _ = fx.restated("steady_3_4")
    t = bt(act[:, 0])
    assert t.dtype == np.float64 and t.shape == (len(rb),) and np.array_equal(t, rb / FPS)
    r = dt(dbn_np.combined(act[:, 0], act[:, 1]))
    assert r.shape == (len(rr), 2) and np.array_equal(r[:, 0], rr[:, 0] / FPS) and np.array_equal(r[:, 1], rr[:, 1])
    assert bt(np.zeros(0, np.float32)).shape == (0,) and dt(np.zeros((0, 2), np.float32)).shape == (0, 2)
    many = bt.track_many([act[:, 0], fx.fixtures()["steady_4_4"][0][:, 0]])
    assert np.array_equal(many[0], t) and len(many[1]) == len(fx.restated("steady_4_4")[0])


def test_batch_invariance_bitwise(engine):
    names = list(fx.fixtures())
    songs = [fx.fixtures()[n][0] for n in names if fx.fixtures()[n][1].threshold]
    rng = np.random.default_rng(3)
    while len(songs) < 64:
        T = int(rng.integers(1, 900))
        a, _ = synth.beat_activations(100 + len(songs), T, ((None, float(rng.uniform(80, 200))),), int(rng.integers(3, 5)), jitter=0.003)
        songs.append(a)
    solo = [engine.track_arrays([s], dbn.IN_ACTIVATIONS)[0] for s in songs]
    order = list(rng.permutation(64))
    a = engine.track_arrays(songs, dbn.IN_ACTIVATIONS)
    b = engine.track_arrays([songs[i] for i in order], dbn.IN_ACTIVATIONS)
    for i in range(64):
        for name, got in (("batch", a[i]), ("reordered", b[order.index(i)])):
            assert np.array_equal(got[0], solo[i][0]) and np.array_equal(got[1], solo[i][1]) and got[2] == solo[i][2], (name, i)
    assert sum(len(s[0]) for s in solo) > 500


def test_logits_input_applies_the_sigmoid(engine):
    act = fx.fixtures()["steady_4_4"][0]
    logits = np.log(act.astype(np.float64) / (1.0 - act.astype(np.float64))).astype(np.float32)
    x = torch.from_numpy(logits).cuda()
    got = engine.track(x, [len(act)], dbn.IN_LOGITS)[0]
    want = engine.track(torch.sigmoid(x).contiguous(), [len(act)], dbn.IN_ACTIVATIONS)[0]
    rb, _, _ = fx.restated("steady_4_4")
    assert np.array_equal(got[0], rb) and np.array_equal(want[0], rb) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def det():
    from etude_amd import BeatDetector
    return BeatDetector(state_dict=synth.beat_state_dict(7), tracker="native")


def _restated_detect(det, feat):
    beat, down = det.activations(feat)
    c = det.config
    return dbn_np.detect(beat, down, dbn_np.TrackerCfg(fps=det.fps, min_bpm=c.min_bpm, max_bpm=c.max_bpm, threshold=c.threshold, beats_per_bar=tuple(c.beats_per_bar)), fx.hmms())


def test_detector_native(tmp_path, det):
    from etude_amd import TinyREMITokenizer, structuralize_many
    feats = [synth.beat_features(31, 700), synth.beat_features(32, 1), synth.beat_features(33, 1300)]
    want = [_restated_detect(det, f) for f in feats]
    p = tmp_path / "song.npy"
    np.save(p, feats[0])
    out = tmp_path / "sub" / "beat_pred.json"
    res = det.detect(p, out, cleanup_input=False)
    assert p.exists() and res == want[0] and json.loads(out.read_text()) == res
    det.detect(p)
    assert not p.exists()                                            # cleanup_input defaults to True, as in the reference
    np.save(p, feats[2])
    outs = [tmp_path / "a.json", None, tmp_path / "c" / "c.json"]
    many = det.detect_many([feats[0], feats[1], p], outs)
    assert many == want and p.exists()
    assert json.loads(outs[0].read_text()) == want[0] and json.loads(outs[2].read_text()) == want[2]
    tempo = structuralize_many(det, feats)
    assert len(tempo) == 3
    for td in tempo:
        TinyREMITokenizer.from_tempo_data(td)
    print("[measured] beats per song:", [len(w["beat_pred"]) for w in want], "regions:", [len(t) for t in tempo])


def test_structuralize_planted_song(det, monkeypatch):
    """planted 4/4 activations through detect_many's tracking + BeatAnalyzer -> a tempo.json the tokenizer takes, with the planted tempo"""
    from etude_amd import TinyREMITokenizer, structuralize_many
    act, planted = synth.beat_activations(41, 3000, ((None, 120.0),), 4, jitter=0.002)
    lg = torch.from_numpy(np.log(act.astype(np.float64) / (1.0 - act.astype(np.float64))).astype(np.float32)).cuda()
    monkeypatch.setattr(det, "_songs_to_device", lambda songs: (None, [len(act)]))
    monkeypatch.setattr(det, "_run", lambda feat, Ts, want_tempo=True: (lg, None))
    tempo = structuralize_many(det, [None])[0]
    assert len(tempo) >= 1 and tempo[0]["time_sig"] == 4 and abs(tempo[0]["bpm"] - 120.0) < 1.0
    tk = TinyREMITokenizer.from_tempo_data(tempo)
    assert tk is not None


def test_default_tracker_is_still_madmom():
    from etude_amd import BeatDetector
    d = BeatDetector(state_dict=synth.beat_state_dict(7))
    assert d.tracker == "madmom" and d._dbn is None


def test_workspace_bound():
    cfg = dbn.make_cfg(FPS, 70.0, 250.0, 0.2, (3, 4))
    for i, beats in enumerate((1, 3, 4)):
        n = dbn.workspace_bytes(cfg, 7752, i)
        print(f"[measured] workspace HMM {i}: {n} bytes")
        assert n <= 7752 * (beats * 28 * 2 + 64) + (1 << 20)


def test_madmom_cross_check(engine):
    """documents the parity where madmom is installed (unpinned: madmom takes its logarithms in float32)"""
    madmom_beats = pytest.importorskip("madmom.features.beats")
    proc = madmom_beats.DBNBeatTrackingProcessor(min_bpm=70.0, max_bpm=250.0, fps=FPS, threshold=0.2)
    for name in ("steady_4_4", "tempo_change", "steady_3_4"):
        act = fx.fixtures()[name][0]
        assert np.allclose(proc(act[:, 0]), fx.restated(name)[0] / FPS), name
