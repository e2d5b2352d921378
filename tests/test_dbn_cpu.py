"""DBN trackers, CPU side: etd_dbn_describe (host only) against the numpy restatement (tests/dbn_np.py), the config refusals, the restatement's own consistency
(transition rows, dense against sparse recursion, planted beats) and the robustness of every fixture the GPU tests compare on."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dbn_fixtures as fx  # noqa: E402
import dbn_np  # noqa: E402

from etude_amd import _lib, dbn, synth  # noqa: E402

CONFIGS = {
    "default": dict(fps=44100 / 1024, min_bpm=70.0, max_bpm=250.0, beats_per_bar=(3, 4)),
    "madmom_defaults_fps100": dict(fps=100.0, min_bpm=55.0, max_bpm=215.0, beats_per_bar=(3, 4)),
    "log_spaced": dict(fps=100.0, min_bpm=55.0, max_bpm=215.0, beats_per_bar=(4,), num_tempi=20),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_describe_matches_restatement(name):
    c = CONFIGS[name]
    cfg = dbn.make_cfg(c["fps"], c["min_bpm"], c["max_bpm"], 0.2, c["beats_per_bar"], num_tempi=c.get("num_tempi"))
    for i, b in enumerate((None,) + tuple(c["beats_per_bar"])):
        h = dbn_np.make_hmm(c["fps"], c["min_bpm"], c["max_bpm"], b, num_tempi=c.get("num_tempi"))
        d = dbn.describe(cfg, i, tables=True)
        assert np.array_equal(d["intervals"], h.intervals), (name, i)
        assert d["n_states"] == h.S and d["num_beats"] == (b or 1)
        assert np.array_equal(d["pointers"], h.pointer)
        assert np.array_equal(d["logtrans"], h.lt), "log transitions must agree to the bit (libm exp / log, left-to-right row sums)"
    if name == "default":
        assert list(dbn.describe(cfg, 0)["intervals"]) == list(range(10, 38))
        assert [dbn.describe(cfg, i)["n_states"] for i in range(3)] == [658, 1974, 2632]
    if name == "log_spaced":
        assert 20 <= len(dbn.describe(cfg, 0)["intervals"]) < 82


@pytest.mark.parametrize("over,word", [(dict(min_bpm=250.0, max_bpm=70.0), "min_bpm"), (dict(min_bpm=120.0, max_bpm=120.0), "min_bpm"), (dict(fps=0.0), "fps"),
                                       (dict(fps=-3.0), "fps"), (dict(beats_per_bar=(3, 0)), "beats_per_bar"), (dict(beats_per_bar=(9,)), "beats_per_bar"),
                                       (dict(observation_lambda=1.0), "observation_lambda"), (dict(observation_lambda=0.5), "observation_lambda")])
def test_bad_configs_are_einval(over, word):
    kw = dict(fps=44100 / 1024, min_bpm=70.0, max_bpm=250.0, threshold=0.2, beats_per_bar=(3, 4))
    kw.update(over)
    cfg = dbn.make_cfg(**kw)
    lib = _lib.lib()
    n = C.c_int()
    assert lib.etd_dbn_describe(C.byref(cfg), 0, None, 0, C.byref(n), None, None, None, None) == -22
    assert word in lib.etd_last_error().decode()
    assert lib.etd_dbn_workspace_bytes(C.byref(cfg), 100, 0) == -22
    h = C.c_void_p()
    assert lib.etd_dbn_create(C.byref(cfg), C.byref(h)) == -22          # refused before any HIP call


def test_struct_size_and_capacity_refusals():
    lib = _lib.lib()
    cfg = dbn.make_cfg(44100 / 1024, 70.0, 250.0, 0.2, (3, 4))
    cfg.struct_bytes = 8
    assert lib.etd_dbn_describe(C.byref(cfg), 0, None, 0, None, None, None, None, None) == -22 and "etd_dbn_cfg" in lib.etd_last_error().decode()
    h = C.c_void_p()
    big = dbn.make_cfg(100.0, 55.0, 215.0, 0.0, (3, 4))                # madmom's defaults at 100 fps: 5 617 states per beat (described, not held by the device engine)
    assert dbn.describe(big, 1)["n_states"] == 16851
    assert lib.etd_dbn_create(C.byref(big), C.byref(h)) == -22 and "16851 states" in lib.etd_last_error().decode()
    many = dbn.make_cfg(1000.0, 55.0, 215.0, 0.0, ())                  # 812 intervals
    assert lib.etd_dbn_create(C.byref(many), C.byref(h)) == -22 and "intervals" in lib.etd_last_error().decode()
    ok = dbn.make_cfg(44100 / 1024, 70.0, 250.0, 0.2, (3, 4))
    assert lib.etd_dbn_describe(C.byref(ok), 3, None, 0, None, None, None, None, None) == -22


def test_workspace_has_no_T_by_S_array():
    cfg = dbn.make_cfg(44100 / 1024, 70.0, 250.0, 0.2, (3, 4))
    T = 7752
    for i, beats in enumerate((1, 3, 4)):
        assert dbn.workspace_bytes(cfg, T, i) <= T * (beats * 28 * 2 + 64) + (1 << 20)
    assert dbn.workspace_bytes(cfg, T) == sum(dbn.workspace_bytes(cfg, T, i) for i in range(3))


def test_transition_rows_sum_to_one():
    for h in fx.hmms()[:2]:
        p = np.exp(h.lt)
        assert np.abs(p.sum(axis=1) - 1.0).max() < 1e-12
        assert (np.diag(h.lt) > -math.inf).all() and (h.lt == -math.inf).any()          # the default lambda cuts the far tempo changes off
    A = fx.hmms()[1].dense()
    assert np.abs(np.exp(A).sum(axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("beats", [None, 3])
def test_dense_and_sparse_recursions_agree_bitwise(beats):
    h = dbn_np.make_hmm(30.0, 80.0, 200.0, beats)           # 9..22 frames per beat: small enough for the dense matrix
    rng = np.random.default_rng(5)
    for T, ninf in ((1, 0.0), (2, 0.0), (40, 0.0), (60, 0.2), (25, 1.0)):
        d = np.log(rng.random((T, h.K)))
        d[rng.random((T, h.K)) < ninf] = -math.inf
        pa, la = dbn_np.viterbi(h, d, dense=True)
        pb, lb = dbn_np.viterbi(h, d, dense=False)
        assert np.array_equal(pa, pb) and (la == lb), (beats, T, ninf)
        if ninf == 1.0:
            assert la == -math.inf


def test_planted_beats_are_recovered():
    for name in ("steady_4_4", "tempo_change", "steady_3_4"):
        act, cfg, planted, per_bar = fx.fixtures()[name]
        beats, rows, choice = fx.restated(name)
        assert len(beats) == len(planted), (name, len(beats), len(planted))
        assert np.abs(beats - planted[:, 0]).max() <= 2, name
        assert cfg.beats_per_bar[choice] == per_bar, name
        assert len(rows) == len(planted) and np.abs(rows[:, 0] - planted[:, 0]).max() <= 2
        assert np.array_equal(rows[:, 1], planted[:, 1]), name


def test_synth_activations_are_as_documented():
    act, planted = synth.beat_activations(3, 500, ((None, 120.0),), 4, jitter=0.0, noise=(0.01, 0.1))
    assert act.shape == (500, 2) and act.dtype == np.float32
    floor = np.ones(500, bool)
    for f, _ in planted:
        floor[f - 1:f + 2] = False
    assert act[floor, 0].min() >= 0.01 and act[floor, 0].max() <= 0.1
    assert (act[planted[:, 0], 0] >= 0.8).all()
    down = planted[planted[:, 1] == 1][:, 0]
    assert (act[down, 1] > 0.7).all() and act[floor, 1].max() <= 0.03 + 1e-6


@pytest.mark.parametrize("name", list(fx.fixtures()))
def test_fixture_is_robust_to_density_rounding(name):
    """the GPU tests compare on these fixtures: the restatement must give the same beats when every density moves by 1e-12 relative (up, down, random signs)"""
    b0, r0, c0 = fx.restated(name)
    for mode in (0, 1, 2):
        b, r, c = fx.restated(name, eps=1e-12, mode=mode)
        assert np.array_equal(b, b0) and np.array_equal(r, r0) and c == c0, (name, mode)
    expect_empty = name in ("all_below_threshold", "only_frame_0_above_threshold", "one_frame")
    assert (len(b0) == 0 and len(r0) == 0) == expect_empty, name
