"""BSS Eval on the device, stage by stage through the taps of include/etude_hip_debug.h.

The contract is this project's own.  Truth is the restatement (tests/bss_np.py) in ``np.longdouble``, the yardstick the same restatement in fp64;
``err = max|v - truth| / max|truth|`` per tensor, the device is held to 4 x the yardstick's error (two correct fp64 orders of summation differ by such factors, the
margin of DESIGN.md 4j / 4m / 4n), with a floor of 4 x 2^-53 where the yardstick is lucky.  The metrics are compared in dB, as differences of the dB values,
under the same rule: the floor is 4 x 2^-53 of the largest |dB| of the tensor, NOT 4 x 2^-53 dB -- an fp64 value near 8 dB has an ulp of 1.8e-15 dB, so a floor of
4.4e-16 dB would lie below the half-ulp any rounding of the host's 10 log10(num / den) can move a correct result by.  Every test prints
``ratio = device error / max(yardstick error, 2^-53)``; the largest per stage are in profiles/bss_device.json and DESIGN.md 4p.

Measured on an MI355X, largest ratios and the case each came from: correlations 0.61 (J1C1L16 N251, r), solve 0.58 (n = 1; 0.14 at n = 16 was the largest before
n < 16 was tried), filters 0.78 (J1C1L16 N251, A), projection 1.10 (J2C2L272 W512, ps of window 0; 1.07 for J2C1L16 h128 before), energies 1.25 (J2C1L16 h128, E0),
metrics 1.89 (J1C1L16 N251, isr).  The five cases beyond the first tile edges (J5C2L16, J8C2L16, J1C2L80, J2C2L272, J2C1L512) reach 0.34, 0.17, 1.10, 1.20 and 1.31 in
correlations, filters, projection, energies and metrics."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bss_np as B      # noqa: E402
from test_bss_cpu import GPU_CASES as CASES, GPU_IDS as IDS, gpu_track, make_track      # noqa: E402

pytestmark = pytest.mark.gpu

W = 256                 # the window of every test below that names no case
FLOOR = 2.0 ** -53
LD = np.longdouble
# CASES, (J, C, L, window, hop, N, coloured), live in tests/test_bss_cpu.py, which also shows without a GPU that none of them is silent or singular
PRODUCT = CASES[6]      # five stereo stems: the 32-column layout
assert PRODUCT[:2] == (5, 2)
_cache = {}


def reference(case):
    """the track, its truth and its yardstick, computed once"""
    if case not in _cache:
        _, _, L, window, hop, _, _ = case
        ref, est = gpu_track(case)
        _cache[case] = (ref, est, B.evaluate(ref, est, L, window, hop, dtype=LD), B.evaluate(ref, est, L, window, hop, dtype=np.float64))
    return _cache[case]


def engine(case, **kw):
    from etude_amd.bss import BSSEval, BSSEvalConfig
    eng = BSSEval(BSSEvalConfig(filters_len=case[2], window=case[3], hop=case[4], **kw))
    eng.guard = 64
    return eng


def held(name, dev, yard, truth):
    """the rule of the module docstring -> the ratio; asserts it"""
    truth, dev, yard = np.asarray(truth, LD), np.asarray(dev, LD), np.asarray(yard, LD)
    inf = np.isinf(truth)                 # (a metric over an energy that is exactly zero, e.g. SIR of a single source: the device must say so too)
    assert np.array_equal(dev[inf], truth[inf]), f"{name}: the device does not repeat the infinite entries"
    if inf.all():
        return 0.0
    truth, dev, yard = truth[~inf], dev[~inf], yard[~inf]
    scale = LD(1) if np.abs(truth).max() == 0 else np.abs(truth).max()      # (a tensor that is exactly zero, e.g. e_interf of a single source: absolute)
    e_dev = float(np.abs(dev - truth).max() / scale)
    e_yard = float(np.abs(yard - truth).max() / scale)
    ratio = e_dev / max(e_yard, FLOOR)
    print(f"BSS_RATIO {name}: device {e_dev:.3e} yardstick {e_yard:.3e} ratio {ratio:.3f}")
    assert e_dev <= 4 * max(e_yard, FLOOR), f"{name}: device {e_dev:.3e}, yardstick {e_yard:.3e}, ratio {ratio:.2f} > 4"
    return ratio


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than fp64 here: the truth of this module does not exist"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_correlations(case):
    ref, est, truth, yard = reference(case)
    eng = engine(case)
    r, d = eng.debug_corr(ref, est)
    assert eng.guards_intact()
    held("corr r", r, yard["r"], truth["r"])
    held("corr d", d, yard["d"], truth["d"])


@pytest.mark.parametrize("n,m", [(16, 5), (48, 5), (80, 5), (200, 5), (1, 5), (15, 5), (17, 5), (48, 16)], ids=["16", "48", "80", "200", "1", "15", "17", "48-m16"])
def test_solve_on_a_callers_matrix(n, m):
    """order 16: one panel; 48, 80: several panels and trailing updates; 200: a partial last panel; 1, 15: below one panel, the rest of it the identity's; 17: one row
    past a panel; m = 16: every right-hand side of the block is the caller's"""
    rng = np.random.default_rng(n if m == 5 else 1000 * m + n)
    M = rng.standard_normal((n, 2 * n))
    G = M @ M.T / (2 * n) + 0.05 * np.eye(n)
    D = rng.standard_normal((n, m))
    truth, st = B.spd_solve(G.astype(LD), D.astype(LD))
    yard, _ = B.spd_solve(G, D)
    eng = engine(CASES[0])
    x, status = eng.debug_solve(G, D)
    assert eng.guards_intact() and status == 0 and st == 0
    assert x.shape == (n, m)
    held(f"solve n={n} m={m}", x, yard, truth)


def test_indefinite_matrix_sets_the_status_and_the_next_call_works():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((48, 96))
    G = M @ M.T / 96 + 0.05 * np.eye(48)
    bad = G.copy()
    bad[20, 20] = -1.0
    D = rng.standard_normal((48, 2))
    eng = engine(CASES[0])
    _, status = eng.debug_solve(bad, D)
    assert status == 1
    x, status = eng.debug_solve(G, D)
    assert status == 0 and np.abs(G @ x - D).max() < 1e-10
    assert eng.guards_intact()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filters(case):
    ref, est, truth, yard = reference(case)
    eng = engine(case)
    A, Bf, status = eng.debug_filters(ref, est)
    assert eng.guards_intact() and status == 0
    held("filters A", A, yard["A"], truth["A"])
    held("filters B", Bf, yard["B"], truth["B"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_projection_with_a_callers_filters(case):
    """the first window and the last (the extended one where N = 4 W + 37), with the yardstick's fp64 filters as the caller's; at the 32-column layout of five stereo
    stems a middle window too (w = 2: the hop is half a window there, so its samples start inside window 1)"""
    J, C, L, window, hop, N, _ = case
    ref, est, _, yard = reference(case)
    eng = engine(case)
    A, Bf = yard["A"], yard["B"]
    bounds = B.window_bounds(N, window, hop)
    for w in sorted({0, len(bounds) - 1} | ({2} if case == PRODUCT else set())):
        a, b = bounds[w]
        ps, pa = eng.debug_project(ref, w, A, Bf)
        assert ps.shape == (J, C, b - a + L - 1)
        xw = B.signals(ref, LD)[:, a:b]
        tps, tpa = B.project(A.astype(LD), Bf.astype(LD), xw, J, C)
        yps, ypa = B.project(A, Bf, xw.astype(np.float64), J, C)
        held(f"project ps w={w}", ps, yps, tps)
        held(f"project pa w={w}", pa, ypa, tpa)
    assert eng.guards_intact()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energies_and_metrics(case):
    ref, est, truth, yard = reference(case)
    eng = engine(case)
    res = eng.evaluate_many([ref], [est])[0]
    assert eng.guards_intact()
    assert res["status"] == 0 and not res["silent"].any() and not truth["silent"].any()
    assert res["E"].shape == truth["E"].shape
    for i in range(8):
        held(f"energy E{i}", res["E"][..., i], yard["E"][..., i], truth["E"][..., i])
    with np.errstate(divide="ignore"):
        tm = {k: 10 * np.log10(truth["E"][..., a] / truth["E"][..., b]) for k, (a, b) in dict(sdr=(0, 1), isr=(0, 2), sir=(3, 4), sar=(5, 6), sdr_plain=(0, 7)).items()}
    for k in B.NAMES:
        held(f"metric {k}", res[k], yard["metrics"][k], tm[k])
        assert np.array_equal(res["scores"][k], B.track_scores({k: res[k]})[k])


def test_silent_windows_are_nan_and_their_neighbours_are_not():
    case = (2, 2, 32, W, 256, 4 * W + 37, 1)
    J, C, L, _, hop, N, colour = case
    ref, est = make_track(J, C, N, colour, seed=40)
    ref[1, :, W:2 * W] = 0           # a silent reference source in window 1
    est[0, :, 3 * W:] = 0            # a silent estimate source in window 3 (the extended one)
    ref[0, 0, 2 * W:3 * W] = 0       # one channel only: window 2 is not silent
    truth, yard = B.evaluate(ref, est, L, W, hop, dtype=LD), B.evaluate(ref, est, L, W, hop)
    eng = engine(case)
    res = eng.evaluate_many([ref], [est])[0]
    assert eng.guards_intact()
    assert res["silent"].tolist() == [False, True, False, True] == truth["silent"].tolist()
    assert np.isnan(res["E"][:, [1, 3]]).all()
    for k in B.NAMES:
        assert np.isnan(res[k][:, [1, 3]]).all() and np.isfinite(res[k][:, [0, 2]]).all()
    held("energies beside silent windows", res["E"][:, [0, 2]], yard["E"][:, [0, 2]], truth["E"][:, [0, 2]])


def test_a_track_is_bit_identical_alone_in_a_batch_under_a_tight_budget_and_across_runs():
    from etude_amd.bss import BSSEval, BSSEvalConfig
    L, hop = 32, 128
    shapes = [(2, 2, 4 * W + 37), (3, 1, W - 5), (1, 2, 7 * W + 11), (5, 2, 4 * W + 37)]      # (the last: NC = 32, the layout of five stereo stems)
    tracks = [make_track(J, C, N, i % 2, seed=50 + i) for i, (J, C, N) in enumerate(shapes)]
    eng = BSSEval(BSSEvalConfig(filters_len=L, window=W, hop=hop))
    alone = [eng.energies_many([r], [e])[0] for r, e in tracks]
    for order in ([0, 1, 2, 3], [2, 3, 0, 1], [3, 1, 2, 0]):
        batch = eng.energies_many([tracks[i][0] for i in order], [tracks[i][1] for i in order])
        for pos, i in enumerate(order):
            assert np.array_equal(batch[pos]["E"], alone[i]["E"], equal_nan=True) and np.array_equal(batch[pos]["silent"], alone[i]["silent"])
    again = eng.energies_many([t[0] for t in tracks], [t[1] for t in tracks])
    for i in range(len(shapes)):
        assert np.array_equal(again[i]["E"], alone[i]["E"], equal_nan=True)
        assert np.isfinite(alone[i]["E"]).all()
    for i, (J, C, N) in enumerate(shapes):      # a budget that just admits the track: one window's projections at a time
        tight = BSSEval(BSSEvalConfig(filters_len=L, window=W, hop=hop, workspace_bytes=eng.workspace_bytes(J, C, N)))
        assert np.array_equal(tight.energies_many([tracks[i][0]], [tracks[i][1]])[0]["E"], alone[i]["E"], equal_nan=True)
        tight.close()
    eng.close()


def test_a_track_over_the_budget_is_refused_with_its_bytes_and_the_engine_goes_on():
    from etude_amd.bss import BSSEval, BSSEvalConfig
    big, small = make_track(3, 2, 4 * W + 37, 0, seed=60), make_track(1, 1, 2 * W, 0, seed=61)
    probe = BSSEval(BSSEvalConfig(filters_len=32, window=W, hop=W))
    need_big, need_small = probe.workspace_bytes(3, 2, 4 * W + 37), probe.workspace_bytes(1, 1, 2 * W)
    assert need_small < need_big
    eng = BSSEval(BSSEvalConfig(filters_len=32, window=W, hop=W, workspace_bytes=need_big - 1))
    with pytest.raises(ValueError, match=str(need_big)):
        eng.evaluate_many([small[0], big[0]], [small[1], big[1]])
    res = eng.evaluate_many([small[0]], [small[1]])[0]
    assert np.array_equal(res["E"], probe.evaluate_many([small[0]], [small[1]])[0]["E"])
    with pytest.raises(ValueError, match="non-finite"):
        bad = small[1].copy()
        bad[0, 0, 5] = np.inf
        eng.evaluate_many([small[0]], [bad])


def test_evaluate_separator_equals_bsseval_on_the_separators_own_output():
    from etude_amd import BSSEval, BSSEvalConfig, SeparatorConfig, StemSeparator, evaluate_separator
    cfg = SeparatorConfig(instruments=("vocals", "other"), sample_rate=8000, n_fft=1024, hop=256, T=64, F=64, conv_n_filters=(3, 5, 8, 16, 24, 40))
    sep = StemSeparator(cfg, seed=1)
    rng = np.random.default_rng(70)
    tracks = []
    for N in (9000, 7001):
        stems = {n: (0.3 * rng.standard_normal((2, N))).astype(np.float32) for n in cfg.instruments}
        tracks.append((stems["vocals"] + stems["other"], stems))
    bss = BSSEval(BSSEvalConfig(filters_len=16, window=2048, hop=2048))
    out = evaluate_separator(sep, tracks, bss=bss)
    ests = sep.separate_many([t[0] for t in tracks])
    refs = [np.stack([t[1][n] for n in cfg.instruments]) for t in tracks]
    want = bss.evaluate_many(refs, ests)
    assert out["n_tracks"] == 2 and set(out["aggregate"]) == set(cfg.instruments)
    for got, w in zip(out["results"], want):
        assert np.array_equal(got["E"], w["E"], equal_nan=True) and np.isfinite(w["E"]).all()
    for t, w in zip(out["tracks"], want):
        for j, n in enumerate(cfg.instruments):
            assert t[n]["sdr"] == float(w["scores"]["sdr"][j])
    one = evaluate_separator(sep, tracks, bss=bss, instruments=["other"])
    assert np.array_equal(one["results"][0]["E"][0], bss.evaluate_many([refs[0][1:]], [ests[0][1:]])[0]["E"][0], equal_nan=True)
    with pytest.raises(ValueError, match="Hz"):
        evaluate_separator(sep, tracks, bss=bss, sample_rate=44100)
