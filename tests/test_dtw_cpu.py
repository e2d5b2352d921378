"""The fp64 restatement of the DTW contract (tests/dtw_np.py) against an independent triple loop, hand-written paths and planted answers; and the
library's host-only DTW entry points (sizes, limits, refusals that need no GPU)."""
import ctypes as C

import numpy as np
import pytest

import dtw_np as R
from etude_amd import _lib

# planted-warp fixture (dtw_np.planted_warp_fixture, seed 20240611): the restatement's path lies within D_MEASURED frames of the planted warp (measured when this
# test was written: 2.76); asserted with a factor 2 over it
D_MEASURED = 2.76


def triple_loop(C_, w):
    """the recursion, cell by cell: the independent statement dtw_np.recursion is held to"""
    N1, N2 = C_.shape
    D = np.zeros((N1, N2))
    K = np.zeros((N1, N2), np.uint8)
    for i in range(N1):
        for j in range(N2):
            if i == 0 and j == 0:
                D[0, 0] = C_[0, 0]
                continue
            best, bk = np.inf, 0
            for k, (di, dj) in enumerate(R.STEPS):
                pi, pj = i - di, j - dj
                if pi < 0 or pj < 0:
                    continue
                v = D[pi, pj] + w[k] * C_[i, j]
                if v < best:
                    best, bk = v, k
            D[i, j], K[i, j] = best, bk
    return D, K


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (2, 3), (12, 9), (9, 12), (5, 5)])
def test_recursion_matches_the_triple_loop(shape):
    rng = np.random.default_rng(sum(shape))
    for w in (R.W_FINAL, R.W_SHIFT):
        # integer-valued costs make ties frequent: the tie rule is exercised
        for C_ in (rng.random(shape), rng.integers(0, 3, shape).astype(np.float64)):
            D, K = R.recursion(C_, w)
            D2, K2 = triple_loop(C_, w)
            assert (D == D2).all()
            mask = np.ones(shape, bool); mask[0, 0] = False
            assert (K[mask] == K2[mask]).all()
            p = R.backtrack(K)
            assert p[:, 0].tolist() == [0, 0] and p[:, -1].tolist() == [shape[0] - 1, shape[1] - 1]
            assert abs(R.path_total(C_, p, w) - D[-1, -1]) <= 1e-12 * max(1.0, D[-1, -1])


def test_identical_sequences_give_the_diagonal_and_a_repetition_the_staircase():
    rng = np.random.default_rng(3)
    c = np.eye(12, dtype=np.float32)[:, rng.permutation(12)[:9]] * 4      # 9 distinct chroma columns
    o = np.zeros((12, 9), np.float32)
    C_ = R.cost_matrix((c, o), (c, o))
    p = R.backtrack(R.recursion(C_)[1])
    assert p.tolist() == [list(range(9)), list(range(9))]
    assert R.strictly_monotonic(p).tolist() == p.tolist()
    c2, o2 = np.repeat(c, 2, axis=1), np.repeat(o, 2, axis=1)              # the origin holds every frame twice
    p = R.backtrack(R.recursion(R.cost_matrix((c, o), (c2, o2)))[1])
    # (i, 2i) by a diagonal step (weight 2.0 on cost 0.5), then (i, 2i + 1) by a step along the origin: the staircase
    assert p.tolist() == [[i // 2 for i in range(18)], list(range(18))]
    assert R.strictly_monotonic(p).tolist() == [[0] + list(range(1, 8)) + [8], [0] + [2 * i for i in range(1, 8)] + [17]]


def test_strictly_monotonic_on_hand_written_paths():
    f = lambda rows: R.strictly_monotonic(np.array(rows)).tolist()
    assert f([[0], [0]]) == [[0], [0]]
    assert f([[0, 0, 0], [0, 1, 2]]) == [[0, 0], [0, 2]]                              # first and last always stay
    assert f([[0, 1, 2, 3], [0, 1, 2, 3]]) == [[0, 1, 2, 3], [0, 1, 2, 3]]
    assert f([[0, 1, 1, 2, 3], [0, 0, 1, 2, 3]]) == [[0, 2, 3], [0, 2, 3]]            # (1, 0) and (1, 1) each repeat a coordinate of their predecessor
    assert f([[0, 1, 2, 2, 2], [0, 1, 2, 3, 4]]) == [[0, 1, 2], [0, 1, 4]]            # (2, 2) is not below the last point (2, 4) in both coordinates: it goes
    assert f([[0, 1, 2, 3, 4], [0, 1, 2, 2, 2]]) == [[0, 1, 4], [0, 1, 2]]
    assert f([[0, 1, 1], [0, 1, 2]]) == [[0, 1], [0, 2]]
    out = np.array(f([[0, 0, 1, 2, 2, 3, 4, 4], [0, 1, 2, 2, 3, 4, 5, 6]]))
    assert (np.diff(out, axis=1) > 0).all()


@pytest.mark.parametrize("shift", range(12))
def test_transposition_rule_recovers_a_planted_shift(shift):
    rng = np.random.default_rng(100 + shift)
    origin, _ = R.chord_song(rng, 600, seg=(40, 120))
    cover = np.roll(origin, shift, axis=0)[:, ::1]
    tot = R.shift_totals(cover, origin)
    assert int(np.argmin(tot)) == shift == R.optimal_shift(cover, origin)
    ps = R.pitch_shift_of(shift)
    assert -5 <= ps <= 6 and (ps + shift) % 12 == 0
    best, second = np.sort(tot)[:2]
    assert second - best > 1e-6 * max(abs(second), 1e-300)      # the gap the GPU transposition test relies on


def test_planted_warp_is_recovered_within_the_recorded_distance():
    cover, origin, warp, tr = R.planted_warp_fixture()
    r = R.align(cover, origin)
    assert r["opt_shift"] == tr == 3 and r["pitch_shift"] == -3
    tot = np.sort(R.shift_totals(cover[0], origin[0]))
    assert tot[1] - tot[0] > 1e-6 * tot[1]
    wp = r["wp"]
    assert (np.diff(wp, axis=1) > 0).all() and wp[:, 0].tolist() == [0, 0] and wp[:, -1].tolist() == [cover[0].shape[1] - 1, origin[0].shape[1] - 1]
    dev = np.abs(warp[wp[0]] - wp[1]).max()
    print("planted warp: max distance", dev)
    assert dev <= 2 * D_MEASURED


def test_cens_smooths_decimates_and_normalises():
    x = np.zeros((12, 230), np.float32); x[3, :] = 2.0; x[7, 100:] = 1.0
    f = R.cens(x)
    assert f.shape == (12, 5)
    assert np.allclose((f * f).sum(axis=0), 1.0)
    assert f[7, 0] < f[7, 2] < f[7, 4] and abs(f[7, 2] / f[3, 2] - 0.25) < 0.01      # frame 100: half the window over the step
    assert np.allclose(R.cens(np.zeros((12, 60))), 1 / np.sqrt(12))


# ---- the library's host-only entry points

def _handle(**kw):
    from etude_amd.aligner import make_cfg
    cfg = make_cfg(**kw)
    h = C.c_void_p()
    rc = _lib.lib().etd_dtw_create(C.byref(cfg), C.byref(h))
    return rc, h, cfg


def test_create_refuses_bad_configs_and_mismatched_struct_bytes():
    lib = _lib.lib()
    rc, h, cfg = _handle()
    assert rc == 0
    lib.etd_dtw_destroy(h)
    cfg.struct_bytes -= 4
    assert lib.etd_dtw_create(C.byref(cfg), C.byref(h)) == -22 and b"etd_dtw_cfg" in lib.etd_last_error()
    for kw in (dict(cens_window=200), dict(cens_decimation=0), dict(alpha=1.5), dict(step_weights=(1.5, 0.0, 2.0)), dict(norm_threshold=float("nan"))):
        assert _handle(**kw)[0] == -22, kw


def test_workspace_bytes_follows_the_documented_formula_and_refuses_over_capacity():
    from etude_amd.aligner import limits
    lib = _lib.lib()
    lim = limits()
    assert lim["row_block"] >= 64 and lim["cells_per_word"] == 16 and lim["max_frames"] >= 1 << 15
    rc, h, _ = _handle()
    A = lambda x: (x + 255) // 256 * 256

    def ask(N1, N2):
        n = len(N1)
        r, off = C.c_longlong(), (C.c_int64 * n)()
        ws = lib.etd_dtw_workspace_bytes(h, n, (C.c_int64 * n)(*N1), (C.c_int64 * n)(*N2), C.byref(r), off)
        return ws, r.value, list(off)
    N1, N2 = [9000, 1, 513], [9000, 500, 37]
    ws, r, off = ask(N1, N2)
    want = A(3 * 160)
    for a, b in zip(N1, N2):
        M1, M2 = (a - 1) // 50 + 1, (b - 1) // 50 + 1
        want += A(96 * a) + A(96 * b) + A(48 * M1) + A(48 * M2) + A(8 * b) + 12 * A(8 * M2) + A(96) + A(4 * a * ((b + 15) // 16)) + A(8 * (min(a, b) + 1)) + A(8 * (a + b))
    assert ws == want
    assert r == sum(8 + 2 * (min(a, b) + 1) for a, b in zip(N1, N2)) and off == [0, 8 + 2 * 9001, 8 + 2 * 9001 + 8 + 4]
    assert 20e6 < ask([9000], [9000])[0] < 24e6                       # 2 bits per cell dominate: 20 MB for 9 000 x 9 000
    over = lim["max_frames"] + 1
    assert ask([over], [10])[0] == -22 and str(over).encode() in lib.etd_last_error()
    assert ask([10], [over])[0] == -22
    assert ask([0], [10])[0] == -22 and ask([10], [0])[0] == -22
    assert lib.etd_dtw_workspace_bytes(h, 0, None, None, None, None) == -22
    lib.etd_dtw_destroy(h)
