"""The exact DTW alignment on the MI355X (csrc/dtw.hip, etude_amd.aligner) against the fp64 restatement of DESIGN.md 4e (tests/dtw_np.py).

Bitwise: the restatement's recursion run on the device's OWN fp32 cost matrix (etd_dtw_debug_cost) must give the device's path and D[-1,-1] bit for bit -- D is fp64
and w_k * (double)C is exact, so each cell takes one rounding on either side.
Cost accuracy: E = max |C_dev - C_64| <= 4 E32 + 1e-6, E32 = the same error of the formula in fp32 numpy, computed in the test on the same input: 4 covers another
summation order, 1e-6 is 4 ulp at 2.0 (the largest value a cost term takes).
Optimality without the cost hook: the device's step path scored under C_64 is at most the optimum + 2 L w_max E_max, L = steps of the path, E_max = the bound above:
any path's total moves by at most L w_max E_max between two cost matrices that differ by E_max per cell."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dtw_np as R  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def _eng():
    from etude_amd.aligner import DTWEngine
    if "eng" not in _cache:
        _cache["eng"] = DTWEngine()
    return _cache["eng"]


def _limits():
    from etude_amd.aligner import limits
    return limits()


def _pair(N1, N2, seed=0):
    key = ("pair", N1, N2, seed)
    if key not in _cache:
        c, o = R.random_pair(np.random.default_rng(1000 * N1 + N2 + seed), N1, N2)
        for a in (*c, *o):
            a.setflags(write=False)
        _cache[key] = (c, o)
    return _cache[key]


def _planted():
    if "planted" not in _cache:
        cover, origin, warp, tr = R.planted_warp_fixture()
        _cache["planted"] = (cover, origin, warp, tr, R.align(cover, origin))
    return _cache["planted"]


def _bitwise(cover, origin):
    eng = _eng()
    got = eng.align_many([(cover, origin)], details=True)[0]
    Cd = eng.debug_cost(cover, origin, got["opt_shift"])
    assert Cd.dtype == np.float32 and Cd.shape == (cover[0].shape[1], origin[0].shape[1])
    D, K = R.recursion(Cd, R.W_FINAL)
    raw = R.backtrack(K)
    wp = R.strictly_monotonic(raw)
    assert got["wp"].dtype == np.int64 and got["wp"].shape == wp.shape and (got["wp"] == wp).all()
    assert got["total"] == D[-1, -1]                                              # bitwise: == on doubles
    assert eng.debug_total(cover, origin, got["opt_shift"]) == D[-1, -1]
    assert (eng.debug_path(cover, origin, got["opt_shift"]) == raw).all()
    assert got["num_frames_cover"] == Cd.shape[0] and got["num_frames_origin"] == Cd.shape[1]
    return got


@pytest.mark.parametrize("shape", [(1, 1), (1, 500), (500, 1), (2, 3), (63, 65), (64, 64), (65, 63)])
def test_bitwise_path_small_shapes(shape):
    _bitwise(*_pair(*shape))


@pytest.mark.parametrize("rows", [-1, 0, 1])
def test_bitwise_path_around_the_row_block(rows):
    B = _limits()["row_block"]
    _bitwise(*_pair(B + rows, 700))


def test_bitwise_path_three_row_blocks():
    _bitwise(*_pair(2 * _limits()["row_block"] + 1, 37))


def test_bitwise_path_every_residue_of_the_backpointer_word():
    W = _limits()["cells_per_word"]
    for k in range(W):
        _bitwise(*_pair(21, 2 * W + k))


def test_cost_accuracy():
    eng = _eng()
    worst = 0.0
    for shape, shift in (((63, 65), 0), ((200, 310), 5), ((65, 63), 11)):
        cover, origin = _pair(*shape)
        C64 = R.cost_matrix(cover, origin, shift)
        C32 = R.cost_matrix(cover, origin, shift, dtype=np.float32)
        Cd = eng.debug_cost(cover, origin, shift)
        E, E32 = np.abs(Cd.astype(np.float64) - C64).max(), np.abs(C32.astype(np.float64) - C64).max()
        print(f"cost {shape} shift {shift}: E = {E:.3e}  E32 = {E32:.3e}")
        assert E <= 4 * E32 + 1e-6
        worst = max(worst, E)
    assert worst > 0          # (fp32 was compared, not a copy of the fp64 matrix)


def test_optimality_without_the_cost_hook():
    eng = _eng()
    for shape in ((200, 310), (513, 140)):
        cover, origin = _pair(*shape)
        got = eng.align_many([(cover, origin)], details=True)[0]
        raw = eng.debug_path(cover, origin, got["opt_shift"])
        assert raw[:, 0].tolist() == [0, 0] and raw[:, -1].tolist() == [shape[0] - 1, shape[1] - 1]
        steps = np.diff(raw, axis=1)
        assert set(map(tuple, steps.T.tolist())) <= set(R.STEPS)
        assert (R.strictly_monotonic(raw) == got["wp"]).all()
        C64 = R.cost_matrix(cover, origin, got["opt_shift"])
        C32 = R.cost_matrix(cover, origin, got["opt_shift"], dtype=np.float32)
        E_max = 4 * np.abs(C32.astype(np.float64) - C64).max() + 1e-6
        D, _ = R.recursion(C64, R.W_FINAL)
        L = raw.shape[1]
        mine = R.path_total(C64, raw, R.W_FINAL)
        print(f"optimality {shape}: device path {mine!r}  optimum {D[-1, -1]!r}  allowance {2 * L * max(R.W_FINAL) * E_max:.3e}")
        assert mine <= D[-1, -1] + 2 * L * max(R.W_FINAL) * E_max
        assert abs(got["total"] - mine) <= L * max(R.W_FINAL) * E_max


def test_batch_invariance():
    eng = _eng()
    B = _limits()["row_block"]
    pairs = [_pair(1, 1), _pair(63, 65), _pair(B + 1, 140), _pair(2, 3), _pair(200, 310), _pair(65, 63)]
    alone = [eng.align_many([p], details=True)[0] for p in pairs]
    batch = eng.align_many(pairs, details=True)
    rev = eng.align_many(pairs[::-1], details=True)[::-1]
    for a, b, c in zip(alone, batch, rev):
        for other in (b, c):
            assert a["wp"].tobytes() == other["wp"].tobytes() and a["wp"].shape == other["wp"].shape
            assert a["total"] == other["total"] and a["opt_shift"] == other["opt_shift"] and a["pitch_shift"] == other["pitch_shift"]


def test_canaries_around_result_and_workspace():
    eng = _eng()
    pairs = [_pair(63, 65), _pair(_limits()["row_block"] + 1, 140), _pair(1, 500)]
    tensors = [eng._pair(i, c, o) for i, (c, o) in enumerate(pairs)]
    ws_bytes, res_ints, off = eng.workspace_bytes([t[0].shape[1] for t in tensors], [t[2].shape[1] for t in tensors])
    G = 4096
    ws = torch.full((ws_bytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((res_ints + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert ws.data_ptr() % 256 == 0 and res.data_ptr() % 8 == 0
    host, off2 = eng.align_raw(tensors, ws[G:G + ws_bytes], res[G:G + res_ints])
    torch.cuda.synchronize()
    assert bool((ws[:G] == 0xA5).all()) and bool((ws[G + ws_bytes:] == 0xA5).all())
    assert bool((res[:G] == 0x5A5A5A5A).all()) and bool((res[G + res_ints:] == 0x5A5A5A5A).all())
    assert (res[G:G + res_ints].cpu().numpy() == host).all()
    plain = eng.align_many(pairs)
    for p, r in enumerate(plain):
        L = int(host[off[p]])
        cap = min(r["num_frames_cover"], r["num_frames_origin"]) + 1
        assert L == r["wp"].shape[1] and (host[off[p] + 8: off[p] + 8 + L] == r["wp"][0]).all() and (host[off[p] + 8 + cap: off[p] + 8 + cap + L] == r["wp"][1]).all()
    # a buffer one element short is refused before anything is launched
    from etude_amd._lib import EtudeHipError
    with pytest.raises(EtudeHipError, match="workspace"):
        eng.align_raw(tensors, ws[G:G + ws_bytes - 256], res[G:G + res_ints])
    with pytest.raises(EtudeHipError, match="result"):
        eng.align_raw(tensors, ws[G:G + ws_bytes], res[G:G + res_ints - 1])


def test_transposition_matches_the_restatement():
    eng = _eng()
    fixtures = []
    for shift in (0, 1, 5, 6, 7, 11):
        rng = np.random.default_rng(100 + shift)                 # the fixtures of tests/test_dtw_cpu.py, which proves their gap
        origin, _ = R.chord_song(rng, 600, seg=(40, 120))
        cover = np.roll(origin, shift, axis=0)
        z1, z2 = np.zeros_like(cover), np.zeros_like(origin)
        fixtures.append(((cover, z1), (origin, z2), shift))
    cover, origin, _, tr, _ = _planted()
    fixtures.append((cover, origin, tr))
    got = eng.align_many([(c, o) for c, o, _ in fixtures], details=True)
    for (c, o, shift), g in zip(fixtures, got):
        assert g["opt_shift"] == shift == R.optimal_shift(c[0], o[0])
        assert g["pitch_shift"] == R.pitch_shift_of(shift) and -5 <= g["pitch_shift"] <= 6


def test_refusals():
    from etude_amd import _lib
    from etude_amd.aligner import align_features, make_cfg
    eng = _eng()
    cover, origin = _pair(63, 65)
    lim = _limits()
    big = np.zeros((12, lim["max_frames"] + 1), np.float32)
    with pytest.raises(_lib.EtudeHipError, match=str(lim["max_frames"] + 1)):
        eng.align_many([((big, big), origin)])
    with pytest.raises(ValueError, match="N >= 1"):
        eng.align_many([((np.zeros((12, 0), np.float32), np.zeros((12, 0), np.float32)), origin)])
    for bad in (np.nan, np.inf):
        c = cover[0].copy(); c[3, 7] = bad
        with pytest.raises(ValueError, match="non-finite"):
            eng.align_many([((c, cover[1]), origin)])
        o = torch.from_numpy(origin[1].copy()).cuda(); o[0, 0] = bad
        with pytest.raises(ValueError, match="non-finite"):
            align_features(cover, (origin[0], o))
    c = cover[0].copy(); c[0, 0] = -1
    with pytest.raises(ValueError, match="negative"):
        eng.align_many([((c, cover[1]), origin)])
    with pytest.raises(ValueError, match="differ in length"):
        eng.align_many([((cover[0], cover[1][:, :-1]), origin)])
    lib = _lib.lib()
    n0 = (C.c_int64 * 1)(0)
    n5 = (C.c_int64 * 1)(5)
    ptrs = (C.c_void_p * 4)(1, 1, 1, 1)
    assert lib.etd_dtw_align(eng.h, ptrs, 1, n0, n5, C.c_void_p(256), 1 << 20, C.c_void_p(256), 1 << 10, None, None) == -22
    cfg = make_cfg()
    cfg.struct_bytes += 8
    h = C.c_void_p()
    assert lib.etd_dtw_create(C.byref(cfg), C.byref(h)) == -22
    with pytest.raises(_lib.EtudeHipError, match="2\\^22"):
        eng.debug_cost(_pair(2100, 2000)[0], _pair(2100, 2000)[1], 0)


def test_chain_align_and_filter_many_matches_the_restatement_chain():
    from etude_amd.aligner import AudioAligner, align_and_filter_many, filter_and_weakly_align
    cover, origin, warp, tr, ref = _planted()
    rng = np.random.default_rng(5)
    n_o = origin[0].shape[1]
    downbeats = [float(x) for x in np.arange(0.3, n_o / 50 + 1.0, 0.8)]            # the last ones lie past the path's end
    t_on = rng.uniform(0, cover[0].shape[1] / 50, 60)
    notes = [{"pitch": int(rng.integers(21, 109)), "onset": float(t), "offset": float(t + 0.3), "velocity": 80} for t in t_on]
    small = _pair(63, 65)
    a = AudioAligner()
    outs, meta = align_and_filter_many(a, [(cover, origin), small], [downbeats, [0.1, 0.5, 0.9]], [notes, notes[:5]], 1e9, names=["song", "noise"])
    # the restatement chain: dtw_np.align on the cost matrix the device saw (its path is then the device's, bit for bit), through the host functions
    from etude_amd.aligner import default_engine
    eng = default_engine()
    chain_in = []
    for c, o in ((cover, origin), small):
        r = R.align(c, o, C=eng.debug_cost(c, o, R.optimal_shift(c[0], o[0])))
        chain_in.append({k: r[k] for k in ("wp", "pitch_shift", "num_frames_cover", "num_frames_origin")})
    assert chain_in[0]["pitch_shift"] == ref["pitch_shift"] == -3
    dev = a.align_features_many([(cover, origin), small])
    for d, r in zip(dev, chain_in):
        assert d.keys() == r.keys() and (d["wp"] == r["wp"]).all() and d["pitch_shift"] == r["pitch_shift"]
    assert np.abs(warp[dev[0]["wp"][0]] - dev[0]["wp"][1]).max() <= 2 * 2.76       # tests/test_dtw_cpu.py: D_MEASURED
    print("chain: device path equals the fp64-cost restatement's:", dev[0]["wp"].shape == ref["wp"].shape and bool((dev[0]["wp"] == ref["wp"]).all()))
    want_outs, want_meta = filter_and_weakly_align(chain_in, [downbeats, [0.1, 0.5, 0.9]], [notes, notes[:5]], 1e9, names=["song", "noise"])
    assert outs == want_outs and meta == want_meta and len(outs[0]) > 30 and [m["dir_name"] for m in meta] == ["song", "noise"]
    # the filter: a threshold below the song's WP-Std drops it
    outs2, meta2 = align_and_filter_many(a, [(cover, origin)], [downbeats], [notes], meta[0]["wp_std"] * 0.5)
    assert outs2 == [None] and meta2 == []
