"""fp64 numpy restatement of the DTW alignment contract: what csrc/dtw.hip computes, stated once more for the tests.

Sequence 1 is the cover, sequence 2 the origin.  A side is (quantized chroma [12][N] >= 0, DLNCO [12][N]).  Nothing here is fast; the recursion runs over
anti-diagonals (the cells of one are independent), with the same operations per cell as a plain triple loop (tests/test_dtw_cpu.py holds that loop).
"""
from __future__ import annotations

import numpy as np

STEPS = ((1, 0), (0, 1), (1, 1))
W_FINAL = (1.5, 1.5, 2.0)
W_SHIFT = (1.0, 1.0, 1.0)
ALPHA = 0.5
NORM_THR = 1e-3
CENS_WIN, CENS_DEC = 201, 50


def normalize_cols(x, thr=NORM_THR, dtype=np.float64):
    """every column divided by its L2 norm; a column whose norm is below thr becomes the constant unit vector"""
    x = np.asarray(x, dtype)
    nrm = np.sqrt((x * x).sum(axis=0, dtype=dtype))
    out = np.full_like(x, dtype(1.0) / np.sqrt(dtype(x.shape[0])))
    ok = nrm >= thr
    out[:, ok] = x[:, ok] / nrm[ok]
    return out


def shift_rows(f, s):
    """shift s of sequence 2: row k reads row (k - s) mod 12"""
    return np.roll(f, s, axis=0)


def cost_matrix(cover, origin, shift=0, alpha=ALPHA, dtype=np.float64):
    """C[i, j] = alpha (2 - <c1_i, c2_j>) + (1 - alpha) ||o1_i - o2_j||_2, in `dtype` throughout (fp32: the formula as a plain numpy user would write it)"""
    c1, c2 = normalize_cols(cover[0], dtype=dtype), shift_rows(normalize_cols(origin[0], dtype=dtype), shift)
    o1, o2 = np.asarray(cover[1], dtype), shift_rows(np.asarray(origin[1], dtype), shift)
    dot = c1.T @ c2
    diff = o1.T[:, None, :] - o2.T[None, :, :]
    dist = np.sqrt((diff * diff).sum(axis=2, dtype=dtype))
    return (dtype(alpha) * (dtype(2) - dot) + dtype(1 - alpha) * dist).astype(dtype)


def recursion(C, w=W_FINAL):
    """D[0,0] = C[0,0]; D[i,j] = min_k (D[i - di_k, j - dj_k] + w_k C[i,j]) over the predecessors that exist, ties to the lowest k.  C is taken as given (any float
    type) and widened to fp64.  -> (D [N1][N2] fp64, step index per cell uint8)"""
    C = np.asarray(C).astype(np.float64)
    N1, N2 = C.shape
    D = np.full((N1 + 1, N2 + 1), np.inf)          # D[i + 1][j + 1]; row / column 0 stand for "does not exist"
    K = np.zeros((N1, N2), np.uint8)
    for d in range(N1 + N2 - 1):
        i = np.arange(max(0, d - N2 + 1), min(N1 - 1, d) + 1)
        j = d - i
        c = C[i, j]
        best = D[i, j + 1] + w[0] * c              # (1, 0): from (i - 1, j)
        k = np.zeros(len(i), np.uint8)
        a1 = D[i + 1, j] + w[1] * c                # (0, 1): from (i, j - 1)
        m = a1 < best
        best = np.where(m, a1, best); k[m] = 1
        a2 = D[i, j] + w[2] * c                    # (1, 1)
        m = a2 < best
        best = np.where(m, a2, best); k[m] = 2
        if d == 0:
            best = c.copy()
        D[i + 1, j + 1] = best
        K[i, j] = k
    return D[1:, 1:], K


def backtrack(K):
    """the path from (0, 0) to (N1 - 1, N2 - 1) over the stored step index -> int64 [2][L], increasing"""
    i, j = K.shape[0] - 1, K.shape[1] - 1
    pts = [(i, j)]
    while i > 0 or j > 0:
        di, dj = STEPS[K[i, j]]
        i, j = i - di, j - dj
        pts.append((i, j))
    return np.array(pts[::-1], np.int64).T


def strictly_monotonic(path):
    """THE rule (one place): the first and the last point always stay; an interior point k stays when both of its coordinates are above those of point k - 1 of the
    unfiltered path; if the last point is then not above the kept point before it in both coordinates, that point -- when it is an interior one -- goes."""
    path = np.asarray(path, np.int64)
    L = path.shape[1]
    if L == 1:
        return path.copy()
    keep = [k for k in range(1, L - 1) if path[0, k] > path[0, k - 1] and path[1, k] > path[1, k - 1]]
    if keep and not (path[0, keep[-1]] < path[0, -1] and path[1, keep[-1]] < path[1, -1]):
        keep.pop()
    return path[:, [0] + keep + [L - 1]]


def path_total(C, path, w=W_FINAL):
    """the total of an (unfiltered) step path under a cost matrix; a strictly monotonic path is expanded with `expand` first"""
    C = np.asarray(C, np.float64)
    tot = C[path[0, 0], path[1, 0]]
    for k in range(1, path.shape[1]):
        step = (path[0, k] - path[0, k - 1], path[1, k] - path[1, k - 1])
        tot += w[STEPS.index(tuple(int(x) for x in step))] * C[path[0, k], path[1, k]]
    return tot


def cens(chroma, win=CENS_WIN, dec=CENS_DEC, dtype=np.float64):
    """quantized chroma -> CENS: every pitch row smoothed with a symmetric Hann window of `win` points scaled to sum 1 ("same" length, zeros outside), every dec-th frame
    from 0, columns normalised"""
    x = np.asarray(chroma, np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / (win - 1)) if win > 1 else np.ones(1)
    w = w / w.sum()
    h = (win - 1) // 2
    xp = np.pad(x, ((0, 0), (h, h)))
    sm = np.stack([np.correlate(xp[p], w, mode="valid") for p in range(x.shape[0])])
    return normalize_cols(sm[:, ::dec], dtype=np.float64).astype(dtype)


def shift_totals(cover_chroma, origin_chroma):
    """D[-1,-1] of the CENS DTW (cost 1 - <a, b>, weights (1, 1, 1)) for every shift of the origin"""
    a, b = cens(cover_chroma), cens(origin_chroma)
    return np.array([recursion(1.0 - a.T @ shift_rows(b, s), W_SHIFT)[0][-1, -1] for s in range(12)])


def optimal_shift(cover_chroma, origin_chroma):
    return int(np.argmin(shift_totals(cover_chroma, origin_chroma)))      # (argmin: the first minimum)


def pitch_shift_of(opt):
    ps = (-opt) % 12
    return ps - 12 if ps > 6 else ps


def align(cover, origin, C=None):
    """the whole contract for one pair -> the result dict plus "opt_shift", "total" and the unfiltered "raw_path".  C: a cost matrix to use in place of the fp64 one
    (the device's own, for the bitwise tests)"""
    opt = optimal_shift(cover[0], origin[0])
    if C is None:
        C = cost_matrix(cover, origin, opt)
    D, K = recursion(C, W_FINAL)
    raw = backtrack(K)
    return {"wp": strictly_monotonic(raw), "pitch_shift": pitch_shift_of(opt), "num_frames_cover": C.shape[0], "num_frames_origin": C.shape[1],
            "opt_shift": opt, "total": float(D[-1, -1]), "raw_path": raw}


# ---- fixtures shared by the CPU and the GPU tests

def chord_song(rng, n_frames, seg=(20, 60)):
    """piecewise-constant chords: quantized chroma [12][n] with values 0..4 and the segment boundaries"""
    chroma = np.zeros((12, n_frames), np.float32)
    bounds, t = [], 0
    while t < n_frames:
        ln = int(rng.integers(seg[0], seg[1]))
        root = int(rng.integers(0, 12))
        for iv, v in ((0, 4), (4, 3), (7, 3), (int(rng.integers(9, 12)), 1)):
            chroma[(root + iv) % 12, t:t + ln] = v
        bounds.append(t)
        t += ln
    return chroma, bounds


def onset_peaks(n_frames, onsets, pitches, decay=0.75, length=10):
    """sparse decaying peaks: a DLNCO-like [12][n]"""
    o = np.zeros((12, n_frames), np.float32)
    for t, p in zip(onsets, pitches):
        for k in range(length):
            if 0 <= t + k < n_frames:
                o[p, t + k] = max(o[p, t + k], decay ** k)
    return o


def planted_warp_fixture(seed=20240611, n_origin=400, transpose=3, noise=0.15):
    """An origin of piecewise-constant chords and a cover that is a piecewise +-20 % tempo warp of it, transposed up by `transpose` semitones, plus noise.
    -> (cover feats, origin feats, warp: for every cover frame the origin frame it was taken from (float), transpose)"""
    rng = np.random.default_rng(seed)
    chroma_o, bounds = chord_song(rng, n_origin)
    onsets = sorted(set(bounds + [int(x) for x in rng.integers(0, n_origin, n_origin // 12)]))
    pitches = [int(np.argmax(chroma_o[:, t])) if rng.random() < 0.7 else int(rng.integers(0, 12)) for t in onsets]
    dl_o = onset_peaks(n_origin, onsets, pitches)
    # the warp: segments of the origin played at a rate in 0.8 .. 1.2
    warp, pos = [], 0.0
    while pos < n_origin - 1:
        rate = float(rng.uniform(0.8, 1.2))
        for _ in range(int(rng.integers(40, 90))):
            if pos >= n_origin - 1:
                break
            warp.append(pos)
            pos += rate
    warp.append(float(n_origin - 1))
    warp = np.array(warp)
    src = np.clip(np.round(warp).astype(int), 0, n_origin - 1)
    chroma_c = np.roll(chroma_o[:, src], transpose, axis=0)
    chroma_c = np.clip(np.round(chroma_c + noise * 4 * rng.random(chroma_c.shape) * (rng.random(chroma_c.shape) < 0.3)), 0, 4).astype(np.float32)
    on_c = [int(np.argmin(np.abs(warp - t))) for t in onsets]
    dl_c = onset_peaks(len(warp), on_c, [(p + transpose) % 12 for p in pitches])
    dl_c = (dl_c + noise * 0.2 * rng.random(dl_c.shape)).astype(np.float32)
    return (chroma_c, dl_c), (chroma_o, dl_o), warp, transpose


def random_pair(rng, N1, N2, zero_cols=True):
    """small random features with a few silent chroma columns (the constant-vector branch)"""
    def side(n):
        c = rng.integers(0, 5, (12, n)).astype(np.float32)
        if zero_cols and n > 3:
            c[:, rng.integers(0, n, max(1, n // 9))] = 0
        o = (rng.random((12, n)) * (rng.random((12, n)) < 0.3)).astype(np.float32)
        return c, o
    return side(N1), side(N2)
