"""The BSS Eval contract of DESIGN.md 4p, restated in numpy: what ``etude_amd.BSSEval`` computes on the device, step by step.

This project's own contract, modelled on museval's ``bss_eval`` (v4, images, time-invariant filters); parity with museval is unpinned.  Two routes:

  * ``route="direct"``: the correlations as direct sums, a hand-written Cholesky and substitution.  Takes a dtype, so that it also runs in ``np.longdouble``
    (which LAPACK does not take): the truth of the GPU tests; in fp64 it is their yardstick.
  * ``route="fft"`` (fp64 only): the correlations by ``np.fft`` on the zero-padded signals and ``np.linalg.solve``, the way museval goes.

``variant`` names a deliberately wrong restatement (tests/test_bss_cpu.py shows that each is told apart):
  "lag_sign" (D built from the estimates shifted the other way), "no_tail" (the L - 1 tail dropped from the energies), "b_for_a" (B_j where A belongs),
  "per_window" (filters fitted on each window), "neighbours" (the neighbouring windows' samples allowed into the projection)."""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
NAMES = ("sdr", "isr", "sir", "sar", "sdr_plain")


def signals(a, dtype):
    """[J][C][N] -> [S][N] of dtype"""
    a = np.asarray(a)
    return a.reshape(a.shape[0] * a.shape[1], a.shape[2]).astype(dtype)


def correlations(ref, est, L, dtype=np.float64, route="direct", variant=None):
    """-> r [S][S][L], d [S][S][L]: r[p][q][l] = sum_n x_p[n] x_q[n + l], d[p][e][l] = sum_n x_p[n] y_e[n + l]"""
    x, y = signals(ref, dtype), signals(est, dtype)
    S, N = x.shape
    r, d = np.zeros((S, S, L), dtype), np.zeros((S, S, L), dtype)
    if route == "fft":
        n = 1 << int(np.ceil(np.log2(N + L)))
        X, Y = np.fft.rfft(x, n), np.fft.rfft(y, n)
        r[:] = np.fft.irfft(np.conj(X)[:, None, :] * X[None, :, :], n)[:, :, :L]
        d[:] = np.fft.irfft(np.conj(X)[:, None, :] * Y[None, :, :], n)[:, :, :L]
        return r, d
    for l in range(L):
        r[:, :, l] = x[:, :N - l] @ x[:, l:].T
        if variant == "lag_sign":
            d[:, :, l] = x[:, l:] @ y[:, :N - l].T
        else:
            d[:, :, l] = x[:, :N - l] @ y[:, l:].T
    return r, d


def gram(r, sel=None):
    """G [(p, k)][(q, m)] = r_pq[k - m] (k >= m) or r_qp[m - k], + eps on the diagonal; sel: the signals kept (a source's diagonal block)"""
    if sel is not None:
        r = r[np.ix_(sel, sel)]
    S, _, L = r.shape
    k = np.arange(L)
    lag = k[:, None] - k[None, :]
    R = r[:, :, np.abs(lag)]                                   # [p][q][k][m]
    G4 = np.where(lag >= 0, R, R.transpose(1, 0, 2, 3))
    G = G4.transpose(0, 2, 1, 3).reshape(S * L, S * L).copy()
    G[np.arange(S * L), np.arange(S * L)] += r.dtype.type(EPS)
    return G


def cholesky(G):
    """lower factor by hand, or None at a pivot that is <= 0 or not finite"""
    A = np.array(G, copy=True)
    n = A.shape[0]
    for c in range(n):
        piv = A[c, c]
        if not (piv > 0) or not np.isfinite(piv):
            return None
        A[c:, c] = A[c:, c] / np.sqrt(piv)
        A[c, c] = np.sqrt(piv)
        if c + 1 < n:
            A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c + 1:, c])
    return np.tril(A)


def chol_solve(Lm, D):
    n = Lm.shape[0]
    Y = np.array(D, copy=True)
    for i in range(n):
        Y[i] = (Y[i] - Lm[i, :i] @ Y[:i]) / Lm[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - Lm[i + 1:, i] @ Y[i + 1:]) / Lm[i, i]
    return Y


def spd_solve(G, D, route="direct"):
    """-> (X, status); status 1 = singular (X is NaN)"""
    if route == "fft":
        return np.linalg.solve(G, D), 0
    Lm = cholesky(G)
    if Lm is None:
        return np.full(D.shape, np.nan, G.dtype), 1
    return chol_solve(Lm, D), 0


def filters(r, d, J, C, route="direct"):
    """-> A [S L][S], B [J][C L][C], status"""
    S, _, L = r.shape
    A, st = spd_solve(gram(r), d.transpose(0, 2, 1).reshape(S * L, S), route)
    B = np.zeros((J, C * L, C), r.dtype)
    for j in range(J):
        sel = np.arange(j * C, (j + 1) * C)
        Dj = d[np.ix_(sel, sel)].transpose(0, 2, 1).reshape(C * L, C)
        B[j], s = spd_solve(gram(r, sel), Dj, route)
        st |= s
    return A, B, st


def num_windows(N, window, hop):
    return 1 if N < window else (N - window + hop) // hop


def window_bounds(N, window, hop):
    nw = num_windows(N, window, hop)
    return [(w * hop, N if w == nw - 1 else w * hop + window) for w in range(nw)]


def fir(F, xw):
    """F [P][L][ncol], xw [P][W] -> out [ncol][W + L - 1]: out[col][n] = sum_{p,k} F[p][k][col] xw_p[n - k]"""
    P, L, nc = F.shape
    W = xw.shape[1]
    out = np.zeros((W + L - 1, nc), xw.dtype)
    for p in range(P):
        for k in range(L):
            out[k:k + W] += np.outer(xw[p], F[p, k])
    return out.T


def project(A, B, xw, J, C):
    """one window's references xw [S][W] -> ps [J][C][W + L - 1], pa [J][C][W + L - 1]"""
    S = J * C
    L = A.shape[0] // S
    pa = fir(A.reshape(S, L, S), xw).reshape(J, C, -1)
    ps = np.stack([fir(B[j].reshape(C, L, C), xw[j * C:(j + 1) * C]) for j in range(J)])
    return ps, pa


def energies(ref, est, L, window, hop, dtype=np.float64, route="direct", variant=None):
    """-> dict(E [J][nwin][8], silent [nwin] bool, status, r, d, A, B)"""
    ref, est = np.asarray(ref), np.asarray(est)
    J, C, N = ref.shape
    x, y = signals(ref, dtype), signals(est, dtype)
    r, d = correlations(ref, est, L, dtype, route, variant)
    A, B, st = filters(r, d, J, C, route)
    bounds = window_bounds(N, window, hop)
    E = np.full((J, len(bounds), 8), np.nan, dtype)
    silent = np.zeros(len(bounds), bool)
    for w, (a, b) in enumerate(bounds):
        xw, yw = x[:, a:b], y[:, a:b]
        for sig in (xw, yw):
            if (np.abs(sig).reshape(J, -1).max(axis=1) == 0).any():
                silent[w] = True
        if silent[w] or st:
            continue
        Aw, Bw = A, B
        if variant == "per_window":
            rw, dw = correlations(xw.reshape(J, C, -1), yw.reshape(J, C, -1), L, dtype)
            Aw, Bw, _ = filters(rw, dw, J, C)
        if variant == "neighbours":
            lo = max(a - (L - 1), 0)
            ps, pa = project(Aw, Bw, x[:, lo:min(b + L - 1, N)], J, C)
            ps, pa = ps[:, :, a - lo:a - lo + (b - a) + L - 1], pa[:, :, a - lo:a - lo + (b - a) + L - 1]
            pad = (b - a) + L - 1 - ps.shape[2]
            ps, pa = np.pad(ps, ((0, 0), (0, 0), (0, pad))), np.pad(pa, ((0, 0), (0, 0), (0, pad)))
        else:
            ps, pa = project(Aw, Bw, xw, J, C)
        if variant == "b_for_a":
            pa = ps.copy()
        z = np.zeros((J, C, L - 1), dtype)
        s = np.concatenate([xw.reshape(J, C, -1), z], axis=2)
        ye = np.concatenate([yw.reshape(J, C, -1), z], axis=2)
        e_spat, e_interf, e_artif = ps - s, pa - ps, ye - pa
        terms = [s, e_spat + e_interf + e_artif, e_spat, s + e_spat, e_interf, s + e_spat + e_interf, e_artif]
        if variant == "no_tail":
            terms = [t[:, :, :b - a] for t in terms]
        for i, t in enumerate(terms):
            E[:, w, i] = (t * t).reshape(J, -1).sum(axis=1)
        diff = (xw - yw).reshape(J, -1)
        E[:, w, 7] = (diff * diff).sum(axis=1)
    return dict(E=E, silent=silent, status=int(st), r=r, d=d, A=A, B=B)


def db(num, den):
    """10 log10(num / den); den == 0 gives +inf, NaN stays NaN"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(num / den)
    out = np.where(den == 0, np.inf, out)
    return np.where(np.isnan(num) | np.isnan(den), np.nan, out)


def metrics(E):
    """E [J][nwin][8] -> dict of [J][nwin] float64"""
    E = np.asarray(E, np.float64)
    pairs = dict(sdr=(0, 1), isr=(0, 2), sir=(3, 4), sar=(5, 6), sdr_plain=(0, 7))
    return {k: db(E[..., a], E[..., b]) for k, (a, b) in pairs.items()}


def track_scores(m):
    """nanmedian over the windows, per source; NaN where every window is NaN"""
    out = {}
    for k, v in m.items():
        med = np.full(v.shape[0], np.nan)
        for j in range(v.shape[0]):
            ok = ~np.isnan(v[j])
            if ok.any():
                med[j] = np.median(v[j][ok])
        out[k] = med
    return out


def evaluate(ref, est, L, window, hop, dtype=np.float64, route="direct", variant=None):
    res = energies(ref, est, L, window, hop, dtype, route, variant)
    res["metrics"] = metrics(res["E"])
    res["scores"] = track_scores(res["metrics"])
    return res
