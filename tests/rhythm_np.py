"""fp64 numpy restatement of the rhythm engine's contract: Rhythmic Grid Consistency and IOI Pattern Entropy of one cover, from its sorted, unique onsets.

Written from the contract and from the libraries it names (numpy's reductions, scikit-learn's KMeans with k-means++ seeding and Lloyd's iteration), not from the device
code: every sum is spelled out in the order the contract fixes, one python float at a time, so that the device can be held to it bit for bit where the contract says so.
"""
from __future__ import annotations

import math

import numpy as np

RGC_OK, RGC_FEW_ONSETS, RGC_FEW_IOIS, RGC_FEW_UNIQUE, RGC_NO_TAU = 0, 1, 2, 3, 4
IPE_OK, IPE_FEW_ONSETS, IPE_EMPTY, IPE_NO_SYMBOLS = 0, 1, 2, 3
RGC_ERRORS = {RGC_FEW_ONSETS: "Not enough onsets for IOI calculation.", RGC_FEW_IOIS: "Not enough IOIs to analyze.",
              RGC_FEW_UNIQUE: "Not enough unique IOIs to determine a grid.", RGC_NO_TAU: "Could not infer a valid rhythmic grid period (tau)."}
IPE_ERRORS = {IPE_FEW_ONSETS: "Not enough onsets for IOI calculation.", IPE_EMPTY: "Could not extract a valid IOI sequence after processing.",
              IPE_NO_SYMBOLS: "Could not quantize IOI sequence into symbols."}
N_RANDOM = 29      # 1 for the first centre + 7 further centres x (2 + int(log 8)) local trials


def random_table() -> np.ndarray:
    """the only random numbers KMeans(random_state=42) with one k-means++ start draws: data-independent"""
    return np.random.RandomState(42).random_sample(N_RANDOM)


def np_sum(a) -> float:
    """numpy's add.reduce over a contiguous fp64 vector, restated: 0 + pairwise(a).  Below 8 elements sequential; up to 128 eight accumulators over whole groups of 8,
    combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remainder one by one; above 128 split at n // 2 rounded down to a multiple of 8."""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + float(v)
        return res
    if n <= 128:
        r = [float(a[j]) for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + float(a[i + j])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + float(a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return np_sum(a[:n2]) + np_sum(a[n2:])


def _rint(v: float) -> float:
    return float(np.rint(v))      # half to even


def rgc(onsets, top_k: int = 8, precision_digits: int = 4):
    """-> (status, rgc_score, inferred_tau); score and tau are nan unless status is RGC_OK"""
    t = np.asarray(onsets, np.float64)
    nan = float("nan")
    if t.size < 2:
        return RGC_FEW_ONSETS, nan, nan
    ioi = t[1:] - t[:-1]
    if ioi.size < top_k:
        return RGC_FEW_IOIS, nan, nan
    scale = float(10.0 ** precision_digits)
    order, count = [], {}
    for v in ioi:
        q = _rint(float(v) * scale)
        if q not in count:
            count[q] = 0
            order.append(q)
        count[q] += 1
    if len(order) < 2:
        return RGC_FEW_UNIQUE, nan, nan
    rank = sorted(range(len(order)), key=lambda i: (-count[order[i]], i))[:top_k]      # by count, ties by first occurrence
    top = [order[i] / scale for i in rank]
    best_tau, best = -1.0, float("inf")
    for tau in top:
        if tau < 0.01:
            continue
        dev = []
        for v in top:
            r = v / tau
            dev.append(abs(r - _rint(r)))
        score = np_sum(dev) / float(len(dev))
        if score < best:
            best, best_tau = score, tau
    if best_tau == -1.0:
        return RGC_NO_TAU, nan, nan
    return RGC_OK, best, best_tau


def log_ioi(onsets, min_ioi: float = 0.0625, max_ioi: float = 4.0):
    """the clipped log-IOIs, centred on their mean: (x centred, the tolerance scale var(x)); numpy's own log"""
    t = np.asarray(onsets, np.float64)
    x = np.log(np.clip(t[1:] - t[:-1], min_ioi, max_ioi))
    return centre(x)


def centre(x):
    n = len(x)
    mean = np_sum(x) / float(n)
    xc = np.asarray([float(v) - mean for v in x], np.float64)
    var = np_sum([float(v) * float(v) for v in xc]) / float(n)
    return xc, var


def _sqdist(c: float, x: float) -> float:
    """scikit-learn's euclidean_distances(squared=True) on one feature, in its order"""
    d = ((-2.0 * (c * x)) + c * c) + x * x
    return d if d > 0.0 else 0.0


def kmeans_pp(x, k: int, rnd):
    """k-means++ of scikit-learn on one feature with unit weights -> the indices of the k seeds"""
    n = len(x)
    x = [float(v) for v in x]
    trials = 2 + int(math.log(k))
    # the first centre: RandomState.choice(n, p = 1 / n): cdf = cumsum(p) / cdf[-1], searchsorted(u, side="right")
    p = 1.0 / float(n)
    cdf, s = [], 0.0
    for _ in range(n):
        s = s + p
        cdf.append(s)
    first = n - 1
    for i in range(n):
        if cdf[i] / cdf[-1] > rnd[0]:
            first = i
            break
    idx = [first]
    closest = [_sqdist(x[first], v) for v in x]
    pot = 0.0
    for v in closest:
        pot = pot + v
    r = 1
    for _ in range(1, k):
        vals = [float(rnd[r + t]) * pot for t in range(trials)]
        r += trials
        cand = [n - 1] * trials
        found = [False] * trials
        s = 0.0
        for i in range(n):      # the sequential cumulative sum; searchsorted(side="left"): the first i with cumsum[i] >= v, clipped to n - 1
            s = s + closest[i]
            for t in range(trials):
                if not found[t] and s >= vals[t]:
                    found[t], cand[t] = True, i
        best_t, best_pot, best_new = -1, 0.0, None
        for t in range(trials):
            c = x[cand[t]]
            new = [min(closest[i], _sqdist(c, x[i])) for i in range(n)]
            pt = 0.0
            for v in new:
                pt = pt + v
            if best_t < 0 or pt < best_pot:
                best_t, best_pot, best_new = t, pt, new
        pot, closest = best_pot, best_new
        idx.append(cand[best_t])
    return idx


def lloyd(x, centres, tol: float, max_iter: int = 300):
    """Lloyd's iteration of scikit-learn on one feature with unit weights -> (labels, centres, relocated, iterations)"""
    n, k = len(x), len(centres)
    x = [float(v) for v in x]
    c = [float(v) for v in centres]
    old_labels, labels, relocated, strict, it = [-1] * n, [-1] * n, False, False, 0

    def assign(c):
        cc = [v * v for v in c]
        out = []
        for v in x:
            best, bd = 0, (-2.0 * (v * c[0])) + cc[0]
            for j in range(1, k):
                d = (-2.0 * (v * c[j])) + cc[j]
                if d < bd:
                    best, bd = j, d
            out.append(best)
        return out

    for it in range(1, max_iter + 1):
        labels = assign(c)
        sums, w = [0.0] * k, [0.0] * k
        for i in range(n):
            sums[labels[i]] = sums[labels[i]] + x[i]
            w[labels[i]] = w[labels[i]] + 1.0
        empty = [j for j in range(k) if w[j] == 0.0]
        if empty:
            relocated = True
            dist = [(x[i] - c[labels[i]]) * (x[i] - c[labels[i]]) for i in range(n)]
            if max(dist) != 0.0:
                far = sorted(range(n), key=lambda i: (-dist[i], i))[:len(empty)]      # the project's rule: distance descending, then the lowest index
                for j, i in zip(empty, far):
                    o = labels[i]
                    sums[o] = sums[o] - x[i] * 1.0
                    sums[j] = x[i] * 1.0
                    w[j] = 1.0
                    w[o] = w[o] - 1.0
        heavy = max(range(k), key=lambda j: (w[j], -j))      # argmax: the first maximum
        new = list(sums)
        for j in range(k):      # in place, in ascending j, as _average_centers does
            if w[j] > 0.0:
                new[j] = new[j] * (1.0 / w[j])
            else:
                new[j] = new[heavy]
        shift = []
        for j in range(k):
            d = new[j] - c[j]
            s = math.sqrt(d * d)
            shift.append(s * s)
        c = new
        if labels == old_labels:
            strict = True
            break
        if np_sum(shift) <= tol:
            break
        old_labels = list(labels)
    if not strict:
        labels = assign(c)
    return np.asarray(labels, np.int32), np.asarray(c, np.float64), relocated, it


def entropy_bits(labels, n_gram: int = 8) -> float:
    """Shannon entropy, in bits, of the n-grams of the symbol sequence; the terms in order of first occurrence, summed as numpy sums a list"""
    m = len(labels) - n_gram + 1
    if m < 1:
        return 0.0
    count = {}
    for i in range(m):
        g = tuple(int(v) for v in labels[i:i + n_gram])
        count[g] = count.get(g, 0) + 1
    return -np_sum([(c / m) * float(np.log2(c / m)) for c in count.values()])


def ipe_from_logioi(xc, var, n_unique: int, n_gram: int = 8, n_clusters: int = 8, rnd=None):
    """the clustering and the entropy on given centred log-IOIs (the stage tests hand in the device's own) -> dict(status, score, labels, centres, relocated, k, iterations)"""
    k = min(n_clusters, n_unique)
    if k < 2:
        return dict(status=IPE_NO_SYMBOLS, score=float("nan"), labels=np.zeros(0, np.int32), centres=np.zeros(0), relocated=False, k=k, iterations=0)
    rnd = random_table() if rnd is None else rnd
    seeds = kmeans_pp(xc, k, rnd)
    labels, centres, relocated, it = lloyd(xc, [xc[i] for i in seeds], 1e-4 * var)
    return dict(status=IPE_OK, score=entropy_bits(labels, n_gram), labels=labels, centres=centres, relocated=relocated, k=k, iterations=it)


def ipe(onsets, n_gram: int = 8, n_clusters: int = 8, min_ioi: float = 0.0625, max_ioi: float = 4.0, rnd=None):
    t = np.asarray(onsets, np.float64)
    if t.size < 2:
        return dict(status=IPE_FEW_ONSETS, score=float("nan"), labels=np.zeros(0, np.int32), centres=np.zeros(0), relocated=False, k=0, iterations=0)
    x = np.log(np.clip(t[1:] - t[:-1], min_ioi, max_ioi))
    xc, var = centre(x)
    return ipe_from_logioi(xc, var, len(np.unique(x)), n_gram, n_clusters, rnd)


def same_partition(a, b) -> bool:
    """two labellings are the same up to the names of the clusters"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    fwd, bwd = {}, {}
    for u, v in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(u, v) != v or bwd.setdefault(v, u) != u:
            return False
    return True


def load_cases(path):
    """tests/golden/rhythm_cases.npz -> (the covers with the reference's outputs, the engine's limit the file was made for)"""
    g = np.load(path)
    off, lo = g["offsets"], g["label_offsets"]
    out = []
    for i, name in enumerate(g["names"].tolist()):
        out.append(dict(name=name, onsets=g["onsets"][off[i]:off[i + 1]], labels=g["labels"][lo[i]:lo[i + 1]], rgc_score=float(g["rgc_score"][i]),
                        rgc_tau=float(g["rgc_tau"][i]), rgc_error=str(g["rgc_error"][i]), ipe_score=float(g["ipe_score"][i]), ipe_error=str(g["ipe_error"][i])))
    return out, int(g["limit"])
