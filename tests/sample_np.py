"""Plain-numpy restatement of the decoder's sampler (`wave_sample`, etude_amd/csrc/dec_kernels.hip; the reference's
sampling branch etude_decoder.py:321-331).  No device, no torch.

The draw is a pure function of (logit row, 1 / temperature, top_p, seed, per-slot key, draw counter):

    u = (mix64(mix64(seed ^ mix64(key)) + ctr) >> 40) / 2^24            (mix64 = the splitmix64 finaliser)
    p = softmax(logits * inv_temp); descending order, lower index first on ties
    K = V, or with 0 < top_p < 1 the kept prefix: token k+1 is removed iff cum[k] > top_p (the first token always stays)
    S = sum of the K kept terms, target = u * S, token = first rank k with target < cum[k], else rank K-1

`draw32` does this in float32 exactly as the kernel orders it; `draw_set` does it in float64 and returns every token that
can come out when each cumulative sum and the target are off by up to `delta`.  A draw is DECISIVE when that set has one
element: the device then has to return exactly it.

delta
-----
What separates the kernel's fp32 numbers from the float64 ones of the same row (V <= 256 entries, eps = 2^-24):

* each probability: expf and the division, a few eps relative; the contraction of `lg * inv_temp - mx` into one fma moves
  the exponent by at most |t| eps (<= 16 eps for |t| <= 16).  Summed over a prefix (probabilities add up to 1): <= ~20 eps;
* the normaliser: a sum of V terms, relative error < V eps -- common to every probability, so it moves a cumulative sum by
  < V eps against top_p and cancels between the target u * S and the interval edges;
* a cumulative sum below 1 built by k <= V fp32 additions: each rounds by <= eps / 2, together <= V eps / 2; the
  product u * S rounds once more.

So |cum32[k] - cum64[k]| <= (V / 2 + V + 20) eps against top_p and the target-to-edge distance is off by at most
2 (V / 2 + 20) eps = (V + 40) eps.  Both stay below

    delta(V) = (V + 8) * 2^-22 = (4 V + 32) eps        (3.9e-5 at V = 154, 6.3e-5 at V = 256)

for every V >= 3 (V = 1 has one outcome; at V = 2 the bound holds for |t| <= 14).  The bound is validated on the CPU alone
(tests/test_sample_np_cpu.py: float32 draws under two summation orders never leave a singleton set); it is not tuned
on the device.  The order of two tokens can differ between fp32 and float64 only when their SCALED logits -- formed by the
same fp32 multiply on both sides -- differ by less than 2^-20: exp is monotone and the normaliser is common, so only a tie
within a few ulp of exp's result reorders; exactly equal scaled logits tie on both sides and the lower index comes first.
"""
import numpy as np

M64 = (1 << 64) - 1
SWAP_GAP = 2.0 ** -20


def delta_for(V: int) -> float:
    return (V + 8) * 2.0 ** -22


def mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u24(seed: int, key: int, ctr: int) -> int:
    """the 24 random bits of one draw"""
    return mix64((mix64((seed & M64) ^ mix64(key & M64)) + (ctr & 0xFFFFFFFF)) & M64) >> 40


def _mix64_np(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def u24_np(seed, keys, ctrs):
    """u24 over broadcastable uint64 arrays (wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        s, k, c = np.asarray(seed, np.uint64), np.asarray(keys, np.uint64), np.asarray(ctrs, np.uint64)
        return _mix64_np(_mix64_np(s ^ _mix64_np(k)) + c) >> np.uint64(40)


def _sum32(e, order):
    """fp32 sum of e: 'seq' = one running sum; 'wave' = the kernel's 64 strided partial sums, then the xor butterfly 32 .. 1"""
    if order == "seq":
        return np.cumsum(e, dtype=np.float32)[-1]
    part = np.zeros(64, np.float32)
    for v0 in range(0, e.size, 64):
        c = e[v0:v0 + 64]
        part[:c.size] += c
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ o]
    return part[0]


class Row32:
    """the float32 path of one (row, inv_temp, top_p): sorted ids, cumulative sums, kept count"""

    def __init__(self, logits, inv_temp, top_p, order="wave"):
        lg = np.asarray(logits, np.float32)
        V = lg.size
        with np.errstate(over="ignore", invalid="ignore"):
            t = lg * np.float32(inv_temp)
            e = np.exp(t - t.max()).astype(np.float32)
            p = e / _sum32(e, order)
        self.p = p
        self.si = np.lexsort((np.arange(V), -p))                 # descending, lower index first on ties
        self.cum = np.cumsum(p[self.si], dtype=np.float32)       # sequential fp32 running sum
        tp = np.float32(top_p)
        K = V
        if 0.0 < tp < 1.0:
            over = np.nonzero(self.cum[:V - 1] > tp)[0]
            K = int(over[0]) + 1 if over.size else V
        self.K = K

    def pick(self, u24_bits):
        """token(s) for 24-bit draws (scalar or array)"""
        u = np.asarray(u24_bits).astype(np.float32) * np.float32(2.0 ** -24)
        target = u * self.cum[self.K - 1]
        k = np.minimum(np.searchsorted(self.cum[:self.K], target, side="right"), self.K - 1)   # first k with target < cum[k]
        return self.si[k]


def draw32(logits_f32, inv_temp, top_p, seed, key, ctr, order="wave"):
    return int(Row32(logits_f32, inv_temp, top_p, order).pick(u24(seed, key, ctr)))


class Row64:
    """the float64 path of one (row, inv_temp, top_p), with the slack `delta`"""

    def __init__(self, logits, inv_temp, top_p, delta, scaled64=None):
        lg = np.asarray(logits, np.float32)
        V = lg.size
        with np.errstate(over="ignore", invalid="ignore"):
            t = (lg * np.float32(inv_temp)).astype(np.float64)   # the fp32 product both sides form
        if scaled64 is not None:                                 # (CPU tests: scaled logits given in float64 directly)
            t = np.asarray(scaled64, np.float64)
        fin = np.isfinite(t)
        if not fin.any() or (t == np.inf).any() or np.isnan(t).any():
            raise ValueError("the row needs a finite logit and no +inf / NaN")
        e = np.where(fin, np.exp(np.where(fin, t, 0.0) - t[fin].max()), 0.0)
        p = e / e.sum()
        si = np.lexsort((np.arange(V), -t))                      # -inf entries (p = 0) last, in index order
        ts, ps = t[si], p[si]
        cum = np.cumsum(ps)
        tp = float(np.float32(top_p))
        K = K_lo = K_hi = V
        if 0.0 < tp < 1.0:
            def kept(bound):
                over = np.nonzero(cum[:V - 1] > bound)[0]
                return int(over[0]) + 1 if over.size else V
            K, K_lo, K_hi = kept(tp), kept(tp - delta), kept(tp + delta)
        # runs of rank-neighbours whose scaled logits differ by less than 2^-20 but are not equal: their order is not pinned
        with np.errstate(invalid="ignore"):
            gap = ts[:-1] - ts[1:]
        loose = (gap < SWAP_GAP) & (gap > 0)
        grp = np.concatenate([[0], np.cumsum(~(loose | (gap == 0)))]) if V > 1 else np.zeros(1, np.int64)
        has_loose = np.zeros(int(grp[-1]) + 1, bool)
        if V > 1:
            np.logical_or.at(has_loose, grp[:-1][loose], True)
        self.V, self.p, self.si, self.ps, self.cum, self.delta = V, p, si, ps, cum, delta
        self.K, self.K_lo, self.K_hi, self.grp, self.has_loose = K, K_lo, K_hi, grp, has_loose

    def support(self):
        """token ids the exact float64 filter keeps"""
        return self.si[:self.K]

    def probs(self):
        """the exact float64 distribution after the filter, [V]"""
        out = np.zeros(self.V)
        keep = self.si[:self.K]
        out[keep] = self.p[keep] / self.cum[self.K - 1]
        return out

    def support_slack(self):
        """every token that may survive the cut within the slack (exactly-zero probabilities excluded)"""
        ranks = self._widen(set(range(self.K_hi)))
        return {int(self.si[r]) for r in ranks if self.ps[r] > 0}

    def _widen(self, ranks):
        out = set(ranks)
        for r in ranks:
            g = self.grp[r]
            if self.has_loose[g]:
                out.update(np.nonzero(self.grp == g)[0].tolist())
        return out

    def pick_set(self, u24_bits):
        u = int(u24_bits) * 2.0 ** -24
        d, cum = self.delta, self.cum
        ranks = set()
        for K in range(self.K_lo, self.K_hi + 1):
            target = u * cum[K - 1]
            # rank k can be the first with target < cum[k] iff target < cum[k] + d and (k == 0 or target >= cum[k - 1] - d)
            lo = int(np.searchsorted(cum[:K], target - d, side="right"))         # first k with cum[k] > target - d
            hi = int(np.searchsorted(cum[:K], target + d, side="right"))         # last k with cum[k - 1] <= target + d
            ranks.update(range(min(lo, K - 1), min(hi, K - 1) + 1))
        ranks = self._widen(ranks)
        return {int(self.si[r]) for r in ranks if self.ps[r] > 0}


def draw_set(logits_f32, inv_temp, top_p, seed, key, ctr, delta):
    return Row64(logits_f32, inv_temp, top_p, delta).pick_set(u24(seed, key, ctr))
