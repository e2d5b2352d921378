"""Every sampled token against an exact restatement of the sampler (tests/sample_np.py, itself pinned on the CPU by
tests/test_sample_np_cpu.py).  The draw is a pure function of (logit row, 1 / temperature, top_p, seed, per-slot key, draw
counter), so each device token is compared with `draw_set` on the DEVICE'S OWN logits of that draw: no model tolerance enters,
only the slack delta(V) = (V + 8) 2^-22 between fp32 and float64 cumulative sums that sample_np.py derives (3.9e-5 at V = 154,
6.3e-5 at V = 256).  A draw whose set is a singleton is decisive: the device must return that token.  Every test counts the
other draws, holds them to 5 % of its draws and prints `decisive n/N, mismatches 0`.

(a) the sampler alone (etd_debug_sample_rows: wave_sample, one wave per row): every strided-loop width, padded rows, hand-made
    edges, tie order, the top_p / temperature extremes, -inf logits, u = 1 - 2^-24;
(b) the first token of a bar (k_dargmax after prefill, counter 0) on the logits begin_bars left (etd_debug_decoder_bar_logits);
(c) the fused 16-bit step (k_dstep_head): key of the row's SLOT, counter = tokens the slot has produced, four rows per wave;
(d) k_dargmax inside a step (fp32 engines; 16-bit engines of 256-wide models);
(e) keys of slots that restart a bar while the others are mid-bar;  (f) sampling, then greedy on the same engine.

Non-decisive shares at these deltas, with the float32 restatement standing in for the device (the sampler-alone cases) and on the
oracle's logits (tests/test_sample_np_cpu.py): 0 .. 0.92 % on random rows (worst: V = 255), 1.50 % on the hand-made rows (three of them
sit on a cut by construction), 0.69 % at the top_p / temperature extremes, 0.37 % with -inf logits, 0.35 .. 1.41 % on oracle rows at V = 154.
"""
import numpy as np
import pytest
import torch

from etude_amd import _lib, synth
from tests import sample_np as sn

pytestmark = pytest.mark.gpu

SETTINGS = [(0.8, 0.9), (1.5, 0.6), (1.0, 1.0), (0.7, 0.3)]          # (temperature, top_p)
CAP = 0.05
# (key, counter) with u = (2^24 - 1) / 2^24 under seed U_MAX_SEED, found on the CPU:
#   for blk in range(64):
#       keys = np.arange(blk << 20, (blk + 1) << 20, dtype=np.uint64) + np.uint64(1 << 33)
#       hit = np.nonzero(sn.u24_np(U_MAX_SEED, keys, 7) == 0xFFFFFF)[0]       # first hit: blk 5
U_MAX_SEED, U_MAX_KEY, U_MAX_CTR = 20240229, 8595335736, 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


class Tally:
    """decisive / non-decisive / mismatching draws of one test"""

    def __init__(self):
        self.n = self.undecided = 0
        self.bad = []

    def judge(self, logits, toks, temperature, top_p, seed, keys, ctrs, what=""):
        """row i of `logits` drew toks[i] with (keys[i], ctrs[i]); rows given as one shared 1-D row are prepared once"""
        inv = np.float32(1.0) / np.float32(temperature)
        shared = sn.Row64(logits, inv, top_p, sn.delta_for(logits.size)) if logits.ndim == 1 else None
        for i, tok in enumerate(np.asarray(toks).tolist()):
            r = shared or sn.Row64(logits[i], inv, top_p, sn.delta_for(logits.shape[1]))
            s = r.pick_set(sn.u24(seed, int(keys[i]), int(ctrs[i])))
            self.n += 1
            if len(s) != 1:
                self.undecided += 1
                if tok not in s:                                  # even an undecided draw has to stay inside its set
                    self.bad.append((what, i, int(keys[i]), int(ctrs[i]), tok, sorted(s)))
            elif tok not in s:
                self.bad.append((what, i, int(keys[i]), int(ctrs[i]), tok, sorted(s)))
        return self

    def close(self, what):
        print(f"{what}: decisive {self.n - self.undecided}/{self.n}, mismatches {len(self.bad)} (non-decisive {100.0 * self.undecided / max(self.n, 1):.2f} %)")
        for b in self.bad[:10]:
            print("  mismatch (case, row, key, counter, device token, allowed):", b)
        assert not self.bad, self.bad[:10]
        assert self.undecided <= CAP * self.n, (self.undecided, self.n)


def _sample_rows(dev, logits, V, temperature, top_p, seed, keys, ctrs):
    """etd_debug_sample_rows on host rows [M, ld] (the first V columns are the logits)"""
    M, ld = logits.shape
    lg = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev)
    kd = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(ctrs, np.uint32).view(np.int32)).to(dev)
    out = torch.full((M,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().etd_debug_sample_rows(lg.data_ptr(), M, V, ld, temperature, top_p, seed, kd.data_ptr(), cd.data_ptr(), out.data_ptr(), st), "sample_rows")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _keys(rng, n):
    """distinct 64-bit keys: small ones, the scheduler's (job << 32) | bar form, and values with the high bits set"""
    k = rng.integers(1 << 32, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    k[::3] = rng.permutation(4 * n)[:k[::3].size].astype(np.uint64)
    k[1::3] = ((rng.permutation(4 * n)[:k[1::3].size].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | rng.integers(0, 64, k[1::3].size, dtype=np.uint64)
    assert np.unique(k).size == n
    return k


# ------------------------------------------------------------------------------------------------ (a) the sampler alone
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 154, 255, 256])
def test_sampler_alone_random_rows(dev, V):
    rng = np.random.default_rng(100 + V)
    M = 257
    t = Tally()
    for ld in (V, 257):
        rows = np.full((M, ld), np.nan, np.float32)              # the padding must never be read: a NaN there would poison max and sum
        rows[:, :V] = rng.normal(0.0, 2.5, (M, V)).astype(np.float32)
        for temperature, top_p in SETTINGS:
            keys, ctrs = _keys(rng, M), rng.integers(0, 1 << 32, M, dtype=np.uint64)
            ctrs[::2] = rng.integers(0, 512, ctrs[::2].size)
            seed = int(rng.integers(0, 1 << 63))
            toks = _sample_rows(dev, rows, V, temperature, top_p, seed, keys, ctrs)
            assert ((toks >= 0) & (toks < V)).all()
            t.judge(rows[:, :V], toks, temperature, top_p, seed, keys, ctrs, what=f"V={V} ld={ld} T={temperature} top_p={top_p}")
    t.close(f"sampler alone, V = {V}")


def _hand_rows():
    ln2, ninf = np.log(2.0), -np.inf
    return {
        "ties_across_cut": np.asarray([1.0, 3.0, 3.0, 3.0, 0.0, 3.0, -2.0], np.float32),
        "cum_equals_top_p": np.asarray([-2 * ln2, 0.0, -2 * ln2, -ln2], np.float32),           # ~ 1/8, 1/2, 1/8, 1/4
        "one_hot": np.asarray([-200.0, -200.0, 50.0, -200.0, -200.0], np.float32),
        "neg_inf": np.asarray([0.5, ninf, 1.5, ninf, -0.5, 0.25, ninf, ninf], np.float32),
        "neg_inf_but_one": np.asarray([ninf, ninf, 0.0, ninf], np.float32),
        "v1": np.asarray([0.3], np.float32),
        "v2": np.asarray([-0.2, 0.4], np.float32),
        "v2_tie": np.asarray([1.0, 1.0], np.float32),
        "all_equal_67": np.zeros(67, np.float32),                                               # ties across the 64-lane stride (67: no k / 67 equals a top_p)
    }


def test_sampler_alone_hand_made_rows_and_tie_order(dev):
    rng = np.random.default_rng(7)
    M = 128
    t = Tally()
    drawn = {}
    for name, row in _hand_rows().items():
        rows = np.tile(row, (M, 1))
        for temperature, top_p in SETTINGS + [(1.0, 0.3), (1.0, 0.5), (1.0, 0.75), (1.0, 0.4)]:
            keys, ctrs, seed = _keys(rng, M), rng.integers(0, 64, M, dtype=np.uint64), int(rng.integers(0, 1 << 63))
            toks = _sample_rows(dev, rows, row.size, temperature, top_p, seed, keys, ctrs)
            t.judge(row, toks, temperature, top_p, seed, keys, ctrs, what=f"{name} T={temperature} top_p={top_p}")
            drawn[(name, temperature, top_p)] = set(toks.tolist())
    # the ORDER among equal probabilities: ids 1, 2, 3, 5 hold 0.2386 each; the cut falls between two of them and the lower indices survive
    assert drawn[("ties_across_cut", 1.0, 0.3)] == {1, 2} and drawn[("ties_across_cut", 1.0, 0.5)] == {1, 2, 3}
    assert drawn[("v2_tie", 1.0, 0.4)] == {0} and drawn[("v2_tie", 1.0, 0.5)] == {0, 1}       # cum[0] = 0.5 is not > 0.5: the second stays
    assert drawn[("all_equal_67", 1.0, 0.5)] <= set(range(34)) and drawn[("all_equal_67", 1.0, 0.3)] <= set(range(21))     # 34/67 > 0.5: ranks 0 .. 33 stay; 21/67 > 0.3: 0 .. 20
    assert drawn[("one_hot", 1.0, 1.0)] == {2} and drawn[("neg_inf_but_one", 1.5, 0.6)] == {2} and drawn[("v1", 0.7, 0.3)] == {0}
    assert drawn[("cum_equals_top_p", 1.0, 0.75)] <= {1, 3, 0} and drawn[("cum_equals_top_p", 1.0, 0.4)] == {1}
    t.close("hand-made rows")


def test_sampler_alone_top_p_and_temperature_extremes(dev):
    rng = np.random.default_rng(8)
    M, V = 257, 154
    rows = rng.normal(0.0, 2.5, (M, V)).astype(np.float32)
    rows[::5, 100] = rows[::5].max(axis=1) + np.float32(0.5)     # a tied maximum at ids 20 and 100: argmax must take the lower index
    rows[::5, 20] = rows[::5, 100]
    keys, ctrs, seed = _keys(rng, M), rng.integers(0, 300, M, dtype=np.uint64), 99
    t = Tally()
    got = {tp: _sample_rows(dev, rows, V, 0.9, tp, seed, keys, ctrs) for tp in (-1.0, 0.0, 1e-6, 1.0, 2.0)}
    for tp in (-1.0, 0.0, 2.0):                                  # only 0 < top_p < 1 filters
        assert np.array_equal(got[tp], got[1.0]), tp
        t.judge(rows, got[tp], 0.9, tp, seed, keys, ctrs, what=f"top_p={tp}")
    t.judge(rows, got[1.0], 0.9, 1.0, seed, keys, ctrs, what="top_p=1")
    assert np.array_equal(got[1e-6], rows.argmax(axis=1)) and (got[1e-6][::5] == 20).all()      # np.argmax: first maximum
    t.judge(rows, got[1e-6], 0.9, 1e-6, seed, keys, ctrs, what="top_p=1e-6")
    # temperature 1e-3: scaled logits in the thousands, the softmax is one-hot (the maximum leads by >= 1, i.e. 1 000 after scaling) and nothing is NaN
    sharp = rows.copy()
    sharp[np.arange(M), rows.argmax(axis=1)] += 1.0
    for tp in (0.9, 1.0):
        toks = _sample_rows(dev, sharp, V, 1e-3, tp, seed, keys, ctrs)
        assert np.array_equal(toks, sharp.argmax(axis=1))
        t.judge(sharp, toks, 1e-3, tp, seed, keys, ctrs, what=f"T=1e-3 top_p={tp}")
    for tp in (0.9, 1.0):                                        # temperature 50: nearly flat
        toks = _sample_rows(dev, rows, V, 50.0, tp, seed, keys, ctrs)
        assert np.unique(toks).size > 60
        t.judge(rows, toks, 50.0, tp, seed, keys, ctrs, what=f"T=50 top_p={tp}")
    t.close("top_p / temperature extremes")


def test_sampler_alone_never_draws_a_probability_zero_token(dev):
    rng = np.random.default_rng(9)
    M, V = 4096, 154
    row = rng.normal(0.0, 1.0, V).astype(np.float32)
    dead = rng.permutation(V)[:80]
    row[dead] = -np.inf
    row[[0, V - 1]] = -np.inf                                    # first and last entry, and the whole tail of the order
    keys, ctrs = _keys(rng, M), rng.integers(0, 1 << 32, M, dtype=np.uint64)
    t = Tally()
    for temperature, top_p in ((1.0, 1.0), (2.0, 2.0), (0.8, 0.9)):
        toks = _sample_rows(dev, np.tile(row, (M, 1)), V, temperature, top_p, 5, keys, ctrs)
        assert np.isfinite(row[toks]).all(), "a token of probability 0 was drawn"
        assert np.unique(toks).size > 30
        t.judge(row, toks, temperature, top_p, 5, keys, ctrs, what=f"-inf T={temperature} top_p={top_p}")
    t.close("-inf logits")


def test_sampler_alone_largest_u_stays_inside_the_nucleus(dev):
    """u = (2^24 - 1) / 2^24 on a flat row of 256: target = u * S is the closest a draw gets to the end of the last interval -- the
    case the fall-back `tok = si[K - 1]` exists for.  (S and the running sum are the same additions, and u * S < S after rounding for
    every u <= 1 - 2^-24, so the last interval still catches it: rank 255.)"""
    assert sn.u24(U_MAX_SEED, U_MAX_KEY, U_MAX_CTR) == 0xFFFFFF
    V = 256
    rows = np.zeros((3, V), np.float32)
    rows[1] = 1.25
    rows[2, :200] = 0.5                                          # two plateaus: rank 255 is id 255 of the lower one
    keys, ctrs = np.full(3, U_MAX_KEY, np.uint64), np.full(3, U_MAX_CTR, np.uint64)
    t = Tally()
    for temperature, top_p in ((1.0, 1.0), (0.7, 1.0), (1.0, 2.0)):
        toks = _sample_rows(dev, rows, V, temperature, top_p, U_MAX_SEED, keys, ctrs)
        assert ((toks >= 0) & (toks < V)).all() and toks.tolist() == [255, 255, 255]
        t.judge(rows, toks, temperature, top_p, U_MAX_SEED, keys, ctrs, what="u max")
    toks = _sample_rows(dev, rows, V, 1.0, 0.5, U_MAX_SEED, keys, ctrs)          # with a cut: the last KEPT rank (128/256 = 0.5 is not > 0.5: ranks 0 .. 128)
    assert toks[:2].tolist() == [128, 128]
    t.judge(rows[2:], toks[2:], 1.0, 0.5, U_MAX_SEED, keys[2:], ctrs[2:], what="u max, top_p 0.5")    # (rows 0, 1: cum == top_p exactly, asserted above instead)
    t.close("largest u")


def test_sample_rows_refuses_bad_arguments(dev):
    x = torch.zeros(4, 300, device=dev)
    k = torch.zeros(4, dtype=torch.int64, device=dev); c = torch.zeros(4, dtype=torch.int32, device=dev); o = torch.zeros(4, dtype=torch.int32, device=dev)
    call = lambda V, ld, temp: _lib.lib().etd_debug_sample_rows(x.data_ptr(), 4, V, ld, temp, 0.9, 1, k.data_ptr(), c.data_ptr(), o.data_ptr(), None)     # noqa: E731
    assert call(257, 300, 1.0) != 0 and call(0, 300, 1.0) != 0 and call(16, 300, 0.0) != 0 and call(16, 300, -1.0) != 0 and call(16, 8, 1.0) != 0
    assert call(16, 300, 1.0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engines
def _decoder(precision, weights="bench", **kw):
    from etude_amd.decoder import EtudeDecoder, EtudeDecoderConfig
    sd = synth.decoder_state_dict_ctx(1) if weights == "ctx" else synth.decoder_state_dict(1, {})
    return EtudeDecoder(EtudeDecoderConfig(**synth.decoder_dims()), sd, "cuda", precision=precision, **kw)


def _prompts(rng, n, lo, hi):
    out = []
    for _ in range(n):
        T = int(rng.integers(lo, hi + 1))
        out.append((rng.integers(6, 154, T).astype(np.int32), rng.integers(1, 3, T).astype(np.int32), rng.integers(0, 3, (4, T)).astype(np.int32)))
    return out


def _set_sampling(dec, temperature, top_p, seed):
    _lib.check(_lib.lib().etd_decoder_set_sampling(dec._h, temperature, top_p, seed, dec._stream()), "set_sampling")


def _set_keys(dec, slots, keys):
    sl, k = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(keys, np.uint64)
    _lib.check(_lib.lib().etd_decoder_set_keys(dec._h, len(sl), sl.ctypes.data, k.ctypes.data), "set_keys")


def _begin(dec, prompts, tg, slots, limits):
    n = len(prompts)
    T = np.asarray([len(p[0]) for p in prompts], np.int32)
    ids = np.concatenate([p[0] for p in prompts]); cls = np.concatenate([p[1] for p in prompts])
    a4 = np.ascontiguousarray(np.concatenate([p[2] for p in prompts], axis=1))
    tgt = np.ascontiguousarray(np.tile(np.asarray(tg, np.int32), (n, 1)))
    eos = np.full(n, -1, np.int32); lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limits, np.int32), (n,)))
    sl = np.ascontiguousarray(slots, np.int32)
    _lib.check(_lib.lib().etd_decoder_begin_bars(dec._h, n, sl.ctypes.data, T.ctypes.data, ids.ctypes.data, cls.ctypes.data, a4.ctypes.data, tgt.ctypes.data,
                                                 eos.ctypes.data, lim.ctypes.data, dec._stream()), "begin_bars")


def _step(dec, slots, n_steps):
    sl = np.ascontiguousarray(slots, np.int32)
    _lib.check(_lib.lib().etd_decoder_step(dec._h, sl.ctypes.data, len(sl), n_steps, dec._stream()), "step")


def _read(dec, slots, cap):
    sl = np.ascontiguousarray(slots, np.int32)
    out = np.full((len(sl), cap), -7, np.int32); cnt = np.zeros(len(sl), np.int32)
    _lib.check(_lib.lib().etd_decoder_read_many(dec._h, len(sl), sl.ctypes.data, out.ctypes.data, cap, cnt.ctypes.data, dec._stream()), "read_many")
    return out, cnt


def _slot_list(rng, rows, identity, spare=3):
    return np.arange(rows) if identity else np.sort(rng.permutation(rows + spare)[:rows])


# ------------------------------------------------------------------------------------------------ (b) first token
@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_first_token_is_the_draw_with_counter_zero(dev, precision):
    rng = np.random.default_rng(31)
    dec = _decoder(precision, max_streams=40)
    n = 37
    prompts = _prompts(rng, n, 20, 60)
    t = Tally()
    for rep, (temperature, top_p) in enumerate(SETTINGS + SETTINGS):
        slots = np.sort(rng.permutation(40)[:n])
        keys, seed = _keys(rng, n), int(rng.integers(0, 1 << 63))
        _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, slots, keys)
        _begin(dec, prompts, (2, 1, 1, 1), slots, 4)
        lg = dec.debug_bar_logits(n)
        toks, cnt = _read(dec, slots, 4)
        assert (cnt == 1).all()
        t.judge(lg, toks[:, 0], temperature, top_p, seed, keys, np.zeros(n, np.uint64), what=f"rep {rep}")
    t.close(f"first token, {precision}")
    dec.close()


# ------------------------------------------------------------------------------------------------ (c) the fused 16-bit step
@pytest.mark.parametrize("rows,lo,hi,identity,k", [(1, 20, 60, True, 1), (3, 20, 60, False, 2), (33, 20, 60, False, 7), (33, 20, 60, True, 1), (54, 300, 380, True, 2),
                                                   (54, 300, 380, False, 7), (130, 20, 60, False, 1), (130, 20, 60, True, 7)])
def test_fused_step_draws_with_the_slot_key_and_the_slot_counter(dev, rows, lo, hi, identity, k):
    """toks[r][k] must be the draw from the k-th step's logits of row r with the key of the row's SLOT and counter k"""
    rng = np.random.default_rng(1000 * rows + k)
    spare = 3
    dec = _decoder("f16", max_streams=rows + spare, max_prefill_rows=(rows + spare) * (hi + 8))
    reps = max(2, -(-120 // rows))
    t = Tally()
    for rep in range(reps):
        prompts = _prompts(rng, rows, lo, hi)
        slots = _slot_list(rng, rows, identity, spare)
        key_of_slot = _keys(rng, rows + spare)[rng.permutation(rows + spare)]       # row index != slot != key
        temperature, top_p = SETTINGS[rep % 4]
        seed = int(rng.integers(0, 1 << 63))
        _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, np.arange(rows + spare), key_of_slot)
        _begin(dec, prompts, (2, 1, 1, 1), slots, k + 3)
        dec.debug_step_logits(True)
        _step(dec, slots, k)
        lg = dec.debug_step_logits(False, rows)
        toks, cnt = _read(dec, slots, k + 3)
        assert (cnt == k + 1).all()
        t.judge(lg, toks[:, k], temperature, top_p, seed, key_of_slot[slots], np.full(rows, k, np.uint64), what=f"rep {rep}")
    t.close(f"fused step, {rows} rows, {'identity' if identity else 'scattered'} slots, step {k}")
    dec.close()


def test_fused_step_rows_of_one_wave_share_a_key_and_some_are_done(dev):
    """Eleven rows with ONE key: a wave's four rows differ in their logits and in how far they have come.  Limits 1, 2, 3 finish rows
    0, 1, 2 of each wave early: a finished row emits nothing more and its count stays, and the rows still running draw with their own
    counter -- not with that of the wave's first row."""
    rng = np.random.default_rng(77)
    rows, k = 11, 3
    dec = _decoder("f16", max_streams=rows)
    slots = np.arange(rows)
    limits = np.asarray([1, 2, 3, 9, 9, 1, 9, 2, 3, 9, 9], np.int32)
    t = Tally()
    for rep in range(12):
        temperature, top_p = SETTINGS[rep % 4]
        seed, key = int(rng.integers(0, 1 << 63)), int(rng.integers(1 << 40, 1 << 63))
        _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, slots, np.full(rows, key, np.uint64))
        _begin(dec, _prompts(rng, rows, 20, 60), (2, 1, 1, 1), slots, limits)
        dec.debug_step_logits(True)
        _step(dec, slots, k)
        lg = dec.debug_step_logits(False, rows)
        toks, cnt = _read(dec, slots, 9)
        assert np.array_equal(cnt, np.minimum(limits, k + 1)), cnt
        live = np.nonzero(limits > k)[0]
        t.judge(lg[live], toks[live, k], temperature, top_p, seed, np.full(live.size, key, np.uint64), np.full(live.size, k, np.uint64), what=f"rep {rep}")
        first, _ = _read(dec, slots, 9)
        _step(dec, slots, 1)                                                           # one more step: the finished rows stay as they are
        again, cnt2 = _read(dec, slots, 9)
        done = np.nonzero(limits <= k)[0]
        assert np.array_equal(cnt2[done], limits[done]) and np.array_equal(again[done], first[done])
    t.close("one key per wave, finished rows")
    dec.close()


# ------------------------------------------------------------------------------------------------ (d) k_dargmax inside a step
def _small_decoder(precision, max_streams):
    from etude_amd.decoder import EtudeDecoder, EtudeDecoderConfig
    over = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, max_position_embeddings=128,
                context_num_past_xy_pairs=2, attribute_emb_dim=32)
    return EtudeDecoder(EtudeDecoderConfig(**synth.decoder_dims(**over)), synth.decoder_state_dict(5, over), "cuda", precision=precision, max_streams=max_streams)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("which,rows", [("fp32", 12), ("small_f16", 5)])
def test_unfused_step_draws_with_the_slot_key_and_the_slot_counter(dev, which, rows, k):
    rng = np.random.default_rng(500 + rows + k)
    spare = 2
    dec = _decoder("fp32", max_streams=rows + spare) if which == "fp32" else _small_decoder("f16", rows + spare)
    t = Tally()
    for rep in range(-(-120 // rows)):
        slots = _slot_list(rng, rows, rep % 2 == 0, spare)
        key_of_slot = _keys(rng, rows + spare)[rng.permutation(rows + spare)]
        temperature, top_p = SETTINGS[rep % 4]
        seed = int(rng.integers(0, 1 << 63))
        _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, np.arange(rows + spare), key_of_slot)
        _begin(dec, _prompts(rng, rows, 20, 60), (2, 1, 1, 1), slots, k + 3)
        dec.debug_step_logits(True)
        _step(dec, slots, k)
        lg = dec.debug_step_logits(False, rows)
        toks, cnt = _read(dec, slots, k + 3)
        assert (cnt == k + 1).all()
        t.judge(lg, toks[:, k], temperature, top_p, seed, key_of_slot[slots], np.full(rows, k, np.uint64), what=f"rep {rep}")
    t.close(f"k_dargmax in a step, {which}, {rows} rows, step {k}")
    dec.close()


# ------------------------------------------------------------------------------------------------ (e) keys under restart
@pytest.mark.parametrize("toggle_greedy", [False, True])
def test_restarted_slots_draw_with_their_new_keys(dev, toggle_greedy):
    """Continuous batching: slots 2 and 5 start a new bar (new keys, new prompts) while the other six are three tokens into theirs.  After
    two more steps the restarted slots have drawn with the NEW keys and counter 2, the others with the old keys and counter 5."""
    rng = np.random.default_rng(41)
    dec = _decoder("f16", max_streams=8)
    slots, re = np.arange(8), np.asarray([2, 5])
    t = Tally()
    for rep in range(16):
        temperature, top_p = SETTINGS[rep % 4]
        seed = int(rng.integers(0, 1 << 63))
        old, new = _keys(rng, 8), _keys(rng, 2) + np.uint64(1 << 20)
        _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, slots, old)
        _begin(dec, _prompts(rng, 8, 20, 60), (2, 1, 1, 1), slots, 12)
        _step(dec, slots, 3)
        if toggle_greedy:                                        # the captured step graph reads the device-side config: greedy and back changes nothing
            _set_sampling(dec, 0.0, 1.0, 0)
            _set_sampling(dec, temperature, top_p, seed)
        _set_keys(dec, re, new)
        _begin(dec, _prompts(rng, 2, 20, 60), (2, 0, 2, 1), re, 12)
        dec.debug_step_logits(True)
        _step(dec, slots, 2)
        lg = dec.debug_step_logits(False, 8)
        toks, cnt = _read(dec, slots, 12)
        want_cnt = np.full(8, 6); want_cnt[re] = 3
        assert np.array_equal(cnt, want_cnt), cnt
        keys = old.copy(); keys[re] = new
        last = toks[np.arange(8), cnt - 1]
        t.judge(lg, last, temperature, top_p, seed, keys, (cnt - 1).astype(np.uint64), what=f"rep {rep}")
    t.close(f"keys under restart{', greedy and back in between' if toggle_greedy else ''}")
    dec.close()


# ------------------------------------------------------------------------------------------------ (f) switching
def _vocab():
    from etude_amd.vocab import Vocab
    v = Vocab()
    v.token_to_id = synth.vocab_json()["token_to_id"]
    v.id_to_token = [""] * len(v.token_to_id)
    for tk, i in v.token_to_id.items():
        v.id_to_token[i] = tk
    return v


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_greedy_after_sampling_equals_a_fresh_engine(dev, precision):
    v = _vocab()
    jobs = []
    for s in range(5):
        bars = synth.song_bars(seed=170 + s, n_bars=3)
        jobs.append((bars, [synth.attrs(s % 3, (s + 1) % 3, 1, 2)] * len(bars)))
    used = _decoder(precision, max_streams=6)
    sampled = used.generate_many(jobs, v, max_bar_token_limit=20, temperature=1.2, top_p=0.9, seed=3)
    after = used.generate_many(jobs, v, max_bar_token_limit=20)
    used.close()
    fresh = _decoder(precision, max_streams=6)
    greedy = fresh.generate_many(jobs, v, max_bar_token_limit=20)
    fresh.close()
    assert after == greedy and sampled != greedy
