"""tests/sample_np.py -- the numpy restatement every exact sampling test on the GPU is judged by -- pinned without a GPU:
its float64 path against the oracle's restatement of etude_decoder.py:321-330, its slack `delta` against its own float32
path under two summation orders, the share of draws the slack leaves undecided (a condition: <= 5 %), the generator's
uniformity and independence, and the draw frequencies against the distribution."""
import math

import numpy as np
import pytest
import torch

from etude_amd import synth
from tests import sample_np as sn
from tests._util import neox_dims, torch_sd

SETTINGS = [(0.8, 0.9), (1.5, 0.6), (1.0, 1.0), (0.7, 0.3)]          # (temperature, top_p)
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def oracle_rows():
    """480 next-token logit rows of the oracle: 2 prompts x 120 positions, benchmark and context weights"""
    from oracle import neox
    rng = np.random.default_rng(21)
    rows = []
    for sd_np in (synth.decoder_state_dict(1, {}), synth.decoder_state_dict_ctx(1)):
        sd = torch_sd(sd_np)
        for _ in range(2):
            T = 120
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.int64))[None]      # noqa: E731
            ids, cls, a4 = rng.integers(6, 154, T), rng.integers(1, 3, T), rng.integers(0, 3, (4, T))
            lg, _ = neox.forward_logits(sd, neox_dims({}), t(ids), t(cls), {"pitch_overlap": t(a4[0]), "polyphony": t(a4[1]), "note_sustain": t(a4[2]),
                                                                           "rhythm_intensity": t(a4[3])})
            rows.append(lg[0].numpy().astype(np.float32))
    rows = np.concatenate(rows)
    rows.setflags(write=False)
    return rows


def _hand_rows():
    ninf = -np.inf
    return {
        "ties_across_cut": np.asarray([1.0, 3.0, 3.0, 3.0, 0.0, 3.0, -2.0], np.float32),
        "cum_equals_top_p": np.asarray([-2 * LN2, 0.0, -2 * LN2, -LN2], np.float32),      # ~ 1/8, 1/2, 1/8, 1/4 (exact in float64: CUM64 below)
        "one_hot": np.asarray([-200.0, -200.0, 50.0, -200.0, -200.0], np.float32),
        "one_hot_first": np.asarray([9.0] + [-300.0] * 9, np.float32),
        "neg_inf": np.asarray([0.5, ninf, 1.5, ninf, -0.5, 0.25, ninf, ninf], np.float32),
        "neg_inf_but_one": np.asarray([ninf, ninf, 0.0, ninf], np.float32),
        "v1": np.asarray([0.3], np.float32),
        "v2": np.asarray([-0.2, 0.4], np.float32),
        "v2_tie": np.asarray([1.0, 1.0], np.float32),
    }


CUM64 = np.asarray([-2 * LN2, 0.0, -2 * LN2, -LN2], np.float64)          # exact multiples of ln 2 in float64: probabilities 1/8, 1/2, 1/8, 1/4


def _check_against_oracle(row, temperature, top_p, tie_free=True, scaled64=None):
    from oracle import neox
    inv = np.float32(1.0) / np.float32(temperature)
    r = sn.Row64(row, inv, top_p, 0.0, scaled64=scaled64)
    t64 = (np.asarray(row, np.float32) * inv).astype(np.float64) if scaled64 is None else scaled64   # the oracle gets the same scaled logits, in float64
    want = neox.sampling_distribution(torch.from_numpy(t64)[None], 1.0, float(np.float32(top_p)))[0].numpy()
    got = r.probs()
    if tie_free:
        assert set(np.nonzero(want)[0].tolist()) == set(r.support()[r.p[r.support()] > 0].tolist())
        assert np.abs(got - want).max() <= 1e-12
    else:       # torch.sort does not promise an order among equal probabilities: the kept VALUES must agree, and ours must be the lower indices
        assert np.abs(np.sort(got) - np.sort(want)).max() <= 1e-12
    return r


@pytest.mark.parametrize("temperature,top_p", SETTINGS)
def test_float64_path_equals_the_oracle_filter(oracle_rows, temperature, top_p):
    for row in oracle_rows[::3]:
        _check_against_oracle(row, temperature, top_p)
    for name, row in _hand_rows().items():
        _check_against_oracle(row, temperature, top_p, tie_free=name not in ("ties_across_cut", "v2_tie"))


def test_hand_made_edges():
    h = _hand_rows()
    # four equal maxima of probability 0.2386 each at ids 1, 2, 3, 5: cut after the second / third -- the lower indices survive
    for top_p, keep in ((0.3, [1, 2]), (0.5, [1, 2, 3]), (0.74, [1, 2, 3, 5]), (1e-6, [1])):
        r = _check_against_oracle(h["ties_across_cut"], 1.0, top_p, tie_free=False)
        assert r.support().tolist() == keep, (top_p, r.support(), r.K)
        r32 = sn.Row32(h["ties_across_cut"], 1.0, top_p)
        assert r32.si[:r32.K].tolist() == r.support().tolist()
    # cumulative sum == top_p exactly: 1/2 + 1/4 = 0.75 is NOT > 0.75, so the third token stays and the fourth goes
    r = _check_against_oracle(h["cum_equals_top_p"], 1.0, 0.75, tie_free=False, scaled64=CUM64)
    assert r.p[[1, 3, 0, 2]].tolist() == [0.5, 0.25, 0.125, 0.125] and r.cum[1] == 0.75        # the case is what it claims to be
    assert r.support().tolist() == [1, 3, 0] and r.K == 3
    assert sn.Row64(h["cum_equals_top_p"], 1.0, 0.75, 1e-6).K_lo == 2                           # and the slack tries both cuts
    assert sn.Row64(h["cum_equals_top_p"], 1.0, 0.75, 1e-6).K_hi == 3
    # one-hot, -inf, V = 1, 2
    for key in range(50):
        assert sn.draw_set(h["one_hot"], 1.0, 0.9, 1, key, 0, 1e-5) == {2} and sn.draw32(h["one_hot"], 1.0, 0.9, 1, key, 0) == 2
        assert sn.draw_set(h["one_hot_first"], 0.5, 1.0, 1, key, 3, 1e-5) == {0}
        assert sn.draw_set(h["v1"], 1.0, 0.5, 1, key, 0, 1e-5) == {0} and sn.draw32(h["v1"], 1.0, 0.5, 1, key, 0) == 0
        assert sn.draw_set(h["neg_inf_but_one"], 1.0, 1.0, 1, key, 0, 1e-5) == {2} and sn.draw32(h["neg_inf_but_one"], 1.0, 1.0, 1, key, 0) == 2
        s = sn.draw_set(h["neg_inf"], 1.0, 1.0, 7, key, 1, 1e-5)
        assert s <= {0, 2, 4, 5} and sn.draw32(h["neg_inf"], 1.0, 1.0, 7, key, 1) in s
        assert sn.draw_set(h["v2"], 1.0, 1.0, 1, key, 0, 1e-5) <= {0, 1}
    r = sn.Row64(h["neg_inf"], 1.0, 1.0, 1e-5)
    assert r.si.tolist() == [2, 0, 5, 4, 1, 3, 6, 7] and (r.p[[1, 3, 6, 7]] == 0).all()        # -inf: probability 0, last, in index order
    assert sn.Row64(h["v2_tie"], 1.0, 0.4, 0.0).support().tolist() == [0]
    # 0 < top_p < 1 alone filters
    for tp in (-1.0, 0.0, 1.0, 2.0):
        assert sn.Row64(h["ties_across_cut"], 1.0, tp, 0.0).K == 7 and sn.Row32(h["ties_across_cut"], 1.0, tp).K == 7


@pytest.fixture(scope="module")
def triples(oracle_rows):
    """per setting: (non-decisive, total, mismatches) over 480 rows x 8 keys x 2 counters; float32 draws in both summation orders vs draw_set"""
    rng = np.random.default_rng(5)
    out = {}
    V = oracle_rows.shape[1]
    delta = sn.delta_for(V)
    for temperature, top_p in SETTINGS:
        inv = np.float32(1.0) / np.float32(temperature)
        nd = tot = bad = 0
        for i, row in enumerate(oracle_rows):
            r64 = sn.Row64(row, inv, top_p, delta)
            r32 = [sn.Row32(row, inv, top_p, order) for order in ("seq", "wave")]
            keys = rng.integers(0, 1 << 63, 8, dtype=np.uint64) | (np.uint64(i) << np.uint64(32))
            for key in keys.tolist():
                for ctr in (0, int(rng.integers(1, 600))):
                    u = sn.u24(1234, key, ctr)
                    s = r64.pick_set(u)
                    tot += 1
                    if len(s) != 1:
                        nd += 1
                        continue
                    bad += sum(int(r.pick(u)) not in s for r in r32)
        out[(temperature, top_p)] = (nd, tot, bad)
    return out


def test_delta_holds_for_the_reference_alone(triples):
    assert sum(t for _, t, _ in triples.values()) >= 20000
    for setting, (nd, tot, bad) in triples.items():
        print(f"T, top_p = {setting}: decisive {tot - nd}/{tot}, float32 draws outside a singleton set: {bad}")
        assert bad == 0, setting


def test_decisive_share(triples):
    for setting, (nd, tot, _) in triples.items():
        print(f"T, top_p = {setting}: non-decisive {nd}/{tot} = {100.0 * nd / tot:.2f} % at delta {sn.delta_for(154):.2e}")
        assert nd <= 0.05 * tot, setting


def test_vector_and_scalar_generator_agree():
    rng = np.random.default_rng(2)
    seeds, keys = rng.integers(0, 1 << 63, 64, dtype=np.uint64), rng.integers(0, 1 << 63, 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ctrs = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    got = sn.u24_np(seeds, keys, ctrs)
    assert got.tolist() == [sn.u24(int(s), int(k), int(c)) for s, k, c in zip(seeds, keys, ctrs)]
    assert sn.mix64(0) == 0xE220A8397B1DCDAF                              # splitmix64's first output for state 0


def test_generator_is_uniform_and_streams_are_uncorrelated():
    rng = np.random.default_rng(9)
    seeds = np.concatenate([np.arange(32, dtype=np.uint64), rng.integers(0, 1 << 63, 32, dtype=np.uint64) * np.uint64(2)])
    jobs, bars = np.arange(8, dtype=np.uint64), np.arange(4, dtype=np.uint64)
    keys = np.concatenate([np.arange(16, dtype=np.uint64), ((jobs[:, None] << np.uint64(32)) | bars[None, :]).ravel(),      # the scheduler's (job << 32) | bar
                           rng.integers(1 << 32, 1 << 63, 16, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    ctrs = np.arange(64, dtype=np.uint64)
    assert seeds.size == keys.size == ctrs.size == 64
    u = sn.u24_np(seeds[:, None, None], keys[None, :, None], ctrs[None, None, :]).astype(np.float64) / 2.0 ** 24     # [seed][key][ctr]
    N = u.size
    # 64-bin chi-square, 63 degrees of freedom: the 1 - 1e-6 quantile is 135.0 (Wilson-Hilferty: 63 (1 - 2/567 + 4.753 sqrt(2/567))^3)
    cnt = np.bincount((u.ravel() * 64).astype(np.int64), minlength=64)
    chi2 = float(((cnt - N / 64) ** 2 / (N / 64)).sum())
    print(f"chi-square over 64 bins, {N} draws: {chi2:.1f} (bound 135.0)")
    assert chi2 < 135.0
    # lag-0 correlation of streams that differ in ONE of seed, key, counter: n pairs of uniform variables have a sample correlation
    # of standard deviation 1 / sqrt(n); the two-sided 1e-6 quantile of a normal is 4.89 sigma.  Each axis: neighbours along it.
    z = u - 0.5
    for axis, name in enumerate(("seed", "key", "counter")):
        a, b = np.take(z, range(0, 63), axis).ravel(), np.take(z, range(1, 64), axis).ravel()
        rho = float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
        print(f"neighbouring {name}s: correlation {rho:+.2e} over {a.size} pairs (bound {4.89 / math.sqrt(a.size):.2e})")
        assert abs(rho) < 4.89 / math.sqrt(a.size), name


def test_draw_follows_the_distribution(oracle_rows):
    row = oracle_rows[77]
    N = 200000
    keys = np.random.default_rng(4).integers(0, 1 << 63, N, dtype=np.uint64)
    for temperature, top_p in SETTINGS:
        inv = np.float32(1.0) / np.float32(temperature)
        want = sn.Row64(row, inv, top_p, 0.0).probs()
        toks = sn.Row32(row, inv, top_p).pick(sn.u24_np(77, keys, 3))
        freq = np.bincount(toks, minlength=want.size) / N
        assert freq[want == 0].sum() == 0
        sigma = np.sqrt(want * (1 - want) / N)
        # 5 sigma of the binomial; + 1 / N so that a token of probability ~1e-7 drawn once does not count (its sigma is not Gaussian)
        assert (np.abs(freq - want) <= 5 * sigma + 1.0 / N).all(), (temperature, top_p, np.abs(freq - want).max())
        tv = 0.5 * np.abs(freq - want).sum()
        print(f"T, top_p = {(temperature, top_p)}: total variation {tv:.4f} over {N} draws")
        assert tv < 0.01
