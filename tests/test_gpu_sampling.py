"""Sampling branch of generate() (etude_decoder.py:321-331) through the C ABI.
The reference draws with torch.multinomial from torch's global generator, so draws cannot be compared one by one; what
IS pinned: (1) the distribution -- softmax(logits / T) with the top-p filter -- against the oracle's restatement of
:321-330 on the GPU's own logits, by frequency over thousands of draws and by support (a token the filter removes must
never appear); (2) degenerate settings that make sampling deterministic reproduce the greedy ids exactly;
(3) reproducibility: same seed -> same tokens, independent of stream count / slot placement."""
import ctypes as C

import numpy as np
import pytest
import torch

from etude_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _decoder(precision, **kw):
    from etude_amd.decoder import EtudeDecoder, EtudeDecoderConfig
    return EtudeDecoder(EtudeDecoderConfig(**synth.decoder_dims()), synth.decoder_state_dict(1, {}), "cuda", precision=precision, **kw)


def _vocab():
    from etude_amd.vocab import Vocab
    v = Vocab()
    v.token_to_id = synth.vocab_json()["token_to_id"]
    v.id_to_token = [""] * len(v.token_to_id)
    for t, i in v.token_to_id.items():
        v.id_to_token[i] = t
    return v


def _first_tokens(dec, ids, cls, a4, n_streams, temperature, top_p, seed, key0=0):
    """prefill the same prompt on n_streams streams with different draw keys -> the first generated token of each"""
    lib = _lib.lib()
    st = dec._stream()
    T = len(ids)
    n = n_streams
    slots = np.arange(n, dtype=np.int32)
    _lib.check(lib.etd_decoder_set_sampling(dec._h, temperature, top_p, seed, st), "set_sampling")
    keys = (np.arange(n, dtype=np.uint64) + np.uint64(key0))
    _lib.check(lib.etd_decoder_set_keys(dec._h, n, slots.ctypes.data, keys.ctypes.data), "set_keys")
    Ts = np.full(n, T, np.int32)
    tg = np.tile(np.asarray([2, 1, 1, 1], np.int32), n)
    eos = np.full(n, -1, np.int32); lim = np.full(n, 4, np.int32)
    ids_n, cls_n, a4_n = np.tile(ids, n), np.tile(cls, n), np.ascontiguousarray(np.tile(a4, (1, n)))      # keep the buffers alive over the call
    _lib.check(lib.etd_decoder_begin_bars(dec._h, n, slots.ctypes.data, Ts.ctypes.data, ids_n.ctypes.data, cls_n.ctypes.data,
                                          a4_n.ctypes.data, tg.ctypes.data, eos.ctypes.data, lim.ctypes.data, st), "begin_bars")
    out = np.zeros((n, 8), np.int32); cnt = np.zeros(n, np.int32)
    _lib.check(lib.etd_decoder_read_many(dec._h, n, slots.ctypes.data, out.ctypes.data, 8, cnt.ctypes.data, st), "read_many")
    assert (cnt == 1).all()
    return out[:, 0].copy()


@pytest.mark.parametrize("precision,temperature,top_p", [("fp32", 0.8, 0.9), ("fp32", 1.5, 0.6), ("f16", 1.0, 1.0)])
def test_first_token_distribution_matches_the_reference_filter(dev, precision, temperature, top_p):
    from oracle import neox
    dec = _decoder(precision, max_streams=256)
    rng = np.random.default_rng(3)
    T = 40
    ids = rng.integers(6, 154, T).astype(np.int32); cls = rng.integers(1, 3, T).astype(np.int32); a4 = rng.integers(0, 3, (4, T)).astype(np.int32)
    logits = dec.prefill_logits(ids, cls, a4)[-1]                                   # the GPU's own next-token logits
    want = neox.sampling_distribution(torch.from_numpy(logits)[None], temperature, top_p)[0].numpy().astype(np.float64)
    draws = np.concatenate([_first_tokens(dec, ids, cls, a4, 256, temperature, top_p, seed=1000 + r) for r in range(24)])
    N = draws.size
    freq = np.bincount(draws, minlength=want.size) / N
    # support: nothing the top-p filter removed may ever be drawn -- exactly: every drawn token lies in the support the restatement
    # (tests/sample_np.py) allows for these logits, i.e. the float64 filter widened by the fp32 slack of the cumulative sums at the cut
    from tests import sample_np as sn
    r64 = sn.Row64(logits, np.float32(1.0) / np.float32(temperature), top_p, sn.delta_for(logits.size))
    allowed = r64.support_slack()
    assert set(np.unique(draws).tolist()) <= allowed, sorted(set(np.unique(draws).tolist()) - allowed)
    assert freq[want == 0].sum() <= 1e-9                                            # and against the oracle's own fp32 filter, as before
    # frequencies: every token within 5 sigma of its probability, total variation small
    sigma = np.sqrt(np.maximum(want * (1 - want), 1e-12) / N)
    assert (np.abs(freq - want) <= 5 * sigma + 2e-3).all(), np.abs(freq - want).max()
    assert 0.5 * np.abs(freq - want).sum() < 0.06
    assert (freq > 0).sum() > 1 or r64.p.max() > 0.99                               # it does sample, not argmax


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_degenerate_sampling_equals_greedy_and_seeds_reproduce(dev, precision):
    dec = _decoder(precision, max_streams=6)
    v = _vocab()
    jobs = []
    for s in range(5):
        bars = synth.song_bars(seed=70 + s, n_bars=3)
        jobs.append((bars, [synth.attrs(s % 3, (s + 1) % 3, 1, 2)] * len(bars)))
    greedy = dec.generate_many(jobs, v, max_bar_token_limit=20)
    # top_p -> 0 keeps only the most probable token (:326-328: the first sorted token is never removed)
    assert dec.generate_many(jobs, v, max_bar_token_limit=20, temperature=0.7, top_p=1e-6, seed=5) == greedy
    a = dec.generate_many(jobs, v, max_bar_token_limit=20, temperature=1.3, top_p=0.95, seed=11)
    b = dec.generate_many(jobs, v, max_bar_token_limit=20, temperature=1.3, top_p=0.95, seed=11)
    c = dec.generate_many(jobs, v, max_bar_token_limit=20, temperature=1.3, top_p=0.95, seed=12)
    assert a == b and a != c and a != greedy
    # draws are keyed by (job, bar, token index): a different stream count / placement does not change them.  Exact in fp32 mode
    # (its logits do not depend on the batch shape); in bf16 the GEMM path changes with the batch, logits move in the last bits and
    # a draw that sits on a CDF boundary may flip, so only same-configuration reproducibility is promised there.
    if precision == "fp32":
        one = _decoder(precision, max_streams=2)
        assert one.generate_many(jobs, v, max_bar_token_limit=20, temperature=1.3, top_p=0.95, seed=11) == a
    ev = dec.generate(v, jobs[0][0], jobs[0][1], max_bar_token_limit=20, temperature=0.9, top_p=0.9, seed=3)
    assert len(ev) > 0 and dec.generate_many(jobs, v, max_bar_token_limit=20) == greedy     # greedy again after sampling calls
