"""Teacher-forced scoring on the GPU (etd_decoder_score / etd_decoder_score_jobs; EtudeDecoder.forward and score_many) against data pinned by the
reference (decoder_full.npz logits, clip_ctx.npz greedy ids) or by the oracle (oracle.neox.forward_logits)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from etude_amd import _lib, synth
from etude_amd.decoder import ABI_ATTR_KEYS, IGNORE_INDEX

pytestmark = pytest.mark.gpu

BOS, EOS = 4, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _vocab():
    from etude_amd.vocab import Vocab
    v = Vocab()
    v.token_to_id = synth.vocab_json()["token_to_id"]
    v.id_to_token = [""] * len(v.token_to_id)
    for t, i in v.token_to_id.items():
        v.id_to_token[i] = t
    return v


def _decoder(precision, weights="bench", **kw):
    from etude_amd.decoder import EtudeDecoder, EtudeDecoderConfig
    sd = synth.decoder_state_dict_ctx(1) if weights == "ctx" else synth.decoder_state_dict(1, {})
    return EtudeDecoder(EtudeDecoderConfig(**synth.decoder_dims()), sd, "cuda", precision=precision, **kw)


def _clip_bars(golden_dir):
    g = np.load(golden_dir / "clip_full.npz")
    flat, lens = g["bar_ids"].tolist(), g["bar_lens"].tolist()
    bars, p = [], 0
    for l in lens:
        bars.append(flat[p:p + l]); p += l
    return bars


def _scored_sequence(hist, x, y, ya, limit=512, ratio=0.5, n_ctx=4, max_pos=1024):
    """the sequence score_many builds for a bar (etd_debug_assemble_scored; pinned to the oracle's prompt rule by tests/test_score_cpu.py)"""
    sc = _lib.SchedCfg(bar_bos_id=BOS, bar_eos_id=EOS, n_ctx_pairs=n_ctx, max_position_embeddings=max_pos, max_output_tokens=0,
                       max_bar_token_limit=limit, context_overlap_ratio=ratio, max_streams=1, max_prefill_rows=1, steps_per_poll=1)
    hist = hist[-n_ctx:]
    n = len(hist)
    hx = [np.asarray(h[0], np.int32) for h in hist]
    hy = [np.asarray(h[1], np.int32) for h in hist]
    hxp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in hx])
    hyp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in hy])
    hxn = np.asarray([a.size for a in hx] or [0], np.int32)
    hyn = np.asarray([a.size for a in hy] or [0], np.int32)
    ha = np.ascontiguousarray(np.asarray([[h[2][k] for k in ABI_ATTR_KEYS] for h in hist] or [[0, 0, 0, 0]], np.int32))
    xa, yv = np.asarray(x, np.int32), np.asarray(y, np.int32)
    yat = np.asarray([ya[k] for k in ABI_ATTR_KEYS], np.int32)
    cap = 4096
    ids, cls, lab, at = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((4, cap), np.int32)
    T = C.c_int()
    _lib.check(_lib.lib().etd_debug_assemble_scored(C.byref(sc), n, hxp, hxn.ctypes.data, hyp, hyn.ctypes.data, ha.ctypes.data, xa.ctypes.data, xa.size,
                                                    yv.ctypes.data, yv.size, yat.ctypes.data, ids.ctypes.data, cls.ctypes.data, at.ctypes.data,
                                                    lab.ctypes.data, cap, C.byref(T)), "assemble_scored")
    t = T.value
    return ids[:t], cls[:t], at[:, :t], lab[:t]


def _fwd(dec, ids, cls, a4, labels=None, mask=None, **kw):
    """forward() with the reference's keyword names; ids / cls / labels [B, T], a4 [B, 4, T] in ABI order"""
    return dec(input_ids=ids, class_ids=cls, pitch_overlap_bin_ids=a4[:, 0], polyphony_bin_ids=a4[:, 1], note_sustain_bin_ids=a4[:, 2],
               rhythm_intensity_bin_ids=a4[:, 3], attention_mask=mask, labels=labels, **kw)


@pytest.mark.parametrize("precision,ltol,tol", [("fp32", 1e-4, 1e-4), ("f16", 2e-2, 1e-2)])
def test_forward_loss_pinned_by_reference_logits(dev, golden_dir, precision, ltol, tol):
    g = np.load(golden_dir / "decoder_full.npz")
    dec = _decoder(precision)
    ids = g["prompt_ids"][0].astype(np.int64)
    a4 = np.stack([g["prompt_overlap"][0], g["prompt_polyphony"][0], g["prompt_sustain"][0], g["prompt_rhythm"][0]]).astype(np.int64)
    labels = np.concatenate([ids[1:], [IGNORE_INDEX]])
    ref = g["logits"].astype(np.float64)
    lse = ref.max(-1) + np.log(np.exp(ref - ref.max(-1, keepdims=True)).sum(-1))
    want = float(np.mean(lse[:-1] - ref[np.arange(63), labels[:-1]]))
    out = _fwd(dec, torch.from_numpy(ids[None]).to(dev), g["prompt_cls"][0][None].astype(np.int64), a4[None], torch.from_numpy(labels[None]))
    assert out.logits.shape == (1, 64, 154) and out.logits.dtype == torch.float32 and out.logits.device.type == "cuda"
    assert out.loss.dim() == 0 and out.loss.dtype == torch.float32 and out.past_key_values is None
    lerr = float(np.abs(out.logits[0].cpu().numpy() - ref).max())
    err = abs(float(out.loss) - want)
    print(f"[measured] forward {precision}: loss {float(out.loss):.6f} vs reference {want:.6f} (err {err:.2e}), logits err {lerr:.2e}")
    assert err < ltol and lerr < tol
    loss2, logits2 = _fwd(dec, ids[None], g["prompt_cls"][0][None].astype(np.int64), a4[None], labels[None], return_dict=False)
    assert float(loss2) == float(out.loss) and torch.equal(logits2, out.logits)
    (only,) = _fwd(dec, ids[None], g["prompt_cls"][0][None].astype(np.int64), a4[None], return_dict=False)
    assert torch.equal(only, out.logits)
    none = _fwd(dec, ids[None], g["prompt_cls"][0][None].astype(np.int64), a4[None], np.full((1, 64), IGNORE_INDEX))
    assert torch.isnan(none.loss)
    dec.close()


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_forward_right_padded_batch_equals_rows_alone(dev, precision):
    """EtudeDataset.collate_fn's batch layout: ragged rows right-padded with pad id 0 / class 0 / attribute 0 / label -100, mask 1 then 0"""
    rng = np.random.default_rng(4)
    lens = [37, 64, 5, 120, 90]
    B, T = len(lens), max(lens)
    ids, cls, lab, mask = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64), np.full((B, T), IGNORE_INDEX, np.int64), np.zeros((B, T), np.int64)
    a4 = np.zeros((B, 4, T), np.int64)
    for b, L in enumerate(lens):
        ids[b, :L] = rng.integers(4, 154, L)
        cls[b, :L] = rng.integers(1, 3, L)
        a4[b, :, :L] = rng.integers(0, 3, (4, L))
        mask[b, :L] = 1
        ctx = int(rng.integers(0, L - 1))
        lab[b, ctx:L - 1] = ids[b, ctx + 1:L]                  # dataset.py:426: -100 on the context, the next token on the rest, -100 last
    dec = _decoder(precision)
    out = _fwd(dec, ids, cls, a4, lab, mask)
    lg = out.logits.cpu()
    tot, cnt = 0.0, 0
    for b, L in enumerate(lens):
        alone = _fwd(dec, ids[b:b + 1, :L], cls[b:b + 1, :L], a4[b:b + 1, :, :L], lab[b:b + 1, :L])
        n = int((lab[b, :L] != IGNORE_INDEX).sum())
        tot += float(alone.loss) * n; cnt += n
        if precision == "fp32":
            assert torch.equal(lg[b, :L], alone.logits[0].cpu()), b      # README: the fp32 mode does not depend on the batch
        else:
            assert float((lg[b, :L] - alone.logits[0].cpu()).abs().max()) < 1e-2, b
        assert (lg[b, L:] == 0).all()
    assert abs(float(out.loss) - tot / cnt) < 1e-6
    ce = F.cross_entropy(out.logits.view(-1, 154), torch.from_numpy(lab).to(dev).view(-1))
    assert abs(float(out.loss) - float(ce)) < 1e-5
    with pytest.raises(ValueError):
        _fwd(dec, ids, cls, a4, lab, mask[:, ::-1].copy())     # left padding
    bad = lab.copy(); bad[2, T - 1] = 7
    with pytest.raises(ValueError):
        _fwd(dec, ids, cls, a4, bad, mask)
    with pytest.raises(_lib.EtudeHipError):
        _fwd(dec, ids, cls, a4, np.where(lab == IGNORE_INDEX, IGNORE_INDEX, 154), mask)   # label outside the vocabulary
    dec.close()


def _covers(dec, v, bars, tuples, limit, temperature=0.0, seed=None):
    return [dec.generate_ids(v, bars, [t] * len(bars), max_bar_token_limit=limit, temperature=temperature, seed=seed) for t in tuples]


@pytest.mark.parametrize("precision,tok_tol", [("fp32", 1e-4), ("f16", 2e-2)])
def test_score_many_against_oracle(dev, precision, tok_tol):
    """8 bars x 2 tuples, bench weights, SAMPLED covers (the forced tokens are not all the argmax): each bar's log-likelihood = the oracle's
    log_softmax at the forced tokens, summed over the bar; a budget-stopped cover (its first 5 bars) scores those bars the same"""
    from oracle import neox
    v = _vocab()
    bars = synth.song_bars(seed=3, n_bars=8)
    tuples = [synth.attrs(1, 1, 1, 2), synth.attrs(2, 0, 1, 2)]
    limit = 48
    dec = _decoder(precision, max_streams=4)
    covers = _covers(dec, v, bars, tuples, limit, temperature=1.0, seed=7)
    res = dec.score_many([(bars, c, [t] * len(bars)) for c, t in zip(covers, tuples)] + [(bars, covers[0][:5], [tuples[0]] * len(bars))], v,
                         max_bar_token_limit=limit)
    tsd = {k: torch.from_numpy(x) for k, x in synth.decoder_state_dict(1, {}).items()}
    nd = neox.NeoxDims()
    worst = 0.0
    for c, t, r in zip(covers, tuples, res):
        assert r.bar_logprob.dtype == np.float64 and len(r.bar_logprob) == len(c)
        assert r.bar_tokens.tolist() == [len(y) - 1 for y in c]
        hist = []
        for i, (x, y) in enumerate(zip(bars, c)):
            ids, cls, a4, lab = _scored_sequence([(h[0], h[1], t) for h in hist], x, y, t, limit)
            hist.append((x, y))
            at = {"pitch_overlap": a4[0], "polyphony": a4[1], "note_sustain": a4[2], "rhythm_intensity": a4[3]}
            lg, _ = neox.forward_logits(tsd, nd, torch.from_numpy(ids.astype(np.int64))[None], torch.from_numpy(cls.astype(np.int64))[None],
                                        {k: torch.from_numpy(a.astype(np.int64))[None] for k, a in at.items()})
            ls = torch.log_softmax(lg[0].double(), -1).numpy()
            rows = np.nonzero(lab != IGNORE_INDEX)[0]
            want = float(ls[rows, lab[rows]].sum())
            err = abs(r.bar_logprob[i] - want)
            worst = max(worst, err / max(len(rows), 1))
            assert err < tok_tol * max(len(rows), 1), (i, r.bar_logprob[i], want)
            hits = int((lg[0].numpy()[rows].argmax(-1) == lab[rows]).sum())
            if precision == "fp32":
                assert r.bar_greedy_hits[i] == hits, i
            assert 0 <= r.bar_greedy_hits[i] <= r.bar_tokens[i]
    print(f"[measured] score_many {precision}: worst |bar_logprob - oracle| per token {worst:.2e} (tol {tok_tol:.0e})")
    assert np.array_equal(res[2].bar_tokens, res[0].bar_tokens[:5])
    if precision == "fp32":      # (16-bit: other neighbours in the batched prefill, other roundings -- README "Reproducibility")
        assert np.array_equal(res[2].bar_logprob, res[0].bar_logprob[:5]) and np.array_equal(res[2].bar_greedy_hits, res[0].bar_greedy_hits[:5])
    else:
        assert (np.abs(res[2].bar_logprob - res[0].bar_logprob[:5]) < tok_tol * res[2].bar_tokens).all()
    dec.close()


def test_reference_greedy_ids_are_greedy_under_scoring(dev, golden_dir):
    """the reference's own 13 217 greedy ids of clip_ctx.npz (ctx weights, 92 clip_full bars, attrs (1, 1, 1, 2)): every forced token is the
    scored row's argmax, or the row is a near-tie (top-2 margin < 1e-4, checked through forward on that bar)"""
    g = np.load(golden_dir / "clip_ctx.npz")
    v = _vocab()
    bars = _clip_bars(golden_dir)
    t = synth.attrs(1, 1, 1, 2)
    dec = _decoder("fp32", "ctx")
    # the reference's ids cut into bars: generated tokens can themselves be Bar_BOS, so the bar boundaries come from the engine's own greedy run,
    # whose flat ids are the reference's (test_gpu_decoder_parity.py::test_whole_song_context_weights_against_reference; checked again here)
    cover = dec.generate_ids(v, bars, [t] * len(bars), temperature=0.0)
    assert [i for y in cover for i in y] == g["gen_ids"].tolist() and len(cover) == len(bars)
    (r,) = dec.score_many([(bars, cover, [t] * len(bars))], v)
    assert r.bar_tokens.tolist() == [len(y) - 1 for y in cover] and int(r.bar_tokens.sum()) == len(g["gen_ids"]) - len(bars)
    ties = 0
    for i in np.nonzero(r.bar_greedy_hits != r.bar_tokens)[0]:
        hist = [(bars[j], cover[j], t) for j in range(max(0, i - 4), i)]
        ids, cls, a4, lab = _scored_sequence(hist, bars[i], cover[i], t)
        lg = _fwd(dec, ids[None].astype(np.int64), cls[None].astype(np.int64), a4[None].astype(np.int64)).logits[0].cpu().numpy()
        rows = np.nonzero(lab != IGNORE_INDEX)[0]
        for row in rows[lg[rows].argmax(-1) != lab[rows]]:
            top2 = np.sort(lg[row])[-2:]
            assert top2[1] - lg[row, lab[row]] < 1e-4 and top2[1] - top2[0] < 1e-4, (i, row)
            ties += 1
    print(f"[measured] clip_ctx: {int(r.bar_tokens.sum())} scored ids, {ties} near-tie rows whose argmax is not the reference's id")
    assert int((r.bar_tokens - r.bar_greedy_hits).sum()) == ties
    dec.close()


def _layout_jobs(v, bars, tuples, covers):
    return [(bars, c, [t] * len(bars)) for c, t in zip(covers, tuples)]


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_scores_layout_invariant_and_reproducible(dev, precision):
    """fp32: bit-identical at max_streams 1, 7 and 64 and run to run; 16-bit: bit-identical run to run, within tolerance across layouts
    (a <= 512-row prefill rounds differently, README "Reproducibility").  Default limits: prompts of up to 513 rows, so sequences run both
    on the <= 512-row kernels and alone on the big-tile ones."""
    v = _vocab()
    bars = synth.song_bars(seed=5, n_bars=12)
    tuples = [synth.attrs(p, r, 1, 2) for p in range(3) for r in (0, 2)]
    gen = _decoder(precision, max_streams=8)
    covers = [gen.generate_many([(bars, [t] * len(bars))], v, temperature=0.0)[0] for t in tuples]
    gen.close()
    jobs = _layout_jobs(v, bars, tuples, covers)
    got = {}
    for S in (1, 7, 64):
        dec = _decoder(precision, max_streams=S)
        a = dec.score_many(jobs, v)
        b = dec.score_many(jobs, v)
        for ra, rb in zip(a, b):
            assert np.array_equal(ra.bar_logprob, rb.bar_logprob) and np.array_equal(ra.bar_greedy_hits, rb.bar_greedy_hits), S   # run to run
        got[S] = a
        dec.close()
    for S in (7, 64):
        for r1, rs in zip(got[1], got[S]):
            assert np.array_equal(r1.bar_tokens, rs.bar_tokens)
            if precision == "fp32":
                assert np.array_equal(r1.bar_logprob, rs.bar_logprob) and np.array_equal(r1.bar_greedy_hits, rs.bar_greedy_hits), S
            else:
                assert np.abs(r1.bar_logprob - rs.bar_logprob).max() < 2e-2 * max(int(r1.bar_tokens.max()), 1), S


def test_no_state_leak_between_score_and_generate(dev):
    v = _vocab()
    bars = synth.song_bars(seed=3, n_bars=6)
    at = [synth.attrs(1, 1, 1, 2)] * len(bars)
    dec = _decoder("fp32", max_streams=4)
    first = dec.generate_ids(v, bars, at, temperature=0.0, max_bar_token_limit=64)
    other = [[BOS] + list(range(10, 40)) + [EOS]] * len(bars)
    dec.score_many([(bars, other, at), (bars, first, at)], v, max_bar_token_limit=64)
    again = dec.generate_ids(v, bars, at, temperature=0.0, max_bar_token_limit=64)
    assert again == first
    dec.close()
