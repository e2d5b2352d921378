"""Every stage of the 16-bit decoder against float64 ON ITS OWN TAPPED INPUT (teacher forcing), as tests/test_gpu_extractor_stages.py does for the extractor.

etd_debug_decoder_stage_taps copies each launch's output out of the shared workspaces, per layer; the K / V cache rows are read back.  Stage k's float64
reference (tests/dec_stage_ref.py, pinned to the oracle by tests/test_dec_stage_ref_cpu.py) is computed from the device's own tap of stage k - 1, and the same
stage with the kernels' rounding sites on (`emu`) gives the bound, never the device:  max |got - ref| <= 3 E_max, rms (got - ref) <= 2 E_rms, E = emu - ref.
Stages without a 16-bit site (slab sum + bias + residual, the next embedding) are held per cell to the fp32 bound n 2^-24 sum |terms|, row gathers bit for bit.

Cases (tests/dec_stage_ref.py: case_lengths; max_ctx 640, full geometry):
    S1  fused step, 33 rows (crosses k_dstep_qkv_up's 32-row tile, odd: the pair form's duplicate-row tail), prompts 1 .. 129 + seeded, slots not 0..n-1,
        benchmark weights, one-row and paired attention form; the tapped step is the second of two, so it reads keys written by prefill and by a step
    S2  54 rows, prompts of 300-380 tokens, context weights (sharp attention), the host's own pair rule
    S3  300 rows = 2 x 128 + 44 (k_dstep_qkv_up_mt with a ragged last tile), prompts of 20-90 tokens
    P1  prefill of 1 + 65 + 130 rows on the skinny sequence without attn_down: k_dattn with 16-bit Ob, down_splitk's 5 slabs, k_resid_ln_rows<5>
    P2  prefill of 1 282 rows = 10 x 128 + 2 (k_ln_rows, k_linear<QKV>, k_pattn, k_dmlp_fused, the last-rows tail with n = 9), both weight sets
    S4  6 rows, two of them finished by the first step (limit 2): the running rows pass the stages, the finished ones keep every cache byte, count and token
    S5  one prompt of one token: forward_plain on k_dgemv has no tap; layer 0's K / V row and the logits (whole chain) from the embedding, sites W and KV only
    P3  prefill of 96 x 513 = 49 248 rows (k_pqkv): X1b and Qb of layers 0 and 7 through a sparse layer mask, the qkv stage and the appended K / V rows
Every test prints its stages' E_max, E_rms and the two ratios ([measured], pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from tests import dec_stage_ref as sr
from tests._util import neox_dims

pytestmark = pytest.mark.gpu

H, I, NH, L, V, CTX = 512, 2048, 8, 8, 154, 640
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _decoder(weights, **kw):
    from etude_amd import synth
    from etude_amd.decoder import EtudeDecoder, EtudeDecoderConfig
    sd = synth.decoder_state_dict_ctx(sr.WEIGHT_SEED) if weights == "ctx" else synth.decoder_state_dict(sr.WEIGHT_SEED, {})
    return EtudeDecoder(EtudeDecoderConfig(**synth.decoder_dims()), sd, "cuda", precision="f16", max_ctx=CTX, **kw)


def _begin(dec, prompts, slots, limit=8):
    """limit: one bar-token limit for every stream, or one per stream"""
    from etude_amd import _lib
    n = len(prompts)
    T = np.asarray([len(p[0]) for p in prompts], np.int32)
    ids = np.concatenate([p[0] for p in prompts]); cls = np.concatenate([p[1] for p in prompts])
    a4 = np.ascontiguousarray(np.concatenate([p[2] for p in prompts], axis=1))
    tgt = np.ascontiguousarray(np.tile(np.asarray(sr.TGT_ATTRS, np.int32), (n, 1)))
    eos = np.full(n, -1, np.int32); lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, np.int32), (n,)))
    sl = np.ascontiguousarray(slots, np.int32)
    _lib.check(_lib.lib().etd_decoder_begin_bars(dec._h, n, sl.ctypes.data, T.ctypes.data, ids.ctypes.data, cls.ctypes.data, a4.ctypes.data, tgt.ctypes.data,
                                                 eos.ctypes.data, lim.ctypes.data, dec._stream()), "begin_bars")


def _step(dec, slots, n_steps):
    from etude_amd import _lib
    sl = np.ascontiguousarray(slots, np.int32)
    _lib.check(_lib.lib().etd_decoder_step(dec._h, sl.ctypes.data, len(sl), n_steps, dec._stream()), "step")


def _read(dec, slots, cap):
    from etude_amd import _lib
    sl = np.ascontiguousarray(slots, np.int32)
    out = np.zeros((len(sl), cap), np.int32); cnt = np.zeros(len(sl), np.int32)
    _lib.check(_lib.lib().etd_decoder_read_many(dec._h, len(sl), sl.ctypes.data, out.ctypes.data, cap, cnt.ctypes.data, dec._stream()), "read_many")
    return out, cnt


def _bufs(dec, spec, slices, rows):
    """device tensors of the named taps, [slices, rows, width] (int / next-step taps: [rows, ..])"""
    dt, dv = dec.operand_dtype, dec.device
    width = dict(hin=(H, torch.float32), ln1=(H, dt), ln2=(H, dt), q=(H, torch.float32), qb=(H, dt), xcat=(I + H, dt), hout=(H, torch.float32),
                 slabs=(12 * H, torch.float32), next_h=(H, torch.float32), next_ln1=(H, dt), next_ln2=(H, dt))
    out = {}
    for k in spec:
        if k in ("step_slot", "step_pos", "next_pos"):
            out[k] = torch.empty((rows,), dtype=torch.int32, device=dv)
        elif k.startswith("next_"):
            out[k] = torch.empty((rows, width[k][0]), dtype=width[k][1], device=dv)
        else:
            out[k] = torch.empty((slices, rows, width[k][0]), dtype=width[k][1], device=dv)
        out[k].view(torch.uint8).fill_(0xFF)                      # NaN patterns (ints: -1): a tap that was not written cannot pass for one that was
    return out


STEP_TAPS = ("hin", "ln1", "ln2", "q", "xcat", "slabs", "hout", "step_slot", "step_pos", "next_h", "next_ln1", "next_ln2", "next_pos")


@functools.lru_cache(maxsize=None)
def _step_run(case, weights, force_pair):
    """begin_bars, then two fused steps with every layer tapped: the second step's taps, logits, tokens and the sampled rows' cache -> host"""
    from etude_amd import _lib
    lengths = sr.case_lengths(case)
    n = len(lengths)
    prompts = sr.prompts(sr.PROMPT_SEED, lengths)
    slots = [(7 * i + 3) % (n + 4) for i in range(n)]              # injective for these row counts (asserted), not 0 .. n - 1
    assert len(set(slots)) == n and slots != list(range(n))
    dec = _decoder(weights, max_streams=n + 4)
    try:
        _lib.check(_lib.lib().etd_debug_decoder_force_pair(dec._h, force_pair), "force_pair")
        dec.debug_step_logits(True)
        limits = sr.case_limits(case)
        _begin(dec, prompts, slots, limits)
        bufs = _bufs(dec, STEP_TAPS, L, n)
        dec.debug_stage_taps(layer_mask=(1 << L) - 1, rows=n, slab_cap=12, slices=L, **bufs)
        before = None
        if case == "S4":
            # the two steps as two calls (the second replays the tapped graph the first captured), every listed slot's cache rows and counts read in between
            _step(dec, slots, 1)
            before = ([dec.debug_peek_kv(l, slots, max(lengths) + 4) for l in range(L)], _read(dec, slots, 8))
            _step(dec, slots, 1)
        else:
            _step(dec, slots, 2)
        torch.cuda.synchronize()
        dec.debug_stage_taps()
        logits = torch.from_numpy(dec.debug_step_logits(True, n))
        toks, cnt = _read(dec, slots, 8)
        # tiles: k_dstep_qkv_up_mt 128 rows (k_dstep_qkv_up: 32), k_dstep_head 32; the last pair of the paired attention and the last 4-row block of the row
        # kernels ride with the last tile's edge (the row kernels and the attention work row by row)
        rows = _sample_rows(n, (128, 32), [n - 2, n - 4])
        n_pos = max(lengths) + (4 if case == "S4" else 2)
        kv = [dec.debug_peek_kv(l, [slots[r] for r in rows], n_pos) for l in range(L)]
        res = dict(taps={k: v.cpu() for k, v in bufs.items()}, logits=logits, toks=toks, cnt=cnt, rows=rows, kv=kv, slots=slots, lengths=lengths, dt=dec.operand_dtype,
                   before=before, limits=limits)
    finally:
        dec.close()
    return res


def _sample_rows(n, tiles, extra):
    """first and last row of every tile (of each size in `tiles`) of the kernels under test, `extra` (first / last row of every prompt, tiles that are not
    aligned to the call's rows), and 16 seeded random rows; everything when n <= 64"""
    if n <= 64:
        return list(range(n))
    rows = set(extra)
    for tile in tiles:
        for t in range(0, n, tile):
            rows.update((t, min(t + tile, n) - 1))
    rows.update(np.random.default_rng(5).choice(n, 16, replace=False).tolist())
    rows = sorted(rows)
    assert len(rows) <= 256
    return rows


class _Report:
    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], (0.0, 0.0, "")

    def stage(self, name, got, ref, emu):
        assert got.shape == ref.shape == emu.shape, (name, got.shape, ref.shape, emu.shape)
        assert bool(torch.isfinite(got).all()), name
        e_max, e_rms, r_max, r_rms = sr.ratios(got.double(), ref, emu)
        print(f"[measured] {self.case} {name}: E_max {e_max:.3e} E_rms {e_rms:.3e}; got - ref = {r_max:.2f} E_max, {r_rms:.2f} E_rms (max |ref| {float(ref.abs().max()):.2f})")
        if r_max > self.worst[0]:
            self.worst = (r_max, r_rms, name)
        if r_max > sr.MAX_X:
            self.bad.append((name, "max", r_max, e_max))
        if r_rms > sr.RMS_X:
            self.bad.append((name, "rms", r_rms, e_rms))
        return e_max

    def fp32(self, name, got, terms, n_add):
        """a sum of fp32 terms: |got - exact| <= n_add 2^-24 sum |terms| per cell, n_add the additions of the kernel.  (Any order of n_add additions meets
        gamma_n_add sum |terms|; the partial sums of the kernel's own order would only tighten it, and the second-order part of gamma is 2^-24 of the bound.)"""
        exact, mag = sum(t.double() for t in terms), sum(t.double().abs() for t in terms)
        ratio = float(((got.double() - exact).abs() / (n_add * EPS32 * mag).clamp_min(1e-300)).max())
        print(f"[measured] {self.case} {name}: worst cell at {ratio:.3f} of the fp32 bound ({n_add} additions)")
        if ratio > 1.0:
            self.bad.append((name, "fp32", ratio, n_add))

    def done(self):
        print(f"[measured] {self.case}: worst stage {self.worst[2]} at {self.worst[0]:.2f} E_max / {self.worst[1]:.2f} E_rms")
        assert not self.bad, self.bad


def _both(fn, sites, dt):
    return fn(dict()), fn(dict(sites=sites, dtype=dt))


def _attr_table(sd):
    """the per (attribute, bin) projection vectors etd_decoder_create folds attribute_projection into: [4, bins, H] float64 (the bias rides on attribute 0)"""
    names = ("pitch_overlap", "polyphony", "note_sustain", "rhythm_intensity")
    W, b = sd["attribute_projection.weight"], sd["attribute_projection.bias"]
    E = W.shape[1] // 4
    return torch.stack([sd[f"{n}_embeddings.weight"] @ W[:, a * E:(a + 1) * E].T + (b if a == 0 else 0) for a, n in enumerate(names)])


@pytest.mark.parametrize("case,weights,force_pair", [("S1", "bench", 0), ("S1", "bench", 1), ("S2", "ctx", -1), ("S3", "bench", -1), ("S4", "bench", -1)],
                         ids=["S1-one-row", "S1-pair", "S2", "S3", "S4-running-rows"])
def test_fused_step_stages(dev, case, weights, force_pair):
    run = _step_run(case, weights, force_pair)
    t, rows, dt, lengths = run["taps"], run["rows"], run["dt"], run["lengths"]
    n = len(lengths)
    sd = {k: v.double() for k, v in sr.state_dict(weights).items()}
    d = neox_dims({})
    rep = _Report(f"{case} pair={force_pair}")
    # a stream ends with the step that emits its limit-th token (begin_bars emits the first): with limit 2 it is finished before the tapped step
    live = torch.tensor([lim > 2 for lim in run["limits"]])
    sel = [i for i, r in enumerate(rows) if live[r]]               # (the cache rows were read for every sampled row)
    rows = [rows[i] for i in sel]
    R = torch.tensor(rows)
    pos = t["step_pos"].long()
    # the tapped step is the second: prompt T, one position per step before it (a stream that finished in the first step stays where it stopped, one past its
    # last row); its rows map to the call's slot list
    assert torch.equal(pos, torch.tensor(lengths) + 1) and t["step_slot"].tolist() == run["slots"]
    n_keys = [sr.key_range(p, CTX) for p in pos[R].tolist()]
    for l in range(L):
        hin, x1, x2 = t["hin"][l][R].double(), t["ln1"][l][R].double(), t["ln2"][l][R].double()
        ref, emu = _both(lambda kw: torch.cat(sr.layer_norms(sd, l, hin, d.layer_norm_eps, **kw), 1), sr.STEP_SITES, dt)
        rep.stage(f"L{l} ln", torch.cat([x1, x2], 1), ref, emu)
        K, Vc = (c[sel].double() for c in run["kv"][l])                              # [rows, heads, n_pos, 64]
        ar = torch.arange(len(rows))
        k_new, v_new = K[ar, :, pos[R]], Vc[ar, :, pos[R]]
        ref, emu = _both(lambda kw: sr.qkv(sd, l, x1, pos[R], NH, **kw), sr.STEP_SITES, dt)
        rep.stage(f"L{l} qkv Q", t["q"][l][R], ref[0], emu[0])
        rep.stage(f"L{l} qkv K append", k_new, ref[1], emu[1])
        rep.stage(f"L{l} qkv V append", v_new, ref[2], emu[2])
        g = t["xcat"][l][R][:, :I].double()
        ref, emu = _both(lambda kw: sr.gelu_up(sd, l, x2, **kw), sr.STEP_SITES, dt)
        rep.stage(f"L{l} up GELU", g, ref, emu)
        q = t["q"][l][R].double()
        ref, emu = _both(lambda kw: sr.dense_slabs(sd, l, sr.attention(q, K, Vc, n_keys, **kw), NH, **kw), sr.STEP_SITES, dt)
        slabs = t["slabs"][l].reshape(-1)[:12 * n * H].reshape(12, n, H)
        rep.stage(f"L{l} attn dense slabs", slabs[4:, R], ref, emu)
        ref, emu = _both(lambda kw: sr.down_slabs(sd, l, g, 4, **kw), sr.STEP_SITES, dt)
        rep.stage(f"L{l} down slabs", slabs[:4, R], ref, emu)
        bias = sr.cat_weight(sd, l, hin)[1].float()
        rep.fp32(f"L{l} resid hout", t["hout"][l][R], [s for s in slabs[:, R]] + [bias.expand(len(rows), H), t["hin"][l][R]], 13)      # 14 terms, 13 additions
        if l + 1 < L:
            assert torch.equal(t["hout"][l], t["hin"][l + 1]), f"layer {l + 1} does not read layer {l}'s output"
    # ---- head: logits, token, next step's rows
    hf = t["hout"][L - 1][live].double()
    ref, emu = _both(lambda kw: sr.head_logits(sd, hf, d.layer_norm_eps, **kw), sr.STEP_SITES, dt)
    logits = run["logits"][live]
    e_max = rep.stage("head logits", logits, ref, emu)
    tok = torch.from_numpy(run["toks"][:, 2]).long()[live]
    assert (torch.from_numpy(run["cnt"])[live] == 3).all()
    assert torch.equal(tok, logits.argmax(-1)), "the emitted token is not the argmax of the device's own logits"
    share, clear = sr.near_tie_share(ref, sr.MAX_X * e_max)
    print(f"[measured] {rep.case} head: rows exempt as near-ties {share:.4f}, agreement with the float64 argmax {float((tok == ref.argmax(-1)).double().mean()):.4f}")
    assert share <= sr.TIE_CAP and bool((tok == ref.argmax(-1))[clear].all())
    assert torch.equal(t["next_pos"].long(), pos + live.long())
    tab = _attr_table(sd)
    tg = sr.TGT_ATTRS
    nl = int(live.sum())
    proj = [tab[a, tg[a]].expand(nl, H) for a in range(4)]       # exact entries: the device's are these rounded to fp32 once
    word, clsv = sd["word_embeddings.weight"][tok].float(), sd["class_embeddings.weight"][sr.TGT_CLASS_ID].float().expand(nl, H)
    rep.fp32("head next embedding", t["next_h"][live], [word, clsv] + proj, 9)        # 4 table entries rounded from float64, 3 + 2 additions
    nh = t["next_h"][live].double()
    ref, emu = _both(lambda kw: torch.cat(sr.layer_norms(sd, 0, nh, d.layer_norm_eps, **kw), 1), sr.STEP_SITES, dt)
    rep.stage("head next ln", torch.cat([t["next_ln1"][live].double(), t["next_ln2"][live].double()], 1), ref, emu)
    rep.done()


def test_finished_streams_are_left_alone_by_a_step(dev):
    """S4: 6 rows, two of them finished by the first step (limit 2): the tapped second step changes no byte of their cache rows -- the whole peeked range, which
    reaches 3 rows past their length -- and neither their token counts nor their tokens; the running rows append one K / V row and one token"""
    run = _step_run("S4", "bench", -1)
    (kv0, (tok0, cnt0)), lengths = run["before"], run["lengths"]
    done = [i for i, lim in enumerate(run["limits"]) if lim == 2]
    assert len(done) == 2
    assert run["rows"] == list(range(len(lengths)))
    for i in range(len(lengths)):
        fin = i in done
        assert cnt0[i] == 2 and run["cnt"][i] == (2 if fin else 3), (i, cnt0[i], run["cnt"][i])
        assert np.array_equal(tok0[i, :2], run["toks"][i, :2])
        T = lengths[i]
        for l in range(L):
            for before, after in zip(kv0[l], run["kv"][l]):
                b, a = before[i].view(torch.int16), after[i].view(torch.int16)
                if fin:
                    assert torch.equal(b, a), f"finished row {i}: layer {l} cache bytes changed"
                else:
                    assert torch.equal(b[:, :T + 1], a[:, :T + 1]) and torch.equal(b[:, T + 2:], a[:, T + 2:]), f"row {i}: layer {l} wrote outside position {T + 1}"
                    assert not torch.equal(b[:, T + 1], a[:, T + 1]), f"row {i}: layer {l} appended nothing"


def test_paired_and_one_row_form_tap_the_same_bytes(dev):
    a, b = _step_run("S1", "bench", 0), _step_run("S1", "bench", 1)
    for k in STEP_TAPS:
        if k != "xcat":                                          # (its attention block is stale in the fused step)
            assert torch.equal(a["taps"][k].view(torch.uint8), b["taps"][k].view(torch.uint8)), k
    assert torch.equal(a["taps"]["xcat"][:, :, :I].view(torch.int16), b["taps"]["xcat"][:, :, :I].view(torch.int16))


PREFILL_TAPS = ("hin", "ln1", "ln2", "q", "qb", "xcat", "slabs", "hout")


@functools.lru_cache(maxsize=None)
def _prefill_run(case, weights):
    lengths = sr.case_lengths(case)
    n, M = len(lengths), sum(lengths)
    prompts = sr.prompts(sr.PROMPT_SEED, lengths)
    slots = list(range(n, 0, -1))
    dec = _decoder(weights, max_streams=n + 1, max_prefill_rows=max(M, CTX))
    try:
        bufs = _bufs(dec, PREFILL_TAPS, L + 1, M)
        dec.debug_stage_taps(layer_mask=(1 << L) - 1, rows=M, slab_cap=12, slices=L + 1, **bufs)
        _begin(dec, prompts, slots)
        torch.cuda.synchronize()
        dec.debug_stage_taps()
        logits = torch.from_numpy(dec.debug_bar_logits(n))
        toks, cnt = _read(dec, slots, 8)
        kv = [dec.debug_peek_kv(l, slots, max(lengths)) for l in range(L)]
        res = dict(taps={k: v.cpu() for k, v in bufs.items()}, logits=logits, toks=toks, cnt=cnt, kv=kv, slots=slots, lengths=lengths, dt=dec.operand_dtype)
    finally:
        dec.close()
    return res


@pytest.mark.parametrize("case,weights", [("P1", "bench"), ("P2", "bench"), ("P2", "ctx")], ids=["P1", "P2-bench", "P2-ctx"])
def test_prefill_stages(dev, case, weights):
    run = _prefill_run(case, weights)
    t, dt, lengths = run["taps"], run["dt"], run["lengths"]
    n, M = len(lengths), sum(lengths)
    big = case == "P2"                                             # forward_prefill16 (k_pattn, k_dmlp_fused, last-rows tail); P1: forward_skinny16
    sd = {k: v.double() for k, v in sr.state_dict(weights).items()}
    d = neox_dims({})
    rep = _Report(f"{case} {weights}")
    row0 = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    last = torch.tensor(row0 + np.asarray(lengths) - 1)
    # tiles: k_linear / k_dmlp_fused 128 rows of the call; k_pattn 128 queries RIGHT-ALIGNED to each prompt's end (a one-token first tile where T = 128 k + 1)
    pattn = [r0 + q for r0, T in zip(row0.tolist(), lengths) for e in range(T, 0, -128) for q in (max(e - 128, 0), e - 1)]
    rows = _sample_rows(M, (128,), row0.tolist() + last.tolist() + pattn)
    R = torch.tensor(rows)
    seq_of = np.repeat(np.arange(n), lengths)
    pos_all = torch.tensor(np.concatenate([np.arange(T) for T in lengths]))
    sites = sr.ALL_SITES if big else sr.STEP_SITES

    def layer_stages(l, s, R, seq, pos, tail):
        """the stages of layer l on rows R of slice s (row i: stream seq[i] at position pos[i]); tail / skinny: fp32 Q, k_dattn, split-K slabs + row kernel"""
        ar = torch.arange(len(R))
        K, Vc = (c.double()[seq] for c in run["kv"][l])
        hin, x1, x2 = t["hin"][s][R].double(), t["ln1"][s][R].double(), t["ln2"][s][R].double()
        tag = f"L{l}{' tail' if tail and big else ''}"
        ref, emu = _both(lambda kw: torch.cat(sr.layer_norms(sd, l, hin, d.layer_norm_eps, **kw), 1), sites, dt)
        rep.stage(f"{tag} ln", torch.cat([x1, x2], 1), ref, emu)
        ref, emu = _both(lambda kw: sr.qkv(sd, l, x1, pos, NH, q_site=None if tail else "Qb", **kw), sites, dt)
        qt = (t["q"] if tail else t["qb"])[s][R].double()
        rep.stage(f"{tag} qkv Q", qt, ref[0], emu[0])
        rep.stage(f"{tag} qkv K append", K[ar, :, pos], ref[1], emu[1])
        rep.stage(f"{tag} qkv V append", Vc[ar, :, pos], ref[2], emu[2])
        n_keys = [sr.key_range(p, CTX) for p in pos.tolist()]
        ref, emu = _both(lambda kw: sr.attention(qt, K, Vc, n_keys, p_site=None if tail else "P", **kw), sites, dt)
        attn = t["xcat"][s][R][:, I:].double()
        rep.stage(f"{tag} attn", attn, ref, emu)
        if tail:
            g = t["xcat"][s][R][:, :I].double()
            ref, emu = _both(lambda kw: sr.gelu_up(sd, l, x2, **kw), sites, dt)
            rep.stage(f"{tag} up GELU", g, ref, emu)
            m = n if big else M
            slabs = t["slabs"][s].reshape(-1)[:5 * m * H].reshape(5, m, H)
            ref, emu = _both(lambda kw: sr.down_slabs(sd, l, torch.cat([g, attn], 1), 5, **kw), sites, dt)
            rep.stage(f"{tag} down slabs", slabs[:, R], ref, emu)
            bias = sr.cat_weight(sd, l, hin)[1].float()
            rep.fp32(f"{tag} resid hout", t["hout"][s][R], [x for x in slabs[:, R]] + [bias.expand(len(R), H), t["hin"][s][R]], 6)      # 7 terms, 6 additions
        else:
            ref, emu = _both(lambda kw: sr.mlp_resid(sd, l, x2, attn, hin, **kw), sites, dt)
            rep.stage(f"{tag} mlp hout", t["hout"][s][R], ref, emu)

    for l in range(L):
        if big and l == L - 1:
            # every position's K / V from the big QKV, then the tail on the prompts' last rows: the gather is exact
            hin, x1 = t["hin"][l][R].double(), t["ln1"][l][R].double()
            ref, emu = _both(lambda kw: torch.cat(sr.layer_norms(sd, l, hin, d.layer_norm_eps, **kw), 1), sites, dt)
            rep.stage(f"L{l} ln", torch.cat([x1, t["ln2"][l][R].double()], 1), ref, emu)
            ref, emu = _both(lambda kw: sr.qkv(sd, l, x1, pos_all[R], NH, q_site="Qb", **kw), sites, dt)
            rep.stage(f"L{l} qkv Q", t["qb"][l][R].double(), ref[0], emu[0])
            K, Vc = (c.double()[seq_of[rows]] for c in run["kv"][l])
            ar = torch.arange(len(rows))
            rep.stage(f"L{l} qkv K append", K[ar, :, pos_all[R]], ref[1], emu[1])
            rep.stage(f"L{l} qkv V append", Vc[ar, :, pos_all[R]], ref[2], emu[2])
            assert torch.equal(t["hin"][L][:n], t["hin"][l][last]), "k_gather_rows"
            layer_stages(l, L, torch.arange(n), np.arange(n), pos_all[last], True)
        else:
            layer_stages(l, l, R, seq_of[rows], pos_all[R], not big)
        if l + 1 < L:
            assert torch.equal(t["hout"][l][:M], t["hin"][l + 1][:M]), f"layer {l + 1} does not read layer {l}'s output"
    hf = (t["hout"][L][:n] if big else t["hout"][L - 1][last]).double()
    ref, emu = _both(lambda kw: sr.head_logits(sd, hf, d.layer_norm_eps, **kw), sr.STEP_SITES, dt)
    e_max = rep.stage("head bar logits", run["logits"], ref, emu)
    tok = torch.from_numpy(run["toks"][:, 0]).long()
    assert (run["cnt"] == 1).all()
    assert torch.equal(tok, run["logits"].argmax(-1)), "the emitted token is not the argmax of the device's own logits"
    share, clear = sr.near_tie_share(ref, sr.MAX_X * e_max)
    print(f"[measured] {rep.case} head: rows exempt as near-ties {share:.4f}")
    assert share <= sr.TIE_CAP and bool((tok == ref.argmax(-1))[clear].all())
    rep.done()


def test_taps_are_validated_before_any_launch(dev):
    """a call that does not fit the stated buffer sizes is refused with ETD_EINVAL and leaves the stream state alone; a wrong geometry is refused at registration"""
    from etude_amd import _lib
    dec = _decoder("bench", max_streams=4)
    try:
        prompts = sr.prompts(3, [5, 9, 4])
        _begin(dec, prompts, [2, 0, 1])
        bufs = _bufs(dec, ("hin", "slabs"), L, 2)
        dec.debug_stage_taps(layer_mask=1, rows=2, slab_cap=12, slices=L, **bufs)
        before, _ = _read(dec, [2, 0, 1], 8)
        with pytest.raises(_lib.EtudeHipError):
            _step(dec, [2, 0, 1], 1)                               # 3 rows, buffers of 2
        with pytest.raises(_lib.EtudeHipError):
            _begin(dec, prompts, [2, 0, 1])                        # 18 rows
        with pytest.raises(_lib.EtudeHipError):
            dec.debug_stage_taps(layer_mask=1 << L, rows=4, slab_cap=12, slices=L, **bufs)
        with pytest.raises(_lib.EtudeHipError):
            dec.debug_stage_taps(layer_mask=0b101, rows=2, slab_cap=12, slices=1, **bufs)      # two layers, buffers of one slice
        dec.debug_stage_taps()
        after, cnt = _read(dec, [2, 0, 1], 8)
        assert np.array_equal(before, after) and (cnt == 1).all()
        _step(dec, [2, 0, 1], 1)
        assert (_read(dec, [2, 0, 1], 8)[1] == 2).all()
        assert bool((bufs["hin"].view(torch.uint8) == 0xFF).all()) and bool((bufs["slabs"].view(torch.uint8) == 0xFF).all())
    finally:
        dec.close()


def test_the_tail_slice_of_a_batched_prefill_is_counted(dev):
    """a batched prefill writes its last-rows tail into the slice BEHIND the tapped layers': buffers stated to hold the layers' slices only are refused before any
    launch when the last layer is tapped, and taken when it is not"""
    from etude_amd import _lib
    dec = _decoder("bench", max_streams=3, max_prefill_rows=CTX)
    try:
        prompts = sr.prompts(3, [300, 300])                        # 600 rows: the batched prefill, two prompts: the tail runs
        bufs = _bufs(dec, ("hin",), 2, 600)
        dec.debug_stage_taps(layer_mask=1 << (L - 1), rows=600, slab_cap=12, slices=1, **bufs)
        with pytest.raises(_lib.EtudeHipError):
            _begin(dec, prompts, [2, 1])
        assert bool((bufs["hin"].view(torch.uint8) == 0xFF).all())
        dec.debug_stage_taps(layer_mask=1 << 3, rows=600, slab_cap=12, slices=1, **bufs)
        _begin(dec, prompts, [2, 1])
        torch.cuda.synchronize()
        dec.debug_stage_taps()
        assert bool(torch.isfinite(bufs["hin"][0]).all()) and bool((bufs["hin"][1].view(torch.uint8) == 0xFF).all())
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _p3_run():
    """96 prompts of 513 tokens = 49 248 rows (192 256-token workgroups of k_pqkv and a ragged one of 96): X1b and Qb of layers 0 and 7 through a SPARSE layer
    mask (slices 0 and 1; the tail's slice 2 holds the 96 last rows); only the sampled rows and their streams' cache rows leave the device"""
    lengths = sr.case_lengths("P3")
    n, M = len(lengths), sum(lengths)
    assert M == 49248 and M >= 49152
    prompts = sr.prompts(sr.PROMPT_SEED, lengths)
    slots = list(range(n - 1, -1, -1))
    row0 = np.arange(n) * 513
    wg = [0, 96, 191, 192]                                         # the first, a middle, the last whole and the ragged 256-token workgroup
    edges = [r for g in wg for r in (256 * g, min(256 * g + 256, M) - 1)]
    rng = np.random.default_rng(5)
    rows = sorted(set(edges) | set(row0.tolist()) | set((row0 + 512).tolist()) | set(rng.choice(M, 16, replace=False).tolist()))
    assert len(rows) <= 256
    layers = (0, L - 1)
    dec = _decoder("bench", max_streams=n, max_prefill_rows=M)
    try:
        bufs = _bufs(dec, ("ln1", "qb"), 3, M)
        dec.debug_stage_taps(layer_mask=sum(1 << l for l in layers), rows=M, slab_cap=12, slices=3, **bufs)
        _begin(dec, prompts, slots)
        torch.cuda.synchronize()
        dec.debug_stage_taps()
        R = torch.tensor(rows, device=bufs["ln1"].device)
        taps = {k: v[:2, R].cpu() for k, v in bufs.items()}
        u8 = bufs["ln1"].view(torch.uint8)
        tail = (bool(torch.isfinite(bufs["ln1"][2, :n].float()).all()), bool((u8[2, n:] == 0xFF).all()), bool((bufs["qb"].view(torch.uint8)[2] == 0xFF).all()))
        seq = sorted(set(r // 513 for r in rows))
        kv = [dec.debug_peek_kv(l, [slots[i] for i in seq], 513) for l in layers]
        res = dict(taps=taps, rows=rows, seq=seq, kv=kv, layers=layers, dt=dec.operand_dtype, tail=tail)
    finally:
        dec.close()
    return res


def test_pqkv_stage(dev):
    """P3: the qkv stage of k_pqkv (Qb, and the K / V rows it appends) from the device's own X1b, layers 0 and 7"""
    run = _p3_run()
    t, rows, dt = run["taps"], run["rows"], run["dt"]
    sd = {k: v.double() for k, v in sr.state_dict("bench").items()}
    rep = _Report("P3 bench")
    pos = torch.tensor([r % 513 for r in rows])
    si = torch.tensor([run["seq"].index(r // 513) for r in rows])
    ar = torch.arange(len(rows))
    for s, l in enumerate(run["layers"]):
        x1 = t["ln1"][s].double()
        assert bool(torch.isfinite(x1).all()), f"layer {l}: X1b tap not written (slice {s})"
        ref, emu = _both(lambda kw: sr.qkv(sd, l, x1, pos, NH, q_site="Qb", **kw), sr.ALL_SITES, dt)
        K, Vc = (c.double() for c in run["kv"][s])
        rep.stage(f"L{l} qkv Q", t["qb"][s].double(), ref[0], emu[0])
        rep.stage(f"L{l} qkv K append", K[si, :, pos], ref[1], emu[1])
        rep.stage(f"L{l} qkv V append", Vc[si, :, pos], ref[2], emu[2])
    # the tail's slice is the one behind the two layers': X1b of the 96 last rows and nothing else (the tail keeps its queries in fp32: no Qb)
    assert run["tail"] == (True, True, True), run["tail"]
    rep.done()


def test_single_row_plain_sequence(dev):
    """S5: one prompt of one token runs forward_plain on k_dgemv (16-bit weights, fp32 activations, LayerNorms in the GEMM prologues; sites W and KV only).  No tap
    reaches it, so it is held from the one layer input a test can reconstruct, the embedding: layer 0's appended K / V row by the stage rule, and the logits by the
    same rule over the whole chain (E = the float64 chain with sites W and KV on; a single key, so the attention is V itself)."""
    sites = frozenset(("W", "KV"))
    p = sr.prompts(sr.PROMPT_SEED, sr.case_lengths("S5"))
    dec = _decoder("bench", max_streams=4)
    try:
        _begin(dec, p, [3])
        torch.cuda.synchronize()
        logits = torch.from_numpy(dec.debug_bar_logits(1))
        K, Vc = (c.double() for c in dec.debug_peek_kv(0, [3], 1))
        toks, cnt = _read(dec, [3], 8)
        dt = dec.operand_dtype
    finally:
        dec.close()
    sd = {k: v.double() for k, v in sr.state_dict("bench").items()}
    d = neox_dims({})
    ids, cls, a4 = (torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)) for x in p[0])
    rep = _Report("S5 bench")
    h0 = sr.embed(sd, ids, cls, a4)
    x1 = sr.layer_norms(sd, 0, h0, d.layer_norm_eps)[0]
    ref, emu = _both(lambda kw: sr.qkv(sd, 0, x1, torch.zeros(1, dtype=torch.long), NH, **kw), sites, dt)
    rep.stage("L0 qkv K append", K[:, :, 0], ref[1], emu[1])
    rep.stage("L0 qkv V append", Vc[:, :, 0], ref[2], emu[2])
    ref, emu = _both(lambda kw: sr.forward(sd, d, ids, cls, a4, **kw)[0], sites, dt)
    rep.stage("logits (whole chain)", logits, ref, emu)
    assert cnt[0] == 1 and toks[0, 0] == int(logits[0].argmax())
    rep.done()
