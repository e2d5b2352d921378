#!/usr/bin/env python3
"""Teacher-forced scoring throughput (EtudeDecoder.score_many / etd_decoder_score) on the configs[1]-shaped song: the 92 condition bars of
tests/golden/clip_full.npz, each attribute tuple's cover = the engine's own greedy output, all 27 tuples scored in one call; both precisions,
max_streams 1 and 64.

    python tools/bench_score.py [--tuples 27] [--precisions fp32,f16] [--streams 1,64] [--reps 2]

Per (precision, max_streams) one JSON line: scored tokens/s and rows/s of the score call (etd_decoder_score on the pre-assembled sequences; best of
--reps), the end-to-end score_many time (prompt assembly included), and a prefill-only pass over the same sequences (etd_decoder_begin_bars, limit 1:
the forward with the LM head on each sequence's last row only) -- score_ms - prefill_ms is what the head on every scored row and the reductions cost."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from etude_amd import _lib, pipeline, synth  # noqa: E402
from etude_amd.decoder import ABI_ATTR_KEYS, EtudeDecoder, EtudeDecoderConfig, IGNORE_INDEX  # noqa: E402


def vocab():
    from etude_amd.vocab import Vocab
    v = Vocab()
    v.token_to_id = synth.vocab_json()["token_to_id"]
    v.id_to_token = [""] * len(v.token_to_id)
    for t, i in v.token_to_id.items():
        v.id_to_token[i] = t
    return v


def clip_bars():
    g = np.load(ROOT / "tests" / "golden" / "clip_full.npz")
    flat, lens = g["bar_ids"].tolist(), g["bar_lens"].tolist()
    bars, p = [], 0
    for n in lens:
        bars.append(flat[p:p + n]); p += n
    return bars


def assemble(cfg, bos, eos, bars, cover, t, limit=512, ratio=0.5):
    """the sequences score_many builds for one job (etd_debug_assemble_scored, bar by bar): list of (ids, cls, attrs4 [4][T], labels)"""
    sc = _lib.SchedCfg(bar_bos_id=bos, bar_eos_id=eos, n_ctx_pairs=cfg.context_num_past_xy_pairs, max_position_embeddings=cfg.max_position_embeddings,
                       max_bar_token_limit=limit, context_overlap_ratio=ratio, max_streams=1, max_prefill_rows=1, steps_per_poll=1)
    ya = np.asarray([t[k] for k in ABI_ATTR_KEYS], np.int32)
    out, hist = [], []
    cap = 4096
    for x, y in zip(bars, cover):
        h = hist[-cfg.context_num_past_xy_pairs:]
        hx = [np.asarray(a, np.int32) for a, _ in h]
        hy = [np.asarray(b, np.int32) for _, b in h]
        hxp = (C.c_void_p * max(len(h), 1))(*[a.ctypes.data for a in hx])
        hyp = (C.c_void_p * max(len(h), 1))(*[a.ctypes.data for a in hy])
        hxn = np.asarray([a.size for a in hx] or [0], np.int32)
        hyn = np.asarray([a.size for a in hy] or [0], np.int32)
        ha = np.ascontiguousarray(np.tile(ya, (max(len(h), 1), 1)))
        xa, yv = np.asarray(x, np.int32), np.asarray(y, np.int32)
        ids, cls, lab, at = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((4, cap), np.int32)
        T = C.c_int()
        _lib.check(_lib.lib().etd_debug_assemble_scored(C.byref(sc), len(h), hxp, hxn.ctypes.data, hyp, hyn.ctypes.data, ha.ctypes.data, xa.ctypes.data,
                                                        xa.size, yv.ctypes.data, yv.size, ya.ctypes.data, ids.ctypes.data, cls.ctypes.data, at.ctypes.data,
                                                        lab.ctypes.data, cap, C.byref(T)), "assemble_scored")
        n = T.value
        if n:
            out.append((ids[:n].copy(), cls[:n].copy(), at[:, :n].copy(), lab[:n].copy()))
        hist.append((x, y))
    return out


def prefill_only(dec, seqs, tgt):
    """every sequence through etd_decoder_begin_bars (limit 1) in passes of <= max_streams sequences and <= max_prefill_rows rows; synchronised"""
    lib = _lib.lib()
    i = 0
    while i < len(seqs):
        k, rows = 0, 0
        while i + k < len(seqs) and k < dec.max_streams and (k == 0 or rows + len(seqs[i + k][0]) <= dec.max_prefill_rows):
            rows += len(seqs[i + k][0]); k += 1
        part = seqs[i:i + k]
        T = np.asarray([len(s[0]) for s in part], np.int32)
        ids = np.concatenate([s[0] for s in part]); cls = np.concatenate([s[1] for s in part])
        a4 = np.ascontiguousarray(np.concatenate([s[2] for s in part], axis=1))
        slots = np.arange(k, dtype=np.int32)
        tg = np.ascontiguousarray(np.tile(tgt, (k, 1)))
        eos = np.full(k, -1, np.int32); lim = np.ones(k, np.int32)
        with torch.cuda.device(dec.device):
            _lib.check(lib.etd_decoder_begin_bars(dec._h, k, slots.ctypes.data, T.ctypes.data, ids.ctypes.data, cls.ctypes.data, a4.ctypes.data,
                                                  tg.ctypes.data, eos.ctypes.data, lim.ctypes.data, dec._stream()), "begin_bars")
        i += k
    dec._ts.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=int, default=27)
    ap.add_argument("--precisions", default="fp32,f16")
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    v = vocab()
    bos, eos = v.get_bar_bos_id(), v.get_bar_eos_id()
    bars = clip_bars()
    tuples = pipeline.attr_grid(a.tuples)
    cfg = EtudeDecoderConfig(**synth.decoder_dims())
    sd = synth.decoder_state_dict(1, {})
    for prec in a.precisions.split(","):
        gen = EtudeDecoder(cfg, sd, "cuda", precision=prec, max_streams=64)
        covers = gen.generate_many([(bars, [t] * len(bars)) for t in tuples], v, temperature=0.0)
        gen.close()
        jobs = [(bars, c, [t] * len(bars)) for c, t in zip(covers, tuples)]
        seqs = [s for c, t in zip(covers, tuples) for s in assemble(cfg, bos, eos, bars, c, t)]
        T = np.asarray([len(s[0]) for s in seqs], np.int32)
        ids = np.concatenate([s[0] for s in seqs]); cls = np.concatenate([s[1] for s in seqs]); lab = np.concatenate([s[3] for s in seqs])
        a4 = np.ascontiguousarray(np.concatenate([s[2] for s in seqs], axis=1))
        tokens, rows = int((lab != IGNORE_INDEX).sum()), int(T.sum())
        for S in (int(s) for s in a.streams.split(",")):
            dec = EtudeDecoder(cfg, sd, "cuda", precision=prec, max_streams=S)
            dec._score(T[:2], ids[:int(T[:2].sum())], cls[:int(T[:2].sum())], a4[:, :int(T[:2].sum())], lab[:int(T[:2].sum())])     # warm-up
            best_score = best_pre = best_many = float("inf")
            for _ in range(a.reps):
                t0 = time.perf_counter(); lp, tok, _h = dec._score(T, ids, cls, a4, lab); best_score = min(best_score, time.perf_counter() - t0)
                t0 = time.perf_counter(); prefill_only(dec, seqs, np.asarray([tuples[0][k] for k in ABI_ATTR_KEYS], np.int32))
                best_pre = min(best_pre, time.perf_counter() - t0)
                t0 = time.perf_counter(); res = dec.score_many(jobs, v); best_many = min(best_many, time.perf_counter() - t0)
            assert int(tok.sum()) == tokens == int(sum(r.bar_tokens.sum() for r in res))
            print(json.dumps(dict(precision=prec, max_streams=S, jobs=len(jobs), sequences=len(seqs), scored_tokens=tokens, rows=rows,
                                  score_ms=round(best_score * 1e3, 1), tokens_per_s=round(tokens / best_score), rows_per_s=round(rows / best_score),
                                  prefill_only_ms=round(best_pre * 1e3, 1), score_over_prefill=round(best_score / best_pre, 3),
                                  score_many_ms=round(best_many * 1e3, 1), mean_logprob_per_token=round(float(lp.sum()) / tokens, 5))), flush=True)
            dec.close()


if __name__ == "__main__":
    main()
