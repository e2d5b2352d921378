"""What tests/test_gpu_beat_stages.py, tests/test_gpu_beat_archs.py and tests/test_beat_stage_ref_cpu.py share besides the float64 reference (tests/beat_stage_ref.py):
the cases, the bounds (the project's existing yardsticks, restated with a pointer), ``Report`` and ``check_call`` (every tapped stage of one call against the reference
ON ITS OWN TAPPED INPUT), and the device side of the GPU tests (``detector``, ``device_taps``, ``end_to_end``)."""
from __future__ import annotations

import numpy as np

from beat_stage_ref import (C2_COLS, INSTR_STAGES, SEG, TIME_STAGES, conv1, conv2_patches, dattn, gemm_mag, gemm_stage, has_instr_layer, head, iattn, instr_params, ln,
                            patch3, pool3, skipacc, song_slices, tempo, tempo_part, time_params)

# ------------------------------------------------------------------------------------------------ bounds
EPS32 = 2.0 ** -24
GEMM_REL = 1e-6               # tests/test_gpu_gemm3.py / test_gpu_gemm3_epilogues.py: |y - ref| <= 1e-6 (sum |x w| + |b| (+ |resid|)) per cell, every epilogue
LN_X = 2.0                    # tests/test_gpu_gemm3_epilogues.py::test_ln_rows_f32: <= 2 x the error of torch's fp32 F.layer_norm, no floor
ATT_MAX_X, ATT_ULP, ATT_RMS_X = 4.0, 4.0, 2.0      # tests/test_gpu_dtw.py's cost rule (4 E32 + 4 ulp); tests/test_gpu_extractor_stages.py's rms factor

R1_T = [1, 2, 5, 37, 129, 140]
R2_T = [1030]
R3_T = [5, 37, 129]
ARCH_T = [3, 70]
ARCHS = {"instr1": dict(instr=1), "instr8": dict(instr=8), "nlayers1": dict(nlayers=1), "nlayers4": dict(nlayers=4), "nlayers11": dict(nlayers=11),
         "dhid256": dict(d_hid=256), "dhid2048": dict(d_hid=2048), "ntoken1": dict(ntoken=1), "ntoken3": dict(ntoken=3)}


def edge_features(seed, T):
    """R3's input edges: stem 0 all -80 (a silent stem after power_to_db), stem 1 all 0, stem 2 at the inclusive bound +80, stems 3 and 4 ordinary"""
    from etude_amd import synth
    f = synth.beat_features(seed, T)
    f[0], f[1], f[2] = -80.0, 0.0, 80.0
    return f


def att_bounds(ref, f32):
    """(max bound, rms bound) of an attention stage: 4 E32 + 4 ulp at the largest output; 2 rms(E32) + the same floor"""
    e = np.asarray(f32, np.float64) - ref
    floor = ATT_ULP * float(np.spacing(np.float32(np.abs(ref).max())))
    return ATT_MAX_X * float(np.abs(e).max()) + floor, ATT_RMS_X * float(np.sqrt((e ** 2).mean())) + floor


def sum_n(stage, I=0, nseg=0):
    """additions (roundings) per output cell of the fixed-order fp32 sums, read off the kernels: conv1 15 fmaf + the bias start, through max and ReLU (1-Lipschitz);
    skipacc I - 1 additions, the division, the accumulation; head: the mean (I - 1, division), one product, 3 fmaf, 6 butterfly stages, the bias; tempo_part a chain of
    <= 128 frames; tempo: nseg - 1 additions, the division, a chain of 256 fmaf, the bias"""
    return {"c1": 16, "tacc": I + 1, "logits": I + 11, "part": SEG - 1, "tempo": nseg + 257}[stage]


def case(name):
    """(dims, state dict, [features per song], layer mask, front-end taps?) of a case of the GPU test"""
    from etude_amd import synth
    if name in ARCHS:
        dims = synth.beat_dims(**ARCHS[name])
        feats = [synth.beat_features(700 + i, T, instr=dims["instr"]) for i, T in enumerate(ARCH_T)]
        return dims, synth.beat_state_dict(7, dims), feats, (1 << dims["nlayers"]) - 1, True
    dims = synth.beat_dims()
    if name == "R1":
        return dims, synth.beat_state_dict(7), [synth.beat_features(600 + i, T) for i, T in enumerate(R1_T)], 0x1FF, True
    if name == "R2":
        return dims, synth.beat_state_dict(7), [synth.beat_features(650, R2_T[0])], (1 << 0) | (1 << 7) | (1 << 8), False
    if name == "R3":
        return dims, synth.beat_state_dict(8), [edge_features(660 + i, T) for i, T in enumerate(R3_T)], 0x1FF, True
    raise KeyError(name)


def tapped_stages(dims, mask, front):
    """the names of everything a call with this layer mask taps (``chain``'s names), the call's outputs included"""
    L = dims["nlayers"]
    return {f"{s}.{l}" for l in range(L) if (mask >> l) & 1 for s in TIME_STAGES + (INSTR_STAGES if has_instr_layer(l, L) else ())} | \
        {"logits", "part", "tempo"} | ({"c1", "c2", "x3", "c3", "front"} if front else set())


# ------------------------------------------------------------------------------------------------ the checker
class Report:
    """collects every stage's measured ratio to its bound; prints them as [measured]; `done` asserts that none is above 1"""

    def __init__(self, case):
        self.case, self.bad, self.worst, self.checked = case, [], {}, []

    def add(self, stage, ratio, note=""):
        key = stage.split(".")[0]
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)
        self.checked.append(stage)
        print(f"[measured] {self.case} {stage}: {ratio:.3f} of its bound {note}")
        if not ratio <= 1.0:
            self.bad.append((stage, ratio))

    def cells(self, stage, got, ref, bound, note=""):
        """per-cell bound"""
        assert got.shape == ref.shape == bound.shape, (stage, got.shape, ref.shape, bound.shape)
        assert np.isfinite(got).all(), stage
        self.add(stage, float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max()), note)

    def exact(self, stage, got, ref):
        assert got.shape == ref.shape, (stage, got.shape, ref.shape)
        same = np.array_equal(got, ref)
        self.checked.append(stage)
        print(f"[measured] {self.case} {stage}: bit for bit {'yes' if same else 'NO'}")
        self.worst[stage.split(".")[0]] = max(self.worst.get(stage.split(".")[0], 0.0), 0.0 if same else np.inf)
        if not same:
            self.bad.append((stage, "bits"))

    def attention(self, stage, got, ref, f32):
        assert got.shape == ref.shape == f32.shape and np.isfinite(got).all(), stage
        bmax, brms = att_bounds(ref, f32)
        d = got.astype(np.float64) - ref
        self.add(stage, float(np.abs(d).max()) / bmax, "(max)")
        self.add(stage, float(np.sqrt((d ** 2).mean())) / brms, "(rms)")

    def layernorm(self, stage, got, x, g, b):
        ref = ln(x, g, b)
        e32 = float(np.abs(ln(x, g, b, np.float32) - ref).max())
        self.add(stage, float(np.abs(got.astype(np.float64) - ref).max()) / (LN_X * e32), f"(fp32 LayerNorm's own error {e32:.2e})")

    def gemm(self, sd, stage, l, got, x, resid=None):
        name = stage if l is None else f"{stage}.{l}"
        self.cells(name, got, gemm_stage(sd, stage, l, x, resid), GEMM_REL * gemm_mag(sd, stage, l, x, resid))

    def done(self):
        print(f"[measured] {self.case} worst per stage: " + ", ".join(f"{k} {v:.3f}" for k, v in self.worst.items()))
        assert not self.bad, self.bad



def check_call(rep, sd, dims, Ts, t, mask, front=True):
    """Every tapped stage of one call against float64 ON ITS OWN TAPPED INPUT.  t: the call's taps by the names of ``chain`` (whole-call arrays in the global row /
    frame / segment order, `c2` as [R][>= 31][64] per row, `feat` the songs' features, `logits`, `tempo` the call's outputs).  A stage whose input was not tapped (a
    sparse layer mask, no front-end taps) cannot be compared: it is printed as such.  Returns the names of the stages that WERE compared (``Report.checked``: a name
    gets there only through a comparison)."""
    I, L = dims["instr"], dims["nlayers"]
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    songs = list(song_slices(Ts, I))
    f64 = lambda a: np.asarray(a, np.float64)
    per_rows = lambda fn, *arrs: np.concatenate([fn(*[a[rs] for a in arrs], T) for rs, _, T in songs])
    n0 = len(rep.checked)
    if front:
        pairs = [conv1(sd, f, mag=True) for f in t["feat"]]
        rep.cells("c1", t["c1"], np.concatenate([p[0] for p in pairs]), sum_n("c1") * EPS32 * np.concatenate([p[1] for p in pairs]))
        x2 = conv2_patches(t["c1"])
        R = t["c1"].shape[0]
        rep.cells("c2", t["c2"].reshape(R, -1, 64)[:, :C2_COLS].reshape(R * C2_COLS, 64), gemm_stage(sd, "c2", None, x2), GEMM_REL * gemm_mag(sd, "c2", None, x2))
        rep.exact("x3", t["x3"], per_rows(lambda c2, T: patch3(c2.reshape(I * T, -1, 64), I, T), t["c2"].reshape(R, -1)))
        rep.gemm(sd, "c3", None, t["c3"], t["x3"])
        rep.exact("front", t["front"], pool3(t["c3"]))
    x_in = t["front"] if front else None
    tacc_in = None
    for l in range(L):
        on = (mask >> l) & 1
        if not on:
            x_in = tacc_in = None
            continue
        p = time_params(sd, l)
        if x_in is not None:
            rep.layernorm(f"ln1.{l}", t[f"ln1.{l}"], x_in, p["norm1.weight"], p["norm1.bias"])
        rep.gemm(sd, "qkv", l, t[f"qkv.{l}"], t[f"ln1.{l}"])
        q = t[f"qkv.{l}"]
        s64, s32 = (per_rows(lambda a, T: dattn(p, a, I, T, l, dt), q) for dt in (np.float64, np.float32))
        rep.attention(f"skip.{l}", t[f"skip.{l}"], s64, s32)
        if x_in is not None:
            rep.attention(f"x_attn.{l}", t[f"x_attn.{l}"], f64(x_in) + s64, x_in.astype(np.float32) + s32)
        if l == 0 or tacc_in is not None:
            prs = [skipacc(t[f"skip.{l}"][rs], None if l == 0 else tacc_in[fs], I, T, mag=True) for rs, fs, T in songs]
            rep.cells(f"tacc.{l}", t[f"tacc.{l}"], np.concatenate([a for a, _ in prs]), sum_n("tacc", I) * EPS32 * np.concatenate([m for _, m in prs]))
        x = t[f"x_attn.{l}"]
        rep.layernorm(f"ln2.{l}", t[f"ln2.{l}"], x, p["norm2.weight"], p["norm2.bias"])
        rep.gemm(sd, "hid", l, t[f"hid.{l}"], t[f"ln2.{l}"])
        rep.gemm(sd, "x_ffn", l, t[f"x_ffn.{l}"], t[f"hid.{l}"], resid=x)
        x_in, tacc_in = t[f"x_ffn.{l}"], t[f"tacc.{l}"]
        if has_instr_layer(l, L):
            qi = instr_params(sd, l)
            rep.layernorm(f"iln1.{l}", t[f"iln1.{l}"], x_in, qi["norm1.weight"], qi["norm1.bias"])
            rep.gemm(sd, "iqkv", l, t[f"iqkv.{l}"], t[f"iln1.{l}"])
            a64, a32 = (per_rows(lambda a, T: iattn(a, I, T, dt), t[f"iqkv.{l}"]) for dt in (np.float64, np.float32))
            rep.attention(f"iao.{l}", t[f"iao.{l}"], a64, a32)
            rep.gemm(sd, "ix_attn", l, t[f"ix_attn.{l}"], t[f"iao.{l}"], resid=x_in)
            rep.layernorm(f"iln2.{l}", t[f"iln2.{l}"], t[f"ix_attn.{l}"], qi["norm2.weight"], qi["norm2.bias"])
            rep.gemm(sd, "ihid", l, t[f"ihid.{l}"], t[f"iln2.{l}"])
            rep.gemm(sd, "ix_ffn", l, t[f"ix_ffn.{l}"], t[f"ihid.{l}"], resid=t[f"ix_attn.{l}"])
            x_in = t[f"ix_ffn.{l}"]
    if x_in is not None:                      # the last layer was tapped: the heads
        prs = [head(sd, x_in[rs], I, T, mag=True) for rs, _, T in songs]
        rep.cells("logits", t["logits"], np.concatenate([a for a, _ in prs]), sum_n("logits", I) * EPS32 * np.concatenate([m for _, m in prs]))
        ref = np.concatenate([tempo_part(tacc_in[fs], T) for _, fs, T in songs])
        rep.cells("part", t["part"], ref, sum_n("part") * EPS32 * ref)
        g0, outs = 0, []
        for i, (_, _, T) in enumerate(songs):
            ns = -(-T // SEG)
            o, m = tempo(sd, t["part"][g0:g0 + ns], T, mag=True)
            outs.append((o, sum_n("tempo", nseg=ns) * EPS32 * m))
            g0 += ns
        rep.cells("tempo", t["tempo"], np.stack([o for o, _ in outs]), np.stack([b for _, b in outs]))
    seen = sorted(set(rep.checked[n0:]))
    left = sorted(tapped_stages(dims, mask, front) - set(seen))
    if left:
        print(f"[measured] {rep.case} tapped but not comparable (the stage's input was not tapped): " + ", ".join(left))
    return seen


# ------------------------------------------------------------------------------------------------ the device side (GPU tests only)
def detector(dims, sd, max_rows, tracker="madmom"):
    from etude_amd import BeatDetector
    from etude_amd.config import BeatDetectorConfig, BeatDetectorModelConfig
    cfg = BeatDetectorConfig()
    cfg.model = BeatDetectorModelConfig(**dims)
    return BeatDetector(cfg, state_dict=sd, max_rows=max_rows, tracker=tracker)


def device_taps(det, dims, feats, mask, front):
    """one ragged call with taps off, then the same call with every tap of `mask` on: asserts that logits and tempo are bit-identical (taps are pure copies) and
    returns the taps under ``chain``'s names (host float32 arrays; buffers are pre-filled with NaN patterns, so a tap that was not written cannot pass)"""
    import torch
    I, L, H = dims["instr"], dims["nlayers"], dims["d_hid"]
    Ts = [f.shape[1] for f in feats]
    rows, frames, segs = I * sum(Ts), sum(Ts), sum(-(-T // SEG) for T in Ts)
    packed = torch.cat([torch.from_numpy(np.ascontiguousarray(f)).reshape(-1) for f in feats]).cuda()
    lg0, tp0 = det._run(packed, Ts)
    torch.cuda.synchronize()
    layers = [l for l in range(L) if (mask >> l) & 1]
    ilayers = [l for l in layers if has_instr_layer(l, L)]
    width = dict(c1=42 * 32, c2=42 * 64, x3=3 * 1152, c3=3 * 256, front=256, qkv=768, iqkv=768, hid=H, ihid=H)
    bufs = {}
    for k in (("c1", "c2", "x3", "c3", "front") if front else ()) + TIME_STAGES + (INSTR_STAGES if ilayers else ()) + ("part",):
        n_sl = 1 if k in width and k not in ("qkv", "iqkv", "hid", "ihid") or k == "part" else len(ilayers) if k in INSTR_STAGES else len(layers)
        per = frames if k == "tacc" else segs if k == "part" else rows
        bufs[k] = torch.empty((n_sl, per, width.get(k, 256)), dtype=torch.float32, device="cuda")
        bufs[k].view(torch.uint8).fill_(0xFF)
    det.debug_stage_taps(layer_mask=mask, rows=rows, frames=frames, segs=segs, slices=len(layers), islices=len(ilayers), **bufs)
    try:
        lg1, tp1 = det._run(packed, Ts)
        torch.cuda.synchronize()
    finally:
        det.debug_stage_taps()
    assert torch.equal(lg0, lg1) and torch.equal(tp0, tp1), "logits / tempo differ between taps on and taps off"
    t = dict(feat=feats, logits=lg1.cpu().numpy(), tempo=tp1.cpu().numpy(), part=bufs["part"][0].cpu().numpy())
    if front:
        t.update({k: bufs[k][0].cpu().numpy() for k in ("c1", "c2", "x3", "c3", "front")})
        t["c1"], t["c2"] = t["c1"].reshape(rows, 42, 32), t["c2"].reshape(rows, 42, 64)
        t["x3"], t["c3"] = t["x3"].reshape(rows * 3, 1152), t["c3"].reshape(rows * 3, 256)
    for s, l in enumerate(layers):
        t.update({f"{k}.{l}": bufs[k][s].cpu().numpy() for k in TIME_STAGES})
    for s, l in enumerate(ilayers):
        t.update({f"{k}.{l}": bufs[k][s].cpu().numpy() for k in INSTR_STAGES})
    for k, v in t.items():
        if k != "feat":
            assert np.isfinite(v).all(), f"tap {k} was not (wholly) written"
    return t


def end_to_end(name, sd, dims, feats, t, forward):
    """the call's logits and tempo against `forward` (beat_np.forward) per song, by tests/test_gpu_beat.py's bar 1e-4 max(1, max |ref|): printed and asserted"""
    f0 = 0
    for i, f in enumerate(feats):
        T = f.shape[1]
        r = forward(sd, f, nlayers=dims["nlayers"])
        for what, got, ref in (("logits", t["logits"][f0:f0 + T], r["logits"]), ("tempo", t["tempo"][i], r["tempo"])):
            err, bar = float(np.abs(got.astype(np.float64) - ref).max()), 1e-4 * max(1.0, float(np.abs(ref).max()))
            print(f"[measured] {name} song {i} (T = {T}) end to end {what}: max |d| {err:.3e} = {err / bar:.4f} of the 1e-4 bar")
            assert err <= bar, (name, i, what, err, bar)
        f0 += T