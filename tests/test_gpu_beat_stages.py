"""Every launch of the Beat-Transformer engine (csrc/beat.hip: run_chunk) against float64 ON ITS OWN TAPPED INPUT, as tests/test_gpu_extractor_stages.py and
tests/test_gpu_decoder_stages.py do for the other engines.

etd_beat_debug_stage_taps copies each launch's output out of the shared workspace; stage k's float64 reference (tests/beat_stage_ref.py, pinned to the reference
goldens through tests/beat_np.py by tests/test_beat_cpu.py and to its own mutants by tests/test_beat_stage_ref_cpu.py) is computed from the device's tap of stage
k - 1.  The engine has no 16-bit rounding site, so the bounds are the project's fp32 yardsticks (constants, cases and the checker in tests/beat_stage_check.py):
    k_gemm3 stages      per cell 1e-6 (sum |x w| + |b| (+ |resid|)), every epilogue (tests/test_gpu_gemm3.py, test_gpu_gemm3_epilogues.py); conv2 on columns 0 .. 30
    LayerNorm rows      2 x the error of torch's fp32 F.layer_norm on the same rows (test_gpu_gemm3_epilogues.py::test_ln_rows_f32)
    patch3, pool3       bit for bit
    fp32 sums           per cell n 2^-24 sum |terms| (conv1 n = 16, skipacc instr + 1, head instr + 11, tempo_part 127, tempo segments + 257)
    skip, x_attn, iao   max <= 4 E32 + 4 ulp at the largest output, rms <= 2 rms(E32) + the same floor; E32 from the float32 stage function on the same tap
Cases: R1 ragged T = 1, 2, 5, 37, 129, 140 in three chunks, every tap, all 9 layers; R2 one song of T = 1030 (far taps of dilations 128 and 256, 9 tempo segments),
layers 0, 7, 8; R3 T = 5, 37, 129 with a second weight seed and a stem each at -80, 0 and the inclusive bound +80.  Taps are pure copies: logits and tempo are
bit-identical with taps on and off (asserted for every case).  Every ratio is printed ([measured], pytest -s).  R2 taps layers 0, 7 and 8 and no front end, so
five of its tapped stages have no tapped input and cannot be compared (NOT_COMPARABLE below says which); every other tapped stage of every case must have been.
R3's edge inputs also go through every public entry point (forward, activations, activations_many, detect_many), which check the range the private ``_run`` does not.

Measured on the MI355X, worst ratio to the bound per stage over R1, R2, R3:
    c1 0.231  c2 0.188  x3, front bit for bit  c3 0.198  ln1 0.640  qkv 0.240  skip 0.196  x_attn 0.153  tacc 0.628  ln2 0.664  hid 0.232  x_ffn 0.217
    iln1 0.588  iqkv 0.211  iao 0.184  ix_attn 0.177  iln2 0.567  ihid 0.233  ix_ffn 0.252  logits 0.034  part 0.079  tempo 0.012
    end to end against beat_np.forward: logits <= 4.2e-6, tempo <= 1.2e-6, at most 0.022 of tests/test_gpu_beat.py's 1e-4 bar
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_np  # noqa: E402
import beat_stage_check as S  # noqa: E402

from etude_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_ROWS = 700           # R1: chunks of 225, 645 and 700 rows, each boundary between two songs; R2's one song exceeds it and gets a workspace of its own


# R2 (layers 0, 7, 8; no front-end taps): ln1.l and x_attn.l = x + skip read the token rows x ENTERING layer l, and tacc.l adds to tacc.(l - 1).  Layer 0's x is the
# untapped front end; layer 7's x and tacc.6 belong to the untapped layer 6.  (tacc.0 has no predecessor, and layer 8 reads layer 7's taps: both are compared.)  What
# R2 is there for, the far taps of dilations 128 and 256, is in skip.7 and skip.8; R1 and R3 compare these five stages at every layer.
NOT_COMPARABLE = {"R1": set(), "R2": {"ln1.0", "x_attn.0", "ln1.7", "x_attn.7", "tacc.7"}, "R3": set()}


@pytest.mark.parametrize("name", ["R1", "R2", "R3"])
def test_stages(name):
    dims, sd, feats, mask, front = S.case(name)
    det = S.detector(dims, sd, MAX_ROWS)
    t = S.device_taps(det, dims, feats, mask, front)
    rep = S.Report(name)
    seen = S.check_call(rep, sd, dims, [f.shape[1] for f in feats], t, mask, front)
    assert set(seen) == S.tapped_stages(dims, mask, front) - NOT_COMPARABLE[name]          # `seen` holds only what was compared
    S.end_to_end(name, sd, dims, feats, t, beat_np.forward)
    rep.done()


def test_every_entry_point_accepts_the_input_edges():
    """R3's stems at -80, 0 and the inclusive bound +80 through every public entry point: none raises, and each returns bit for bit what the unchecked ``_run``
    gives for the same call; one float32 step above the bound every one of them raises ValueError"""
    dims, sd, feats, _, _ = S.case("R3")
    assert all(float(f[0].max()) == -80.0 and not f[1].any() and float(f[2].min()) == 80.0 for f in feats)
    det = S.detector(dims, sd, MAX_ROWS, tracker="native")
    pack = lambda fs: torch.cat([torch.from_numpy(np.ascontiguousarray(f)).reshape(-1) for f in fs]).cuda()
    Ts = [f.shape[1] for f in feats]
    for f, T in zip(feats, Ts):
        lg, tp = det._run(pack([f]), [T])
        lg_f, tp_f = det.forward(torch.from_numpy(f)[None])
        assert torch.equal(lg_f[0], lg) and torch.equal(tp_f, tp), T
        act = torch.sigmoid(lg).cpu().numpy()
        beat, down = det.activations(f)
        assert np.array_equal(beat, act[:, 0]) and np.array_equal(down, act[:, 1]), T
    lg, _ = det._run(pack(feats), Ts)
    act, o = torch.sigmoid(lg).cpu().numpy(), 0
    for (beat, down), T in zip(det.activations_many(feats), Ts):
        assert np.array_equal(beat, act[o:o + T, 0]) and np.array_equal(down, act[o:o + T, 1]), T
        o += T
    tracked = det.detect_many(feats)                                 # native trackers on the same logits; the logits themselves stay on the device
    assert tracked == det._detect_packed(pack(feats), Ts) and len(tracked) == len(feats)
    over = [f.copy() for f in feats]
    over[1][2, 17, 5] = np.nextafter(np.float32(80.0), np.float32(np.inf))
    for call in (lambda: det.forward(torch.from_numpy(over[1])[None]), lambda: det.activations(over[1]), lambda: det.activations_many(over), lambda: det.detect_many(over)):
        with pytest.raises(ValueError):
            call()


def test_taps_are_validated_before_any_launch():
    """a call larger than the stated buffers is ETD_EINVAL before anything is launched; a wrong geometry is refused at registration"""
    dims, sd, feats, _, _ = S.case("R3")
    det = S.detector(dims, sd, MAX_ROWS)
    buf = torch.empty((1, 25, 256), device="cuda")
    buf.view(torch.uint8).fill_(0xFF)
    det.debug_stage_taps(layer_mask=1, rows=25, frames=5, segs=1, slices=1, islices=0, ln1=buf)
    try:
        with pytest.raises(_lib.EtudeHipError):
            det.activations(feats[1])                              # 185 rows, buffers of 25
        assert bool((buf.view(torch.uint8) == 0xFF).all())
        with pytest.raises(_lib.EtudeHipError):
            det.debug_stage_taps(layer_mask=1 << 9, rows=25, frames=5, segs=1, slices=1, islices=0, ln1=buf)
        with pytest.raises(_lib.EtudeHipError):
            det.debug_stage_taps(layer_mask=0b11, rows=25, frames=5, segs=1, slices=1, islices=0, ln1=buf)
        with pytest.raises(ValueError):
            det.debug_stage_taps(layer_mask=0b11, rows=25, frames=5, segs=1, slices=2, islices=0, ln1=buf)      # the tensor holds one slice
        det.debug_stage_taps(layer_mask=1, rows=25, frames=5, segs=1, slices=1, islices=0, ln1=buf)
        det.activations(feats[0])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(buf).all())
    finally:
        det.debug_stage_taps()
