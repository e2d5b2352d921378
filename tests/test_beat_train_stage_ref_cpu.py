"""The per-kernel references of the Beat-Transformer trainer (tests/beat_train_stage_np.py) on their own, in the manner of tests/test_beat_stage_ref_cpu.py: the
checks of tests/test_gpu_beat_train_stages.py run here with the fp32 references in the device's place -- they must pass -- and then with one planted mistake at a time,
on the same inputs and under the same rule: every one must be rejected.  That is the evidence that the GPU file would fail on a subtly wrong kernel.

  last       a pool routes its gradient to the last of equal maxima          pool3_bwd, patch3_bwd
  leak0      the gradient passes a maximum of exactly 0                      pool3_bwd, patch3_bwd, relu_bwd, hmean_bwd, tmean_bwd
  neighbour  a time tap reads t +- 1 across a song boundary                  conv1, patch3, patch3_bwd
  T0         the first song's T for every song                               conv1, patch3, patch3_bwd, skipacc, hmean, dskip, tmean
  drop       the last partial slice (segment, group) is dropped              colsum, slice_sum, conv_wgrad, tmean, ffn_bwd's linear2.bias
  add_first  the first layer's skip is added to tacc, not written            skipacc
  instr2     divided by instr twice                                          skipacc, hmean, tmean_bwd
  swap       ci and kk swapped in the repack                                 repack
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_train_stage_np as S  # noqa: E402


def passes(check, *args):
    rep = S.Report("fp32 reference")
    check(rep, S.RefDevice(), *args)
    rep.done()


def rejected(check, mutant, *args):
    rep = S.Report(f"mutant {mutant}")
    check(rep, S.RefDevice(mutant), *args)
    assert rep.failed, (check.__name__, mutant, args)


@pytest.mark.parametrize("I", S.INSTR)
def test_front_end_references(I):
    for check in (S.check_conv1, S.check_patches_and_pool, S.check_pool3_bwd, S.check_patch3_bwd):
        passes(check, I)
    for m in ("neighbour", "T0"):
        for check in (S.check_conv1, S.check_patches_and_pool, S.check_patch3_bwd):
            rejected(check, m, I)
    for m in ("last", "leak0"):
        for check in (S.check_pool3_bwd, S.check_patch3_bwd):
            rejected(check, m, I)


def test_built_routes_say_what_autograd_says():
    """the routes stated in ROUTES are fp64 autograd's (first maximum; none at a maximum that is not positive)"""
    vals, pos = S.built_triples(len(S.ROUTES) * 3, 0)
    g = S.np32(S.grad_of(S.pool3, [vals[None].transpose(0, 2, 1)], 0, np.ones((1, vals.shape[0])), S.F64))[0].T
    want = np.zeros_like(vals)
    want[np.arange(len(pos))[pos >= 0], pos[pos >= 0]] = 1
    assert np.array_equal(g, want)
    assert set(pos) == {-1, 0, 1, 2}


def test_repack_reference():
    passes(S.check_repack)
    rejected(S.check_repack, "swap")


@pytest.mark.parametrize("M", S.COLSUM_M)
def test_colsum_reference(M):
    passes(S.check_colsum, M)
    if M % S.CS_ROWS:
        rejected(S.check_colsum, "drop", M)


def test_tempo_bias_colsum_reference():
    passes(S.check_colsum_tempo)
    rejected(S.check_colsum_tempo, "drop")


def test_slice_sum_reference():
    passes(S.check_slice_sum)
    rejected(S.check_slice_sum, "drop")


@pytest.mark.parametrize("M,N,K", S.WGRAD_CASES)
def test_conv_wgrad_reference(M, N, K):
    passes(S.check_conv_wgrad, M, N, K)
    if K % S.SEG_ROWS:
        rejected(S.check_conv_wgrad, "drop", M, N, K)


@pytest.mark.parametrize("I", S.INSTR)
def test_means_references(I):
    passes(S.check_skipacc, I)
    passes(S.check_means, I)
    rejected(S.check_skipacc, "add_first", I)
    rejected(S.check_means, "leak0", I)
    rejected(S.check_means, "T0", I)                      # dskip at every instr
    if I > 1:
        for m in ("instr2", "T0"):
            rejected(S.check_skipacc, m, I)
        rejected(S.check_means, "instr2", I)


@pytest.mark.parametrize("I", S.INSTR)
def test_tmean_references(I):
    passes(S.check_tmean, I)
    for m in ("drop", "T0", "leak0") + (("instr2",) if I > 1 else ()):
        rejected(S.check_tmean, m, I)


def test_relu_reference():
    passes(S.check_relu)
    rejected(S.check_relu, "leak0")


@pytest.mark.parametrize("R", S.PIPE_ROWS)
def test_pipeline_references(R):
    for H, act in ((256, 0), (512, 1)):
        passes(S.check_ffn_bwd, R, H, act)
        if R % S.CS_ROWS and R > S.CS_ROWS:
            rejected(S.check_ffn_bwd, "drop", R, H, act)
    passes(S.check_proj_bwd, R)
