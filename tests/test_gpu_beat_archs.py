"""The Beat-Transformer engine at the architectures etd_beat_create accepts beyond the default 5 / 9 / 1024 / 2, as tests/test_gpu_extractor_archs.py does for the
extractor: instr 1 and 8 (k_beat_iattn's lg[8], k_beat_skipacc's and k_beat_head's division), nlayers 1 (no instrument layer), 4 (exactly one), 11 (dilations 512
and 1024: centre tap only), d_hid 256 and 2048, ntoken 1 and 3.  A ragged call of T = 3 and 70 in two chunks (max_rows = 70 instr: the second song alone fills a chunk), checked end to end against beat_np.forward by
tests/test_gpu_beat.py's 1e-4 bar and at every stage by the bounds of tests/test_gpu_beat_stages.py (all layers tapped: the calls are small).

Measured on the MI355X, worst ratio to the bound over the nine architectures:
    c1 0.259  c2 0.201  x3, front bit for bit  c3 0.174  ln1 0.659  qkv 0.228  skip 0.205  x_attn 0.183  tacc 0.555  ln2 0.716  hid 0.224  x_ffn 0.208
    iln1 0.637  iqkv 0.186  iao 0.201  ix_attn 0.196  iln2 0.617  ihid 0.194  ix_ffn 0.203  logits 0.044  part 0.052  tempo 0.011
    end to end against beat_np.forward: at most 0.018 of the 1e-4 bar
"""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_np  # noqa: E402
import beat_stage_check as S  # noqa: E402

pytestmark = pytest.mark.gpu


def max_rows(dims):
    """etd_beat_forward admits a song to a chunk while the chunk's rows stay <= max_rows: with 70 instr the T = 3 song (3 instr rows) is a chunk of its own and the
    T = 70 song (70 instr rows) the second"""
    return S.ARCH_T[1] * dims["instr"]


@pytest.mark.parametrize("name", list(S.ARCHS))
def test_architecture(name):
    dims, sd, feats, mask, front = S.case(name)
    assert sum(S.ARCH_T) * dims["instr"] > max_rows(dims) >= max(S.ARCH_T) * dims["instr"]      # two chunks, neither song over the workspace
    det = S.detector(dims, sd, max_rows(dims))
    t = S.device_taps(det, dims, feats, mask, front)
    assert t["logits"].shape == (sum(S.ARCH_T), dims["ntoken"])
    rep = S.Report(name)
    seen = S.check_call(rep, sd, dims, [f.shape[1] for f in feats], t, mask, front)
    assert set(seen) == S.tapped_stages(dims, mask, front)          # every layer and the front end are tapped: every stage has its input
    S.end_to_end(name, sd, dims, feats, t, beat_np.forward)
    rep.done()
