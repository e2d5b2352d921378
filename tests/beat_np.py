"""A plain-numpy restatement of Demixed_DilatedTransformerModel.forward for ONE song (tests only), written from the model's description: conv front end, dilated
5-tap attention with its head / offset table and head 7's key quirk, instrument attention after layers 3-5, beat and tempo heads.  fp64 throughout.  It is the
composition of the per-stage functions of tests/beat_stage_ref.py (one per launch of the engine, in the device's row layout).

forward(sd, feat[instr][T][128], nlayers=9) -> dict(logits [T][ntoken], tempo [300], front [instr][T][D], layer0 [instr][T][D])
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import beat_stage_ref as S  # noqa: E402

OFFSETS = S.OFFSETS


def forward(sd, feat, nlayers: int = 9):
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    feat = np.asarray(feat)
    I, T, _ = feat.shape
    x = S.pool3(S.conv3(sd, S.patch3(S.conv2(sd, S.conv1(sd, feat)), I, T)))
    res = {"front": x.reshape(I, T, -1).copy()}
    tacc = None
    for l in range(nlayers):
        p = S.time_params(sd, l)
        skip = S.dattn(p, S.gemm_stage(sd, "qkv", l, S.ln(x, p["norm1.weight"], p["norm1.bias"])), I, T, l)
        x = x + skip
        tacc = S.skipacc(skip, tacc, I, T)
        x = S.gemm_stage(sd, "x_ffn", l, S.gemm_stage(sd, "hid", l, S.ln(x, p["norm2.weight"], p["norm2.bias"])), resid=x)
        if l == 0:
            res["layer0"] = x.reshape(I, T, -1).copy()
        if S.has_instr_layer(l, nlayers):
            q = S.instr_params(sd, l)
            x = S.gemm_stage(sd, "ix_attn", l, S.iattn(S.gemm_stage(sd, "iqkv", l, S.ln(x, q["norm1.weight"], q["norm1.bias"])), I, T), resid=x)
            x = S.gemm_stage(sd, "ix_ffn", l, S.gemm_stage(sd, "ihid", l, S.ln(x, q["norm2.weight"], q["norm2.bias"])), resid=x)
    res["logits"] = S.head(sd, x, I, T)
    res["tempo"] = S.tempo(sd, S.tempo_part(tacc, T), T)
    return res
