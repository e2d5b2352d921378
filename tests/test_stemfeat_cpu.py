"""Stem mel-dB features, the parts that need no GPU: the C ABI's host entry points, the mel filterbank, and self-checks of the fp64 restatement (tests/stemfeat_np.py)
that the GPU tests take as their oracle."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import stemfeat_np as sn  # noqa: E402

from etude_amd import _lib  # noqa: E402

NS = (1, 1023, 1024, 1025, 4095, 4096, 4097)


def test_symbols_exported():
    lib = _lib.lib()
    for name in ("etd_stemfeat_create", "etd_stemfeat_destroy", "etd_stemfeat_num_frames", "etd_stemfeat_workspace_bytes", "etd_stemfeat_run"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.etd_version() == 3


@pytest.mark.parametrize("framing", sn.FRAMINGS)
def test_num_frames_is_the_formula(framing):
    from etude_amd.stemfeat import StemFeatures
    for n_fft, hop in ((4096, 1024), (256, 64)):
        sf = StemFeatures(n_fft=n_fft, hop=hop, n_mels=32 if n_fft == 256 else 128, framing=framing)
        lead = n_fft if framing == "spleeter" else n_fft // 2
        for N in NS:
            want = 1 + (N + 2 * lead - n_fft) // hop
            assert sf.num_frames(N) == want == sn.num_frames(N, n_fft, hop, framing), (framing, N)
    sf = StemFeatures(framing="librosa")
    assert [sf.num_frames(N) for N in NS] == [1 + N // 1024 for N in NS]
    with pytest.raises(ValueError):
        sf.num_frames(0)


def test_workspace_bytes_host_only():
    from etude_amd.stemfeat import StemFeatures
    sf = StemFeatures()
    one = sf.workspace_bytes([1024 * 40 + 517], 5)
    assert 0 < one < 4096
    assert sf.workspace_bytes([1024 * 600 + 1] * 3, 5) > 3 * 5 * 150 * 4
    with pytest.raises(_lib.EtudeHipError):
        sf.workspace_bytes([0], 5)


def test_filterbank_equals_restatement_and_has_the_stated_structure():
    from etude_amd import mel_filterbank
    fb = mel_filterbank(44100, 4096, 128, 30, 11000)
    ref = sn.mel_filterbank(44100, 4096, 128, 30, 11000)
    assert fb.dtype == np.float32 and fb.shape == (128, 2049)
    assert np.array_equal(fb, ref)
    nz = fb != 0
    assert int(nz.sum()) == 2009
    assert int(nz.sum(1).max()) == 52
    cols = np.flatnonzero(nz.any(0))
    assert (int(cols[0]), int(cols[-1])) == (3, 1021)
    assert (fb >= 0).all() and nz.any(1).all()
    small = mel_filterbank(44100, 256, 32, 30, 11000)
    assert np.array_equal(small, sn.mel_filterbank(44100, 256, 32, 30, 11000))


def test_slaney_scale():
    assert float(sn.hz_to_mel(1000.0)) == 15.0
    assert float(sn.hz_to_mel(200.0 / 3.0)) == 1.0
    assert abs(float(sn.hz_to_mel(6400.0)) - 42.0) < 1e-12
    f = np.array([30.0, 500.0, 1000.0, 4000.0, 11000.0])
    assert np.allclose(sn.mel_to_hz(sn.hz_to_mel(f)), f, rtol=1e-13)
    from etude_amd import stemfeat
    assert stemfeat._hz_to_mel(1000.0) == 15.0


def test_create_refuses_bad_tables_and_configs():
    from etude_amd.stemfeat import StemFeatures, _csr, mel_filterbank
    with pytest.raises(ValueError, match="power of two"):
        StemFeatures(n_fft=3000)
    with pytest.raises(ValueError, match="power of two"):
        StemFeatures(n_fft=8192)
    with pytest.raises(ValueError, match="framing"):
        StemFeatures(framing="torch")
    lib = _lib.lib()
    start, length, w = _csr(mel_filterbank())
    win = np.ones(4096, np.float32)

    def create(cfg, win=win, start=start, length=length, w=w):
        h = C.c_void_p()
        rc = lib.etd_stemfeat_create(C.byref(cfg), win.ctypes.data, start.ctypes.data, length.ctypes.data, w.ctypes.data, C.byref(h))
        if rc == 0:
            lib.etd_stemfeat_destroy(h)
        return rc, (lib.etd_last_error() or b"").decode()
    good = dict(n_fft=4096, hop=1024, n_mels=128, framing=0, amin=1e-10, top_db=80.0)
    assert create(_lib.StemFeatCfg(**good))[0] == 0
    rc, msg = create(_lib.StemFeatCfg(**{**good, "n_fft": 3000}))
    assert rc == -22 and "power of two" in msg
    rc, msg = create(_lib.StemFeatCfg(**{**good, "framing": 3}))
    assert rc == -22 and "framing" in msg
    bad = start.copy(); bad[127] = 2049
    rc, msg = create(_lib.StemFeatCfg(**good), start=bad)
    assert rc == -22 and "band 127" in msg
    bad = w.copy(); bad[5] = np.nan
    rc, msg = create(_lib.StemFeatCfg(**good), w=bad)
    assert rc == -22 and "non-finite" in msg
    bad = w.copy(); bad[5] = -1.0
    assert create(_lib.StemFeatCfg(**good), w=bad)[0] == -22
    cfg = _lib.StemFeatCfg(**good); cfg.struct_bytes = 4
    assert create(cfg)[0] == -22


def test_shape_refusals_need_no_gpu():
    from etude_amd.pipeline import ClipBatchPipeline
    from etude_amd.stemfeat import StemFeatures
    sf = StemFeatures()
    with pytest.raises(ValueError, match=r"\[instr\]\[channels\]\[N\]"):
        sf.features_many([np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="N >= 1"):
        sf.features_many([np.zeros((5, 2, 0), np.float32)])
    with pytest.raises(ValueError, match="differs"):
        sf.features_many([np.zeros((5, 2, 10), np.float32), np.zeros((4, 2, 10), np.float32)])
    with pytest.raises(ValueError, match="librosa_reflect"):
        StemFeatures(framing="librosa_reflect").features_many([np.zeros((5, 2, 2048), np.float32)])
    bare = object.__new__(ClipBatchPipeline)          # (the check comes before anything the pipeline holds is used)
    with pytest.raises(ValueError, match="not both"):
        bare.extract_stage([None], features=[None], stems=[None])
    with pytest.raises(ValueError, match="not both"):
        bare.run([None], features=[None], stems=[None])


# ------------------------------------------------------------------ the restatement itself
def test_restatement_zero_stem_and_range():
    x = sn.synthetic_stems(3, instr=3, channels=2, N=1024 * 12 + 517, silent_stem=1, zero_frames=(0, 5, 8))
    for framing in sn.FRAMINGS:
        y = sn.features(x, framing=framing)
        assert y.shape == (3, sn.num_frames(x.shape[2], framing=framing), 128)
        assert (y[1] == 0.0).all()
        assert y.min() >= -80.0 and y.max() <= 0.0
        assert y[0].max() == 0.0 and y[2].max() == 0.0
        assert (y[0][5:8] == -80.0).all()                     # zero frames inside a live stem
    y32 = sn.features(x, dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - sn.features(x)).max() < 0.05


def test_restatement_framing_against_np_pad():
    rng = np.random.default_rng(0)
    n_fft, hop, N = 256, 64, 64 * 9 + 23
    x = rng.standard_normal(N).astype(np.float32)
    for framing, lead, mode in (("librosa", n_fft // 2, "constant"), ("librosa_reflect", n_fft // 2, "reflect"), ("spleeter", n_fft, "constant")):
        padded = np.pad(x, (lead, lead), mode=mode)
        T = 1 + (padded.size - n_fft) // hop
        direct = np.stack([padded[t * hop:t * hop + n_fft] for t in range(T)])
        got = sn.frames_of(x, n_fft, hop, framing)
        assert got.shape == (T, n_fft) == (sn.num_frames(N, n_fft, hop, framing), n_fft)
        assert np.array_equal(got, direct)
        # frame t covers samples [t * hop - lead, + n_fft)
        t = 5
        lo = t * hop - lead
        seg = np.array([x[i] if 0 <= i < N else 0.0 for i in range(lo, lo + n_fft)], np.float32)
        if mode == "constant":
            assert np.array_equal(got[t], seg)
    with pytest.raises(ValueError):
        sn.frames_of(x[:128], n_fft, hop, "librosa_reflect")


def test_restatement_mono_is_fp32_channel_mean():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 3, 50)).astype(np.float32)
    m = sn.mono_of(x)
    assert m.dtype == np.float32
    assert np.array_equal(m, ((x[:, 0] + x[:, 1]) + x[:, 2]) / np.float32(3))
