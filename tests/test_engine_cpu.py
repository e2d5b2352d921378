"""The engine skeleton (etude_amd/_engine.py), none of which needs a GPU: the handle base, the ctypes helpers, the mono-song checks and the one CSR function the
front end and ``StemFeatures`` share."""
import ctypes as C
import gc
import sys
import warnings

import numpy as np
import pytest
import torch

from etude_amd import _lib
from etude_amd._engine import Engine, i32, i64, mono_songs_to_device, nonneg, ptrs


class _Tuning(Engine):
    """a real handle of the library's cheapest create"""
    _destroy = "etd_tuning_destroy"

    def __init__(self, device="cpu", hop=8192):
        self.device = torch.device(device)
        h = C.c_void_p()
        _lib.check(_lib.lib().etd_tuning_create(C.byref(_lib.TuningCfg(sample_rate=22050, n_fft=16384, hop=hop)), C.byref(h)), "etd_tuning_create")
        self._adopt(h)


def test_failed_create_is_collected_silently(recwarn):
    unraisable = []
    old, sys.unraisablehook = sys.unraisablehook, lambda u: unraisable.append(u)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises(_lib.EtudeHipError, match="tuning_create"):
                _Tuning(hop=1)                    # the library refuses the config: __init__ raises before _adopt
            e = _Tuning.__new__(_Tuning)          # what such an __init__ leaves behind: no handle was ever adopted
            assert not hasattr(e, "h")
            del e
            gc.collect()
    finally:
        sys.unraisablehook = old
    assert unraisable == [] and len(recwarn) == 0


def test_close_twice_is_harmless():
    e = _Tuning()
    assert e.h.value and e._h is e.h          # (the former name reads the same handle)
    e.close()
    assert e.h is None
    e.close()
    assert e.h is None
    e.__del__()
    never = _Tuning.__new__(_Tuning)
    never.close()
    assert never.h is None


def test_align_features_close_closes_its_handles():
    """``AlignFeatures`` owns ``_Handle`` objects, not a handle of its own: close() closes those, twice is harmless, and a later host call makes one again"""
    from etude_amd.alignfeat import AlignFeatures
    af = AlignFeatures("cpu")
    hd = af._handle((0.0,))
    assert hd.h.value
    af.close()
    assert hd.h is None and af._handles == {}
    af.close()
    assert af.num_frames(441) == 1 and len(af._handles) == 1


def test_device_on_cpu_names_the_subclass():
    e = _Tuning("cpu")
    with pytest.raises(_lib.EtudeHipError, match=r"^etude_amd\._Tuning needs a ROCm GPU \(device='cuda'\); there is no CPU path$"):
        e._device()
    from etude_amd.tuning import TuningEstimator
    with pytest.raises(_lib.EtudeHipError, match=r"^etude_amd\.TuningEstimator needs a ROCm GPU"):
        TuningEstimator("cpu")._device()


def test_nonneg_passes_values_and_raises_the_last_error():
    assert nonneg(0, "x") == 0 and nonneg(7, "x") == 7 and nonneg(1 << 40, "x") == 1 << 40
    e = _Tuning()
    rc = _lib.lib().etd_tuning_workspace_bytes(e.h, 1, i64([5]))          # a song below two windows: the library refuses and says why
    assert rc < 0
    with pytest.raises(_lib.EtudeHipError, match=r"etd_tuning_workspace_bytes failed \(rc=-22\): tuning: song 0 has N = 5"):
        nonneg(rc, "etd_tuning_workspace_bytes")


def test_ctypes_arrays_round_trip():
    a = i64([0, -1, 1 << 40, np.int64(7)])
    assert isinstance(a, C.Array) and a._type_ is C.c_int64 and list(a) == [0, -1, 1 << 40, 7]
    b = i32(np.asarray([3, -2, 2 ** 31 - 1]))
    assert b._type_ is C.c_int32 and list(b) == [3, -2, 2 ** 31 - 1]
    assert len(i64([])) == 0
    ts = [torch.zeros(4), torch.zeros(2, 3), torch.zeros(1, dtype=torch.float64)]
    p = ptrs(ts)
    assert p._type_ is C.c_void_p and list(p) == [t.data_ptr() for t in ts]


@pytest.mark.parametrize("min_n, short_msg", [(1, ""), (32768, "is shorter than two windows (32768 samples): the tuning cannot be estimated")])
def test_mono_song_refusals_fire_before_a_device_is_asked_for(min_n, short_msg):
    max_n = min_n + 100
    asked = []

    def dev():
        asked.append(1)
        raise AssertionError("the device was asked for")
    shape_msg = "need mono samples " + ("[N]" if short_msg else "[N >= 1]") + ", got shape "
    ok = np.zeros(min_n, np.float32)
    for shp in ((), (2, 8)):
        with pytest.raises(ValueError) as ei:
            mono_songs_to_device([ok, np.zeros(shp, np.float32)], dev, min_n, max_n, short_msg)
        assert str(ei.value) == f"song 1: {shape_msg}{shp}"
    with pytest.raises(ValueError) as ei:
        mono_songs_to_device([[0.0] * 4], dev, min_n, max_n, short_msg)
    assert str(ei.value) == f"song 0: {shape_msg}None"
    for N in sorted({0, min_n - 1}):
        with pytest.raises(ValueError) as ei:
            mono_songs_to_device([np.zeros(N, np.float32)], dev, min_n, max_n, short_msg)
        assert str(ei.value) == (f"song 0: N = {N} {short_msg}" if short_msg else f"song 0: {shape_msg}({N},)")
    with pytest.raises(ValueError) as ei:
        mono_songs_to_device([ok, ok, np.zeros(max_n + 1, np.float32)], dev, min_n, max_n, short_msg)
    assert str(ei.value) == f"song 2: N = {max_n + 1} is above the engine's {max_n} samples"
    assert asked == []
    with pytest.raises(AssertionError, match="the device was asked for"):      # ... and good shapes do ask
        mono_songs_to_device([ok], dev, min_n, max_n, short_msg)
    assert asked == [1]


def test_engines_refuse_with_their_own_sentences():
    """the two callers' texts, as they were before they shared the block"""
    from etude_amd.alignfeat import AlignFeatures
    from etude_amd.tuning import TuningEstimator
    tn, af = TuningEstimator("cpu"), AlignFeatures("cpu")
    with pytest.raises(ValueError, match=r"^song 0: need mono samples \[N\], got shape \(2, 8\)$"):
        tn.check_songs([np.zeros((2, 8), np.float32)])
    with pytest.raises(ValueError, match=r"^song 0: N = 32767 is shorter than two windows \(32768 samples\): the tuning cannot be estimated$"):
        tn.check_songs([np.zeros(32767, np.float32)])
    with pytest.raises(ValueError, match=r"^song 0: need mono samples \[N >= 1\], got shape \(0,\)$"):
        af.features_many([np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match=r"^song 1: need mono samples \[N >= 1\], got shape \(\)$"):
        af.features_many([np.zeros(4, np.float32), np.zeros((), np.float32)])
    with pytest.raises(_lib.EtudeHipError, match="AlignFeatures needs a ROCm GPU"):      # good shapes reach the device question
        af.features_many([np.zeros(4, np.float32)])


def _scan_rows(fb):
    """``StemFeatures``' former function, verbatim: [n_mels][bins]"""
    start, length, w = [], [], []
    for row in fb:
        nz = np.flatnonzero(row)
        if nz.size == 0:
            start.append(0); length.append(0)
            continue
        start.append(int(nz[0])); length.append(int(nz[-1] - nz[0] + 1))
        w.append(row[nz[0]:nz[-1] + 1])
    weights = np.ascontiguousarray(np.concatenate(w) if w else np.zeros(1, np.float32), np.float32)
    return np.asarray(start, np.int32), np.asarray(length, np.int32), weights


def _scan_columns(fb):
    """the front end's function as it stood, verbatim: [bins][n_mels]"""
    n_mels = fb.shape[1]
    start = np.zeros(n_mels, np.int32)
    length = np.zeros(n_mels, np.int32)
    w = []
    for m in range(n_mels):
        nz = np.flatnonzero(fb[:, m])
        if nz.size:
            start[m], length[m] = nz[0], nz[-1] - nz[0] + 1
            w.append(fb[nz[0]:nz[-1] + 1, m])
    wcat = np.concatenate(w).astype(np.float32) if w else np.zeros(1, np.float32)
    return start, length, wcat


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.flags.c_contiguous and g.tobytes() == w.tobytes()


def test_one_csr_function_serves_both_filterbanks():
    from etude_amd import frontend, stemfeat
    assert stemfeat._dense_to_csr is frontend._dense_to_csr
    # StemFeatures' default filterbank, [128][2049], and a small one with the same structure
    for fb in (stemfeat.mel_filterbank(), stemfeat.mel_filterbank(44100, 256, 32, 30.0, 11000.0)):
        _same(stemfeat._csr(fb), _scan_rows(fb))
        _same(frontend._dense_to_csr(fb.T), _scan_rows(fb))
    # the front end's default filterbank (16 kHz, n_fft 2048, 256 bands) and its n_fft = 64 setting, which has empty bands; rebuilt dense from what _mel_csr returns
    for n_freqs, empty in ((1025, False), (33, True)):
        start, length, w = frontend._mel_csr(n_freqs, 8000.0, 256, 16000)
        dense, o = np.zeros((n_freqs, 256), np.float32), 0
        for m in range(256):
            dense[start[m]:start[m] + length[m], m] = w[o:o + length[m]]
            o += length[m]
        assert o == (0 if not length.any() else w.size) and bool((length == 0).any()) == empty
        _same((start, length, w), _scan_columns(dense))
        _same(frontend._dense_to_csr(dense), _scan_columns(dense))
        _same(stemfeat._csr(np.ascontiguousarray(dense.T)), _scan_rows(np.ascontiguousarray(dense.T)))
        _same(_scan_rows(np.ascontiguousarray(dense.T)), _scan_columns(dense))      # the two former functions agreed on either bank
    _same(stemfeat._csr(np.zeros((3, 9), np.float32)), _scan_rows(np.zeros((3, 9), np.float32)))
