"""g3_pack_weights_host (csrc/gemm3.hip) through etd_debug_g3_pack, host only: the f16 hi / lo planes of a weight matrix in the order k_gemm3 / k_gemm3_s stream them,
[Npad / 128 tile][K / 32 chunk][hi | lo][128 rows][32 k], unpacked here by that documented index formula."""
import ctypes as C

import numpy as np
import pytest

from etude_amd import _lib


def _pack(w):
    N, K = w.shape
    lib = _lib.lib()
    n, lg = C.c_longlong(), C.c_int32()
    assert lib.etd_debug_g3_pack(w.ctypes.data, N, K, None, 0, C.byref(n), C.byref(lg)) == -12          # ETD_ENOMEM: the capacity rule reports what is needed
    npad = (N + 127) // 128 * 128
    assert n.value == npad * K * 2
    buf = np.full(n.value, 0x7E00, np.uint16)                                                           # (f16 NaN: every element must be written)
    _lib.check(lib.etd_debug_g3_pack(w.ctypes.data, N, K, buf.ctypes.data, buf.size, C.byref(n), C.byref(lg)), "etd_debug_g3_pack")
    planes = buf.view(np.float16).reshape(npad // 128, K // 32, 2, 128, 32)
    # element (n, k) of plane p sits at [n >> 7][k >> 5][p][n & 127][k & 31]
    hi, lo = (planes[:, :, p].transpose(0, 2, 1, 3).reshape(npad, K) for p in (0, 1))
    return hi, lo, lg.value


@pytest.mark.parametrize("N,K", [(1, 32), (131, 96), (256, 512)])
def test_planes_reproduce_the_weights(N, K):
    rng = np.random.default_rng(N + K)
    w = (rng.standard_normal((N, K)) * 0.05 * np.exp(rng.uniform(-6, 0, (N, K)))).astype(np.float32)        # magnitudes over several binades
    hi, lo, lg = _pack(w)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    s = np.float32(2.0) ** lg
    mx = float(np.abs(w).max())
    # hi + lo carries the fp32 weight to 2^-22 of the largest one, elementwise
    back = (hi[:N].astype(np.float64) + lo[:N].astype(np.float64)) * 2.0 ** -lg
    assert np.abs(back - w).max() <= 2.0 ** -22 * mx
    # hi is the round-to-nearest f16 of s w (s a power of two: s w is exact), lo that of the remainder
    t = w * s
    assert np.array_equal(hi[:N], t.astype(np.float16))
    assert np.array_equal(lo[:N], (t - hi[:N].astype(np.float32)).astype(np.float16))
    # rows N .. Npad of the last tile are zero in both planes
    assert not hi[N:].any() and not lo[N:].any()
    # the scale puts the largest plane value into [2^14, 2^15)
    top = float(np.abs(hi).max())
    assert 2.0 ** 14 <= top < 2.0 ** 15
    assert 2.0 ** 14 <= mx * float(s) < 2.0 ** 15


def test_all_zero_matrix():
    hi, lo, lg = _pack(np.zeros((131, 96), np.float32))
    assert lg == 0
    assert not hi.any() and not lo.any()


def test_bad_arguments_are_refused():
    lib = _lib.lib()
    n, lg = C.c_longlong(), C.c_int32()
    w = np.zeros((4, 48), np.float32)
    assert lib.etd_debug_g3_pack(w.ctypes.data, 4, 48, None, 0, C.byref(n), C.byref(lg)) == -22           # K % 32
    assert lib.etd_debug_g3_pack(None, 4, 32, None, 0, C.byref(n), C.byref(lg)) == -22
