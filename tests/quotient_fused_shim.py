"""The test-only unit tests/native/quotient_fused_dev.hip (the evaluation-form quotient's three kernels, each on its own behind the
product's launch wrapper, and the two whole chains), with the product's flags as native_build.py reads them from the Makefile.  Scalars go
in and come out as Python ints (canonical values), except in chains_gpu, which takes and returns numpy words as they lie in memory."""
import ctypes as C

import numpy as np

import native_build
from prove_stages_shim import MARKER, ints, words

UNIT = native_build.unit("quotient_fused_dev")
_lib = None


def load():
    global _lib
    if _lib is None:
        L = native_build.load(UNIT)
        u32, u64, u8, p = C.c_uint32, C.c_uint64, C.c_uint8, C.c_void_p
        L.qf_fused_ok.argtypes = [u32]
        L.qf_tile_log.restype = u32
        L.qf_powers_bitrev_gpu.argtypes = [u32, p, p, p]
        L.qf_dif_top_gpu.argtypes = [p, p, u64, u32, u32, u32, p, u8]
        L.qf_mid_gpu.argtypes = [p, u32, u32]
        L.qf_dit_top_ab_gpu.argtypes = [p, u32, u32, p, u64, u8]
        L.qf_chains_gpu.argtypes = [p, p, u64, u32, u32, u32, p, p, u64, u8]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fused_ok(logm):
    return bool(load().qf_fused_ok(logm))


def tile_log():
    return int(load().qf_tile_log())


def powers_bitrev_gpu(logn, base, scale):
    out = np.zeros((1 << logn, 32), dtype=np.uint8)
    rc = load().qf_powers_bitrev_gpu(logn, _p(words([base])), _p(words([scale])), _p(out))
    assert rc == 0, rc
    return ints(out)


def dif_top_gpu(a, b, in_stride, nrows, logm, q, marker=MARKER):
    """a, b: q * in_stride canonical ints -> [a | b], 2 q << logm canonical ints"""
    assert len(a) == len(b) == q * in_stride
    ab, bb, y = words(a), words(b), np.zeros(((2 * q) << logm, 32), dtype=np.uint8)
    rc = load().qf_dif_top_gpu(_p(ab), _p(bb), in_stride, nrows, logm, q, _p(y), marker)
    assert rc == 0, rc
    return ints(y)


def mid_gpu(x, logm, np_):
    assert len(x) == np_ << logm
    xb = words(x)
    rc = load().qf_mid_gpu(_p(xb), logm, np_)
    assert rc == 0, rc
    return ints(xb)


def dit_top_ab_gpu(x, logm, q, y_stride, marker=MARKER):
    """x = [a | b]: 2 q << logm canonical ints -> q * y_stride raw words (the gaps hold marker bytes)"""
    assert len(x) == (2 * q) << logm
    xb, y = words(x), np.zeros((q * y_stride, 32), dtype=np.uint8)
    rc = load().qf_dit_top_ab_gpu(_p(xb), logm, q, _p(y), y_stride, marker)
    assert rc == 0, rc
    return ints(y)


def chains_gpu(a, b, in_stride, nrows, logm, q, y_stride, marker=MARKER):
    """a, b: u8[q * in_stride, 32] residues below r as they lie in memory -> (fused, separate), each u8[q * y_stride, 32]"""
    assert a.shape == b.shape == (q * in_stride, 32) and a.dtype == b.dtype == np.uint8
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    yf, ys = np.zeros((q * y_stride, 32), dtype=np.uint8), np.ones((q * y_stride, 32), dtype=np.uint8)
    rc = load().qf_chains_gpu(_p(a), _p(b), in_stride, nrows, logm, q, _p(yf), _p(ys), y_stride, marker)
    assert rc == 0, rc
    return yf, ys
