"""The test-only shim tests/native/conversion_dev.hip (device/conversion.hpp on the host, and the product's conversion kernels for
either lane width on the GPU), with the product's flags as native_build.py reads them from the Makefile."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("conversion_dev")


def load():
    return native_build.load(UNIT)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _outputs(n):
    return np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)


def steps_host(off, ids, vals, lanes=1, trace=False):
    """device/conversion.hpp's steps on the CPU -> (status, generators, cmus[, trace uint8[n, 64]: generator point 32 | cm 32])"""
    n = off.shape[0] - 1
    status, gens, cmus = _outputs(n)
    tr = np.zeros((n, 64), np.uint8) if trace else None
    rc = load().cvd_steps_host(n, _p(off), ids.shape[0], _p(ids), _p(vals), int(lanes), _p(status), _p(gens), _p(cmus), _p(tr))
    assert rc == 0, rc
    return (status, gens, cmus, tr) if trace else (status, gens, cmus)


def run_gpu(off, ids, vals, lanes):
    """the product's three kernels with `lanes` (1 or 8) lanes per conversion -> (status, generators, cmus)"""
    n = off.shape[0] - 1
    status, gens, cmus = _outputs(n)
    rc = load().cvd_run_gpu(n, _p(off), ids.shape[0], _p(ids), _p(vals), int(lanes), _p(status), _p(gens), _p(cmus))
    assert rc == 0, rc
    return status, gens, cmus
