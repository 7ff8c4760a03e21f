"""The test-only shim tests/native/nullifier_dev.hip (device/nullifier.hpp on the host, and the product's nullifier kernels for
either lane width on the GPU), with the product's flags as native_build.py reads them from the Makefile."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("nullifier_dev")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.nfd_table_mul_host.argtypes = [C.c_int, C.c_char_p, C.c_char_p]
    return _lib


def table_mul(which, k):
    """[k] G_ncr (which = 0) or [k] G_nf (which = 1) from the device's fixed-base table, on the host -> 32 bytes"""
    out = C.create_string_buffer(32)
    assert load().nfd_table_mul_host(which, int(k).to_bytes(32, "little"), out) == 0
    return out.raw


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def steps_host(arrays, lanes=1, trace=False):
    """device/nullifier.hpp's steps on the CPU -> (status, cmus, nfs[, trace uint8[n, 208]: msg 104 | rcm 32 | cm 32 | rho 32 | bad 8])"""
    n = arrays[0].shape[0]
    status, cmus, nfs = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    tr = np.zeros((n, 208), np.uint8) if trace else None
    rc = load().nfd_steps_host(n, *[_p(a) for a in arrays], int(lanes), _p(status), _p(cmus), _p(nfs), _p(tr))
    assert rc == 0, rc
    return (status, cmus, nfs, tr) if trace else (status, cmus, nfs)


def run_gpu(arrays, lanes):
    """the product's four kernels with `lanes` (1 or 8) lanes per note -> (status, cmus, nfs)"""
    n = arrays[0].shape[0]
    status, cmus, nfs = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    rc = load().nfd_run_gpu(n, *[_p(a) for a in arrays], int(lanes), _p(status), _p(cmus), _p(nfs))
    assert rc == 0, rc
    return status, cmus, nfs
