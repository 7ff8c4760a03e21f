"""Build of the test-only shim tests/native/conversion_dev.hip (device/conversion.hpp on the host, and the product's conversion kernels for
either lane width on the GPU), with the product's flags as device_shim.py reads them from the Makefile; rebuilt when it or a source it
includes is newer than the library."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import device_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "conversion_dev.hip")
SO = os.path.join(HERE, "native", "_conversion_dev.so")
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")
_lib = None


def dependencies():
    return [SRC, device_shim.MAKEFILE, os.path.join(CSRC, "k_conversion.hip")] + \
        [p for pat in ("device/*.hpp", "device/*.h", "host/*.h", "*.h") for p in glob.glob(os.path.join(CSRC, pat))]


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in dependencies()):
            flags = device_shim.makefile_flags()
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call([device_shim.HIPCC] + flags + ["-shared", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
    return _lib


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
