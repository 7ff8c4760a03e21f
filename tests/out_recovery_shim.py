"""Build of the test-only shim tests/native/out_recovery_dev.hip (the output recovery scan's device header on its own), with the
product's flags as device_shim.py reads them from the Makefile; rebuilt when it or a header it includes is newer than the library."""
import ctypes as C
import os
import subprocess

import device_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "out_recovery_dev.hip")
SO = os.path.join(HERE, "native", "_out_recovery_dev.so")
DEV = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc", "device")
DEPS = [SRC] + [os.path.join(DEV, f) for f in ("out_recovery.hpp", "blake2b.hpp", "chacha20.hpp", "poly1305.hpp", "field.hpp", "consts.hpp")]
ROW, OUT = 176, 36
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in DEPS):
            flags = device_shim.makefile_flags()
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call([device_shim.HIPCC] + flags + ["-shared", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
    return _lib


def run(pairs, gpu):
    """pairs: (ovk[32], cv[32], cmu[32], epk[32], c_out[80]) -> list of (ock[32], whether the tag verifies)"""
    import numpy as np
    n = len(pairs)
    ovks = np.frombuffer(b"".join(p[0] for p in pairs), np.uint8).reshape(n, 32).copy()
    rows = np.frombuffer(b"".join(b"".join(p[1:]) for p in pairs), np.uint8).reshape(n, ROW).copy()
    out = np.zeros((n, OUT), np.uint8)
    f = load().or_run_gpu if gpu else load().or_run_host
    rc = f(ovks.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [(o[:32].tobytes(), int.from_bytes(o[32:].tobytes(), "little") == 1) for o in out]
