"""The test-only shim tests/native/out_recovery_dev.hip (the output recovery scan's device header on its own), with the
product's flags as native_build.py reads them from the Makefile."""
import ctypes as C

import native_build

UNIT = native_build.unit("out_recovery_dev")
ROW, OUT = 176, 36


def load():
    return native_build.load(UNIT)


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
