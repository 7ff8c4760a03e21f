"""The test-only shim tests/native/note_commit_dev.hip (the compact note scan's device headers on their own), with the product's
flags as native_build.py reads them from the Makefile."""
import ctypes as C

import native_build

UNIT = native_build.unit("note_commit_dev")
STRIDE = 160


def load():
    return native_build.load(UNIT)


def run(op, items, gpu, extra=None):
    """items: (head[<= 32 bytes at the slot's start], message bytes, length); extra: per item 84 bytes (op 6) -> list of 64-byte results"""
    import numpy as np
    n = len(items)
    slots = np.zeros((n, STRIDE), np.uint8)
    lens = np.zeros(n, np.uint32)
    for i, (head, msg, ln) in enumerate(items):
        slots[i, :len(head)] = np.frombuffer(head, np.uint8)
        slots[i, 32:32 + len(msg)] = np.frombuffer(msg, np.uint8)
        lens[i] = ln
    out = np.zeros((n, 64), np.uint8)
    ext = np.zeros((n, 84), np.uint8)
    for i, e in enumerate(extra or []):
        ext[i] = np.frombuffer(e, np.uint8)
    f = load().ncm_run_gpu if gpu else load().ncm_run_host
    rc = f(op, slots.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, ext.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [o.tobytes() for o in out]
