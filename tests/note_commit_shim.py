"""Build of the test-only shim tests/native/note_commit_dev.hip (the compact note scan's device headers on their own), with the product's
flags as device_shim.py reads them from the Makefile; rebuilt when it or a header it includes is newer than the library."""
import ctypes as C
import os
import subprocess

import device_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "note_commit_dev.hip")
SO = os.path.join(HERE, "native", "_note_commit_dev.so")
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, "device", f) for f in ("blake2s.hpp", "blake2b.hpp", "chacha20.hpp", "compact_note.hpp", "group_hash.hpp", "pedersen.hpp", "jubjub.hpp",
                                                           "field.hpp", "consts.hpp")] + \
    [os.path.join(CSRC, "host", f) for f in ("jubjub.h", "fr.h", "mont.h")]
STRIDE = 160
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
