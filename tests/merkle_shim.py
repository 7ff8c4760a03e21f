"""The test-only shim tests/native/merkle_dev.hip (the commitment tree's device header on the host), with the product's flags as
native_build.py reads them from the Makefile."""
import ctypes as C

import native_build

UNIT = native_build.unit("merkle_dev")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.mkl_row_host.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib.mkl_row_host.restype = None
    return _lib


def combine(items):
    """items: (level, lhs 32 bytes, rhs 32 bytes) -> list of 32-byte parents from device/merkle.hpp's merkle_combine on the host"""
    buf = b"".join(int(level).to_bytes(4, "little") + bytes(lhs) + bytes(rhs) for level, lhs, rhs in items)
    out = C.create_string_buffer(32 * len(items))
    assert load().mkl_combine_host(buf, len(items), out) == 0
    return [out.raw[32 * i:32 * i + 32] for i in range(len(items))]


def is_canonical(nodes):
    out = C.create_string_buffer(len(nodes))
    assert load().mkl_is_canonical_host(b"".join(bytes(x) for x in nodes), len(nodes), out) == 0
    return [b != 0 for b in out.raw]


def row(n, i):
    s, w = C.c_uint64(0), C.c_uint64(0)
    load().mkl_row_host(n, i, C.byref(s), C.byref(w))
    return s.value, w.value
