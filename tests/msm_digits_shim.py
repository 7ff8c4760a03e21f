"""Build and loader of the test-only unit tests/native/msm_digits_dev.hip (MsmDigitIter of masp_amd/csrc/device/msm_sort.hpp on the host:
needs no device), with the product's flags as device_shim.py reads them from the Makefile; rebuilt when the unit or a header it includes is
newer than the library.  Scalars go in as Python ints, digits come out as tuples of ints."""
import ctypes as C
import os
import subprocess

import numpy as np

import device_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "msm_digits_dev.hip")
SO = os.path.join(HERE, "native", "_msm_digits_dev.so")
DEVICE = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc", "device")
_lib = None


def dependencies():
    return [SRC, device_shim.MAKEFILE, os.path.join(DEVICE, "msm_sort.hpp"), os.path.join(DEVICE, "msm_geom.h")]


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in dependencies()):
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call([device_shim.HIPCC] + device_shim.makefile_flags() + ["-shared", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
    return _lib


def digits(scalars, c, twin=False):
    """-> per scalar the list of W tuples (table, bucket, neg, non-zero), window after window, as MsmDigitIter::next hands them out"""
    n = len(scalars)
    W = (256 + c - 1) // c
    raw = b"".join(int(s).to_bytes(32, "little") for s in scalars)
    out = (C.c_uint32 * (n * W * 4))()
    got = load().mdd_digits(raw, n, c, 1 if twin else 0, out)
    assert got == W, (got, W)
    return [[tuple(q) for q in per] for per in np.frombuffer(out, np.uint32).reshape(n, W, 4).tolist()]


def scalar_class(s):
    return int(load().mdd_class(int(s).to_bytes(32, "little")))
