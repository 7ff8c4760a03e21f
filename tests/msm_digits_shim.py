"""Loader of the test-only unit tests/native/msm_digits_dev.hip (MsmDigitIter of masp_amd/csrc/device/msm_sort.hpp on the host:
needs no device), with the product's flags as native_build.py reads them from the Makefile.  Scalars go in as Python ints, digits come out
as tuples of ints."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("msm_digits_dev")


def load():
    return native_build.load(UNIT)


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
