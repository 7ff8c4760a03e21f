"""The test-only shim tests/native/bundle_check_dev.hip (device/bundle_check.hpp on the host: the per-item steps of
masp_hip_sapling_check_bundles and a whole call, lane after lane), with the product's flags as native_build.py reads them from the
Makefile.  `HostContext` serves Context.check_bundles from it, with the
proofs' statuses from the host library's `Proof::read`: BatchValidator.check_bundles runs over it without a GPU."""
import ctypes as C

import numpy as np

import native_build
from masp_amd import hip as HIP
from masp_amd import host as H

UNIT = native_build.unit("bundle_check_dev")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.bcd_point.argtypes = [C.c_char_p, C.c_char_p]
        _lib.bcd_balance_term.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        _lib.bcd_multipack.argtypes = [C.c_char_p, C.c_char_p]
        _lib.bcd_multipack.restype = None
        _lib.bcd_check_bundles_host.argtypes = [C.POINTER(HIP.BundleCheckStruct), C.c_char_p]
    return _lib


def point(enc):
    """one Jubjub encoding -> (0 fine / 1 does not decode / 2 small order, u, v): bc_point"""
    out = C.create_string_buffer(64)
    st = load().bcd_point(bytes(enc), out)
    return st, int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def balance_term(identifier, value):
    """one value-balance entry -> (0 / 2 i128::MIN / 3 no generator, the encoding of the term bvk adds): bc_balance_term"""
    out = C.create_string_buffer(32)
    st = load().bcd_balance_term(bytes(identifier), int(value).to_bytes(16, "little", signed=True), out)
    return st, out.raw


def multipack(nullifier):
    out = C.create_string_buffer(64)
    load().bcd_multipack(bytes(nullifier), out)
    return [int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")]


def check_bundles(counts, spends, converts, outputs, balance):
    """Context.check_bundles on the CPU: the kernels' lanes one after the other, `Proof::read` by the host library"""
    s, res, keep = HIP.bundle_check_args(counts, spends, converts, outputs, balance)
    proofs = [bytes(row) for g in keep[1][:3] for row in g[-1]]
    refused = bytes(0 if H.proof_read(p) else 1 for p in proofs)
    rc = load().bcd_check_bundles_host(C.byref(s), refused)
    if rc:
        raise HIP.MaspHipError(rc)
    return res


class HostContext:
    """a stand-in for hip.Context where BatchValidator.check_bundles needs one"""

    def __init__(self):
        self.calls = []

    def check_bundles(self, counts, spends, converts, outputs, balance):
        self.calls.append(len(counts))
        return check_bundles(counts, spends, converts, outputs, balance)
