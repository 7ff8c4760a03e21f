"""The test-only unit tests/native/verify_each_dev.hip (k_final_exp and k_verify_acc of masp_hip_verify_each, each on its own,
and a wrapper over the host's final exponentiation), in the manner of verify_shim.py: the product's flags, canonical values only (Fp12
as 12-tuples of ints, points as bellman uncompressed wire bytes)."""
import ctypes as C

import native_build
from verify_shim import fp12_bytes, fp12_tuple

UNIT = native_build.unit("verify_each_dev")


def load():
    return native_build.load(UNIT)


def final_exp_gpu(vals):
    """Fp12 tuples -> (their powers by 3 (p^12 - 1) / r as tuples, verdict bytes) from k_final_exp, one wavefront per value"""
    n = len(vals)
    out, verdict = C.create_string_buffer(576 * n), C.create_string_buffer(n)
    rc = load().ve_final_exp_gpu(b"".join(fp12_bytes(v) for v in vals), n, out, verdict)
    assert rc == 0, rc
    return [fp12_tuple(out.raw[576 * i:576 * i + 576]) for i in range(n)], list(verdict.raw[:n])


def final_exp_host(f):
    out = C.create_string_buffer(576)
    rc = load().ve_final_exp_host(fp12_bytes(f), out)
    assert rc == 0, rc
    return fp12_tuple(out.raw)


def acc_gpu(ic96, inputs, status=None):
    """ic96: the n_public + 1 IC points (96 bytes each); inputs: one list of n_public ints below 2^256 per proof -> (-acc as 96-byte
    strings, pre bytes) from k_verify_acc"""
    n, n_public = len(inputs), len(ic96) - 1
    assert all(len(row) == n_public for row in inputs)
    status = (C.c_int * n)(*(status or [0] * n))
    out, pre = C.create_string_buffer(96 * n), C.create_string_buffer(n)
    data = b"".join(int(x).to_bytes(32, "little") for row in inputs for x in row)
    rc = load().ve_acc_gpu(b"".join(bytes(p) for p in ic96), n_public, data, status, n, out, pre)
    assert rc == 0, rc
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], list(pre.raw[:n])
