"""Build of the test-only unit tests/native/verify_dev.hip (the GPU batch verifier's kernels, each on its own, and wrappers over the host
pairing), with the product's flags as device_shim.py reads them from the Makefile; rebuilt when it or a header it includes is newer than
the library.  Everything that goes in or comes out is canonical: Fp as Python ints, Fp12 as 12-tuples in the host's flat coefficient
order, points as bellman uncompressed wire bytes (pyref.g1_unc / g2_unc)."""
import ctypes as C
import glob
import os
import subprocess

import device_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "verify_dev.hip")
SO = os.path.join(HERE, "native", "_verify_dev.so")
CSRC = os.path.join(os.path.dirname(HERE), "masp_amd", "csrc")
_lib = None


def dependencies():
    """the unit includes device/pairing.hpp (and through it most of device/), host/pairing.h, host/pairing_prog.h, verify_launch.h, util.h"""
    return [SRC, device_shim.MAKEFILE, os.path.join(CSRC, "verify_launch.h"), os.path.join(CSRC, "util.h"),
            os.path.join(os.path.dirname(HERE), "include", "masp_hip.h")] + \
        sorted(glob.glob(os.path.join(CSRC, "device", "*.hpp")) + glob.glob(os.path.join(CSRC, "device", "*.h"))) + \
        [os.path.join(CSRC, "host", f) for f in ("pairing.h", "pairing_prog.h", "mont.h")]


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


def fp12_bytes(f):
    assert len(f) == 12
    return b"".join(int(c).to_bytes(48, "big") for c in f)


def fp12_tuple(b):
    assert len(b) == 576
    return tuple(int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(12))


# ---- the kernels (GPU) ----
def prepare_gpu(proofs, zs):
    """proofs: 192-byte strings, zs: 16-byte strings -> (status ints, za 96-byte strings, b 192-byte strings, zc 96-byte strings)"""
    n = len(proofs)
    assert n == len(zs) and all(len(p) == 192 for p in proofs) and all(len(z) == 16 for z in zs)
    status = (C.c_int * n)()
    za, b, zc = C.create_string_buffer(96 * n), C.create_string_buffer(192 * n), C.create_string_buffer(96 * n)
    rc = load().vfy_prepare_gpu(b"".join(proofs), b"".join(zs), n, status, za, b, zc)
    assert rc == 0, rc
    cut = lambda buf, w: [buf.raw[w * i:w * i + w] for i in range(n)]
    return list(status), cut(za, 96), cut(b, 192), cut(zc, 96)


def g1_sum_gpu(points96):
    out = C.create_string_buffer(96)
    rc = load().vfy_g1_sum_gpu(b"".join(points96), len(points96), out)
    assert rc == 0, rc
    return out.raw


def miller_gpu(pairs):
    """pairs: (p 96 bytes, q 192 bytes) -> list of Fp12 tuples"""
    return _miller(load().vfy_miller_gpu, pairs)


def fp12_product_gpu(vals):
    out = C.create_string_buffer(576)
    rc = load().vfy_fp12_product_gpu(b"".join(fp12_bytes(v) for v in vals), len(vals), out)
    assert rc == 0, rc
    return fp12_tuple(out.raw)


# ---- host/pairing.h (no GPU) ----
def _miller(f, pairs):
    n = len(pairs)
    out = C.create_string_buffer(576 * n)
    rc = f(b"".join(bytes(p) for p, _ in pairs), b"".join(bytes(q) for _, q in pairs), n, out)
    assert rc == 0, rc
    return [fp12_tuple(out.raw[576 * i:576 * i + 576]) for i in range(n)]


def miller_host(pairs):
    return _miller(load().vfy_miller_host, pairs)


def fp12_mul_host(a, b):
    out = C.create_string_buffer(576)
    rc = load().vfy_fp12_mul_host(fp12_bytes(a), fp12_bytes(b), out)
    assert rc == 0, rc
    return fp12_tuple(out.raw)


def final_exp_is_one_host(f):
    rc = load().vfy_final_exp_is_one_host(fp12_bytes(f))
    assert rc in (0, 1), rc
    return rc == 1


def final_exp_eq_host(a, b):
    rc = load().vfy_final_exp_eq_host(fp12_bytes(a), fp12_bytes(b))
    assert rc in (0, 1), rc
    return rc == 1
