"""The test-only unit tests/native/verify_dev.hip (the GPU batch verifier's kernels, each on its own, and wrappers over the host
pairing), with the product's flags as native_build.py reads them from the Makefile.  Everything that goes in or comes out is canonical:
Fp as Python ints, Fp12 as 12-tuples in the host's flat coefficient order, points as bellman uncompressed wire bytes (pyref.g1_unc /
g2_unc)."""
import ctypes as C

import native_build

UNIT = native_build.unit("verify_dev")


def load():
    return native_build.load(UNIT)


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
