"""The test-only unit tests/native/prove_stages_dev.hip (the prover's witness-to-quotient kernels, each on its own behind the
product's launch wrapper), with the product's flags as native_build.py reads them from the Makefile.  Scalars go in and come out as
Python ints: canonical values, except where a function says `raw` (the 256-bit word a kernel left, a Montgomery residue or an
out-of-range input)."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("prove_stages_dev")
MARKER = 0x5A
_lib = None


def load():
    global _lib
    if _lib is None:
        L = native_build.load(UNIT)
        u32, u64, u8, p = C.c_uint32, C.c_uint64, C.c_uint8, C.c_void_p
        L.pst_to_mont_gpu.argtypes = [p, u64, u32, u32, p, p]
        L.pst_split_forms_gpu.argtypes = [p, u64, u32, u32, u32, p, p]
        L.pst_r1cs_eval_gpu.argtypes = [u32, u32, u32, p, p, p, p, p, p, u32, u32, p, p]
        L.pst_gather_scalars_gpu.argtypes = [p, u64, p, u32, u32, p, u64, u8]
        L.pst_bitrev_gpu.argtypes = [C.c_int, p, u64, u32, u32, u32, p, u8]
        L.pst_mul_bitrev_gpu.argtypes = [p, p, p, u32, u32, p]
        L.pst_ab_eval_gpu.argtypes = [p, p, p, u32, u32, p, u64, u8]
        L.pst_fr_scale_gpu.argtypes = [p, p, p, p, u32, u32, p, u64, u8]
        _lib = L
    return _lib


def words(values):
    """ints below 2^256 -> u8[n, 32] little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def ints(buf):
    b = np.ascontiguousarray(buf, dtype=np.uint8).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _out(n, fill=0):
    return np.full((n, 32), fill, dtype=np.uint8)


def to_mont_gpu(x, x_stride, n, np_):
    """x: np_ * x_stride raw words -> (y raw, np_ * n; flag)"""
    assert len(x) == np_ * x_stride
    xb, y, flag = words(x), _out(np_ * n), C.c_int(-1)
    rc = load().pst_to_mont_gpu(_p(xb), x_stride, n, np_, _p(y), C.byref(flag))
    assert rc == 0, rc
    return ints(y), flag.value


def split_forms_gpu(x, x_stride, n, mont_from, np_):
    """x: np_ * x_stride raw words -> (y raw, np_ * n; x afterwards, raw; flag)"""
    assert len(x) == np_ * x_stride
    xb, y, flag = words(x), _out(np_ * n), C.c_int(-1)
    rc = load().pst_split_forms_gpu(_p(xb), x_stride, n, mont_from, np_, _p(y), C.byref(flag))
    assert rc == 0, rc
    return ints(y), ints(xb), flag.value


def r1cs_eval_gpu(cs, orders, n_long, assignments, n_mat):
    """cs: an R1cs; orders, n_long: per matrix; assignments: np lists of n_inputs + n_aux canonical ints -> ([a, b, c][:n_mat], each a
    list of np lists of n_constraints + n_inputs ints; the range flag)"""
    n_p, nrows = len(assignments), cs.n_constraints + cs.n_inputs
    assert all(len(w) == cs.n_inputs + cs.n_aux for w in assignments)
    arr = lambda items: (C.c_void_p * 3)(*[x.ctypes.data for x in items])
    order = [np.ascontiguousarray(o, dtype=np.uint32) for o in orders]
    nl = np.ascontiguousarray(n_long, dtype=np.uint32)
    w = words([v for a in assignments for v in a])
    out = [_out(n_p * nrows, MARKER) for _ in range(3)]
    flag = C.c_int(-1)
    rc = load().pst_r1cs_eval_gpu(cs.n_inputs, cs.n_aux, cs.n_constraints, arr([m[0] for m in cs.mats]), arr([m[1] for m in cs.mats]),
                                  arr([m[2] for m in cs.mats]), arr(order), _p(nl), _p(w), n_p, n_mat, arr(out), C.byref(flag))
    assert rc == 0, rc
    return [[ints(o[p * nrows:(p + 1) * nrows]) for p in range(n_p)] for o in out[:n_mat]], flag.value


def gather_scalars_gpu(src, src_stride, idx, np_, dst_stride, marker=MARKER):
    """src: np_ * src_stride raw words -> dst, np_ * (dst_stride or len(idx)) raw words (the gaps hold marker bytes)"""
    assert len(src) == np_ * src_stride
    sb, ib = words(src), np.ascontiguousarray(idx, dtype=np.uint32)
    dst = _out(np_ * (dst_stride or len(idx)))
    rc = load().pst_gather_scalars_gpu(_p(sb), src_stride, _p(ib), len(idx), np_, _p(dst), dst_stride, marker)
    assert rc == 0, rc
    return ints(dst)


def bitrev_gpu(montgomery_in, x, x_stride, nrows, logm, np_, marker=MARKER):
    """k_ntt_copy_bitrev (montgomery_in) or k_ntt_load_bitrev: x np_ * x_stride canonical ints -> y np_ << logm canonical ints"""
    assert len(x) == np_ * x_stride
    xb, y = words(x), _out(np_ << logm)
    rc = load().pst_bitrev_gpu(1 if montgomery_in else 0, _p(xb), x_stride, nrows, logm, np_, _p(y), marker)
    assert rc == 0, rc
    return ints(y)


def scale_bitrev_gpu(x, scale, logm, np_):
    assert len(x) == np_ << logm and len(scale) == 1 << logm
    xb, sb, y = words(x), words(scale), _out(np_ << logm)
    rc = load().pst_mul_bitrev_gpu(_p(xb), None, _p(sb), logm, np_, _p(y))
    assert rc == 0, rc
    return ints(y)


def ab_bitrev_gpu(a, b, logm, np_):
    assert len(a) == len(b) == np_ << logm
    ab, bb, y = words(a), words(b), _out(np_ << logm)
    rc = load().pst_mul_bitrev_gpu(_p(ab), _p(bb), None, logm, np_, _p(y))
    assert rc == 0, rc
    return ints(y)


def ab_eval_gpu(a, b, scale, n, np_, y_stride, marker=MARKER):
    """-> y, np_ * y_stride raw words (the gaps hold marker bytes)"""
    assert len(a) == len(b) == np_ * n
    ab, bb, sb, y = words(a), words(b), words([scale]), _out(np_ * y_stride)
    rc = load().pst_ab_eval_gpu(_p(ab), _p(bb), _p(sb), n, np_, _p(y), y_stride, marker)
    assert rc == 0, rc
    return ints(y)


def fr_scale_gpu(x, scale, n, np_, y_stride, c=None, cscale=None, marker=MARKER):
    """k_fr_scale, or k_fr_scale_sub when c and cscale are given -> y, np_ * (y_stride or n) raw words"""
    assert len(x) == np_ * n and len(scale) == n and (c is None) == (cscale is None)
    xb, sb, y = words(x), words(scale), _out(np_ * (y_stride or n))
    cb, csb = (words(c), words([cscale])) if c is not None else (None, None)
    rc = load().pst_fr_scale_gpu(_p(xb), _p(sb), _p(cb), _p(csb), n, np_, _p(y), y_stride, marker)
    assert rc == 0, rc
    return ints(y)
