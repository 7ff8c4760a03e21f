"""Loader of the test-only unit tests/native/setup_dev.hip (the parameter-generation kernels of masp_amd/csrc/device/setup.hpp, the
MSM tables' base import and the loader's single-point imports, each launched on its own), with the product's flags as native_build.py reads
them from the Makefile.
Everything that goes in or comes out is plain: scalars as ints below r, points as affine pairs of ints with None for the identity
(tests/pyref.py), or as raw wire bytes where the encoding itself is under test.  Every function checks that the guard slots behind the
kernel's output still hold the byte 0xA5 the unit filled them with."""
import ctypes as C

import native_build
from groth16_shim import g1_point, g2_point
from pyref import g1_unc, g2_unc

UNIT = native_build.unit("setup_dev")
_lib = None

POISON, ZERO = "poison", "zero"
TAB = 32 * 255


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.sd_guard_slots.restype = C.c_uint32
    return _lib


def _check(rc):
    """0, or the test fails; a HIP error (the unit's codes -2 .. -4) ends the whole session: nothing more is started on a device that faulted"""
    if rc in (-2, -3, -4):
        import pytest
        pytest.exit("HIP error %d in tests/native/setup_dev.hip" % rc, returncode=3)
    assert rc == 0, rc


def guard_slots():
    return load().sd_guard_slots()


def _fr(x):
    return int(x).to_bytes(32, "little")


def _frs(xs):
    return b"".join(_fr(x) for x in xs)


def _u32s(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def _fr_call(fn, n, *args):
    """fn(*args, out, guard) -> n ints; the guard slots must be untouched"""
    out, guard = C.create_string_buffer(32 * max(1, n)), C.create_string_buffer(32 * guard_slots())
    _check(fn(*args, out, guard))
    if n:
        assert guard.raw == b"\xa5" * len(guard.raw), "written behind the end of the output"
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]


# ---- the kernels ----
def lagrange(nrows, omega, tau, z_over_m):
    return _fr_call(load().sd_lagrange, nrows, nrows, _fr(omega), _fr(tau), _fr(z_over_m))


def qap(columns, lag, n_inputs, n_constraints, is_a):
    """columns: per variable a list of (row, coefficient), in the order the kernel is to read them"""
    colptr, rowidx, coef = [0], [], []
    for col in columns:
        for row, c in col:
            rowidx.append(row)
            coef.append(c)
        colptr.append(len(rowidx))
    nv = len(columns)
    return _fr_call(load().sd_qap, nv, _u32s(colptr), _u32s(rowidx), _frs(coef), _frs(lag), len(lag), nv, n_inputs, n_constraints, 1 if is_a else 0)


def lc(at, bt, ct, alpha, beta, scale):
    n = len(at)
    assert len(bt) == len(ct) == n
    return _fr_call(load().sd_lc, n, _frs(at), _frs(bt), _frs(ct), n, _fr(alpha), _fr(beta), _fr(scale))


def nonzero(xs):
    n = len(xs)
    flags = C.create_string_buffer(n + guard_slots())
    _check(load().sd_nonzero(_frs(xs), n, flags))
    if n:
        assert flags.raw[n:] == b"\xa5" * guard_slots(), "written behind the end of the flags"
    return list(flags.raw[:n])


def gather(src, idx):
    return _fr_call(load().sd_gather, len(idx), _frs(src), len(src), _u32s(idx), len(idx))


def h_scalars(tau, c, n):
    return _fr_call(load().sd_h_scalars, n, _fr(tau), _fr(c), n)


def _curve(curve):
    return (96, g1_unc, g1_point) if curve == "g1" else (192, g2_unc, g2_point)


def fixed_table(curve, gen):
    """k_setup_fixed_table -> table[w][d - 1] as affine points"""
    width, unc, conv = _curve(curve)
    slots = TAB + guard_slots()
    out, state = C.create_string_buffer(width * slots), C.create_string_buffer(slots)
    _check((load().sd_fixed_table_g1 if curve == "g1" else load().sd_fixed_table_g2)(unc(gen), out, state))
    assert state.raw[:TAB] == bytes(TAB), "an entry that is still the poison, or all zero"
    assert state.raw[TAB:] == b"\x01" * guard_slots(), "written behind the end of the table"
    flat = [conv(out.raw[width * i:width * i + width]) for i in range(TAB)]
    return [flat[255 * w:255 * w + 255] for w in range(32)]


def fixed_mul(curve, gen, scalars, mont):
    """k_setup_fixed_mul over the table of gen -> the points' wire bytes, one per scalar"""
    width, unc, _ = _curve(curve)
    n = len(scalars)
    out, guard = C.create_string_buffer(width * max(1, n)), C.create_string_buffer(width * guard_slots())
    _check((load().sd_fixed_mul_g1 if curve == "g1" else load().sd_fixed_mul_g2)(unc(gen), _frs(scalars), n, 1 if mont else 0, out, guard))
    if n:
        assert guard.raw == b"\xa5" * len(guard.raw), "written behind the end of the output"
    return [out.raw[width * i:width * i + width] for i in range(n)]


def _rows(raw, state, width, conv):
    out = []
    for i, st in enumerate(state):
        out.append(POISON if st == 1 else ZERO if st == 2 else conv(raw[width * i:width * i + width]))
    return out


def msm_import(curve, encodings):
    """k_msm_import over wire encodings -> (rows: a point, ZERO for the all-zero row or POISON, the status word)"""
    width, _, conv = _curve(curve)
    n = len(encodings)
    assert all(len(e) == width for e in encodings)
    slots = n + guard_slots()
    out, state, status = C.create_string_buffer(width * slots), C.create_string_buffer(slots), C.c_int(-1)
    _check((load().sd_msm_import_g1 if curve == "g1" else load().sd_msm_import_g2)(b"".join(encodings), n, out, state, C.byref(status)))
    rows = _rows(out.raw, state.raw[:slots], width, conv)
    if n:
        assert rows[n:] == [POISON] * guard_slots(), "written behind the end of the table"
    return rows[:n], status.value


def import_one(curve, encoding):
    """k_g1_import_one / k_g2_import_one -> (the slot: a point, ZERO or POISON, the status word)"""
    width, _, conv = _curve(curve)
    assert len(encoding) == width
    slots = 1 + guard_slots()
    out, state, status = C.create_string_buffer(width * slots), C.create_string_buffer(slots), C.c_int(-1)
    _check((load().sd_import_one_g1 if curve == "g1" else load().sd_import_one_g2)(encoding, out, state, C.byref(status)))
    rows = _rows(out.raw, state.raw[:slots], width, conv)
    assert rows[1:] == [POISON] * guard_slots(), "written behind the slot"
    return rows[0], status.value
