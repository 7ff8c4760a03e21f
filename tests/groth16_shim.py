"""Loader of the test-only unit tests/native/groth16_dev.hip (the proof-assembly kernels of masp_amd/csrc/device/groth16.hpp, each
launched on its own through the product's launch_* wrapper), with the product's flags as native_build.py reads them from the Makefile.
Everything that goes in or comes out is plain: points as affine pairs of ints with None for the identity (tests/pyref.py), scalars as
ints.  A point that stands for an MSM result or an assembly piece is a WithZ(point, z): it is uploaded as (x z^2, y z^3, z^2, z^3); a bare
point means z = 1.  An XYZZ slot comes back as a point, or as POISON where it still holds the byte 0xA5 the unit filled it with; a slot
that holds neither raises."""
import collections
import ctypes as C

import native_build
from pyref import g1_unc, g2_unc

UNIT = native_build.unit("groth16_dev")
_lib = None

POISON = "poison"
WithZ = collections.namedtuple("WithZ", "p z")      # z: an int below p for G1, a pair of them (c0, c1) for G2; never zero
TAB = 32 * 255


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.g16_guard_slots.restype = C.c_uint32
        _lib.g16_tab_row_stride.restype = C.c_uint32
    return _lib


def _check(rc):
    """0, or the test fails; a HIP error (the unit's codes -2 .. -4) ends the whole session: nothing more is started on a device that faulted"""
    if rc in (-2, -3, -4):
        import pytest
        pytest.exit("HIP error %d in tests/native/groth16_dev.hip" % rc, returncode=3)
    assert rc == 0, rc


def guard_slots():
    return load().g16_guard_slots()


def tab_row_stride():
    """bytes between the rows of the loader's a / b_g1 tables, which k_g1_subgroup_flag walks"""
    return load().g16_tab_row_stride()


# ---- wire forms ----
def g1_point(b):
    assert len(b) == 96
    if b[0] & 0x40:
        assert b == b"\x40" + bytes(95), b.hex()
        return None
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def g2_point(b):
    assert len(b) == 192
    if b[0] & 0x40:
        assert b == b"\x40" + bytes(191), b.hex()
        return None
    c = [int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(4)]
    return ((c[1], c[0]), (c[3], c[2]))


def _slots(raw, state, width, conv):
    out = []
    for i, st in enumerate(state):
        assert st in (0, 1), "slot %d holds neither a point nor the poison" % i
        out.append(POISON if st else conv(raw[width * i:width * i + width]))
    return out


def _g1_slots(slots):
    """[WithZ(point, z) or point] -> (96-byte forms, 48-byte zs)"""
    pts, zs = [], []
    for s in slots:
        p, z = s if isinstance(s, WithZ) else (s, 1)
        pts.append(g1_unc(p))
        zs.append(int(z).to_bytes(48, "big"))
    return b"".join(pts), b"".join(zs)


def _g2_slots(slots):
    """[WithZ(point, (z0, z1)) or point] -> (192-byte forms, 96-byte zs: c0 | c1)"""
    pts, zs = [], []
    for s in slots:
        p, z = s if isinstance(s, WithZ) else (s, (1, 0))
        pts.append(g2_unc(p))
        zs.append(int(z[0]).to_bytes(48, "big") + int(z[1]).to_bytes(48, "big"))
    return b"".join(pts), b"".join(zs)


def rs_rows(pairs, rs_stride):
    """(r, s) per proof -> rows of rs_stride 32-bit words: r in words 0..7, s in 8..15, the byte 0xA5 in the rest"""
    assert rs_stride >= 16
    return b"".join(int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little") + b"\xa5" * (4 * (rs_stride - 16)) for r, s in pairs)


# ---- the kernels ----
def fixed_table(curve, points):
    """k_fixed_table_xyzz: bases -> (tables[k][w][d - 1] as affine points, the guard slots behind the last table)"""
    n = len(points)
    lib, width, unc, conv = (load().g16_fixed_table_g1, 96, g1_unc, g1_point) if curve == "g1" else (load().g16_fixed_table_g2, 192, g2_unc, g2_point)
    slots = n * TAB + guard_slots()
    out, state = C.create_string_buffer(width * slots), C.create_string_buffer(slots)
    rc = lib(b"".join(unc(p) for p in points), n, out, state)
    _check(rc)
    flat = _slots(out.raw, state.raw[:slots], width, conv)
    tabs = [[flat[k * TAB + w * 255:k * TAB + (w + 1) * 255] for w in range(32)] for k in range(n)]
    return tabs, flat[n * TAB:]


def fixed_g1(points3, pairs, rs_stride):
    """k_groth16_fixed_g1 over the tables of (delta1, alpha1, beta1) -> part: 6 slots per proof, then the guard slots"""
    assert len(points3) == 3
    np_ = len(pairs)
    slots = 6 * np_ + guard_slots()
    out, state = C.create_string_buffer(96 * slots), C.create_string_buffer(slots)
    rc = load().g16_fixed_g1(b"".join(g1_unc(p) for p in points3), rs_rows(pairs, rs_stride), rs_stride, np_, out, state)
    _check(rc)
    return _slots(out.raw, state.raw[:slots], 96, g1_point)


def fixed_g2(point, pairs, rs_stride):
    """k_groth16_fixed_g2 over the table of delta2 -> part2: a slot per proof, then the guard slots"""
    np_ = len(pairs)
    slots = np_ + guard_slots()
    out, state = C.create_string_buffer(192 * slots), C.create_string_buffer(slots)
    rc = load().g16_fixed_g2(g2_unc(point), rs_rows(pairs, rs_stride), rs_stride, np_, out, state)
    _check(rc)
    return _slots(out.raw, state.raw[:slots], 192, g2_point)


def endo_split(ks):
    """the product's endo_split, one lane per scalar -> [(q, rem)]"""
    n = len(ks)
    q, rem = C.create_string_buffer(16 * n), C.create_string_buffer(16 * n)
    rc = load().g16_endo_split(b"".join(int(k).to_bytes(32, "little") for k in ks), n, q, rem)
    _check(rc)
    return [(int.from_bytes(q.raw[16 * i:16 * i + 16], "little"), int.from_bytes(rem.raw[16 * i:16 * i + 16], "little")) for i in range(n)]


def var_mul(which, msm_g1, pairs, rs_stride, endo):
    """k_groth16_var_mul: msm_g1 = 4 slots per proof (H, L, A, B1) -> part: 6 slots per proof, then the guard slots"""
    np_ = len(pairs)
    assert len(msm_g1) == 4 * np_
    pts, zs = _g1_slots(msm_g1)
    slots = 6 * np_ + guard_slots()
    out, state = C.create_string_buffer(96 * slots), C.create_string_buffer(slots)
    rc = load().g16_var_mul(which, pts, zs, rs_rows(pairs, rs_stride), rs_stride, np_, 1 if endo else 0, out, state)
    _check(rc)
    return _slots(out.raw, state.raw[:slots], 96, g1_point)


def subgroup_flag(points, stride_bytes, flag_in=0):
    """k_g1_subgroup_flag over affine points stride_bytes apart; the flag word before -> the flag word after"""
    flag = C.c_int(-1)
    rc = load().g16_subgroup_flag(b"".join(g1_unc(p) for p in points), len(points), stride_bytes, flag_in, C.byref(flag))
    _check(rc)
    return flag.value


FINISH_B, FINISH_AC, FINISH_AC_EARLY, FINISH_C_LATE = 0, 1, 2, 3


def finish(mode, alpha1, beta2, part, part2, msm_g1, msm_g2):
    """one finishing kernel.  part: 6 slots per proof, part2: 1, msm_g1: 4 (H, L, A, B1), msm_g2: 1 (B2)
    -> (the proofs' 192 bytes each, the 192 bytes behind the last proof, part as the kernel left it with its guard slots)"""
    np_ = len(part2)
    assert len(part) == 6 * np_ and len(msm_g1) == 4 * np_ and len(msm_g2) == np_
    p1, z1 = _g1_slots(part)
    p2, z2 = _g2_slots(part2)
    m1, mz1 = _g1_slots(msm_g1)
    m2, mz2 = _g2_slots(msm_g2)
    slots = 6 * np_ + guard_slots()
    proof = C.create_string_buffer(192 * (np_ + 1))
    out, state = C.create_string_buffer(96 * slots), C.create_string_buffer(slots)
    rc = load().g16_finish(mode, g1_unc(alpha1), g2_unc(beta2), p1, z1, p2, z2, m1, mz1, m2, mz2, np_, proof, out, state)
    _check(rc)
    raw = proof.raw
    return [raw[192 * i:192 * i + 192] for i in range(np_)], raw[192 * np_:192 * np_ + 192], _slots(out.raw, state.raw[:slots], 96, g1_point)
