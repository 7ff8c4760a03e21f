"""The final exponentiation of the GPU per-proof verifier is a set of levelled straight-line programs (masp_amd/csrc/host/pairing_prog.h:
product, squaring, Frobenius, Frobenius^2, the two halves of the inversion) under one driver that the device kernel k_final_exp shares.
masp_host_final_exp_program_selftest runs them on the host interpreter in the kernel's order; here its output is compared with plain
square-and-multiply by the integer 3 (p^12 - 1) / r in the tests' own schoolbook tower (tests/verify_ref.py) — no GPU needed."""
import ctypes as C

import pytest

import oracle_lib as O
import verify_shim as VS
from pyref import F1, P, R, ec_mul, g1_unc
from verify_ref import FP12_ONE, fp12_mul

EXPONENT = 3 * (P ** 12 - 1) // R
assert 3 * (P ** 12 - 1) % R == 0


def fp12_pow(f, e):
    r = None
    for bit in bin(e)[2:]:
        if r is not None:
            r = fp12_mul(r, r)
        if bit == "1":
            r = f if r is None else fp12_mul(r, f)
    return r


def selftest(f):
    """-> (return code, result as a 12-tuple, stats)"""
    from masp_amd import host as H
    L = H.load_library()
    L.masp_host_final_exp_program_selftest.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]
    out, st = C.create_string_buffer(576), (C.c_uint32 * 32)()
    rc = L.masp_host_final_exp_program_selftest(VS.fp12_bytes(f), out, st)
    return rc, VS.fp12_tuple(out.raw), list(st)


def miller_values():
    """Miller values of two random pairs, and of (P, Q) and (-P, Q)"""
    pairs = []
    for k in (0x1234567 ** 5 % R, R - 5):
        p, _ = O.g1_mul_gen(k)
        q, _ = O.g2_mul_gen((3 * k + 1) % R)
        pairs.append((bytes(p), bytes(q)))
    p, q = pairs[0]
    x, y = int.from_bytes(p[:48], "big"), int.from_bytes(p[48:], "big")
    pairs.append((g1_unc((x, P - y)), q))
    return VS.miller_host(pairs)


@pytest.fixture(scope="module")
def values():
    return miller_values()


@pytest.mark.parametrize("which", [0, 1])
def test_programs_give_the_power_3_p12_minus_1_over_r_of_a_miller_value(values, which):
    rc, got, _ = selftest(values[which])
    assert rc == 0                                                   # equal to the library's own final_exp
    assert got == fp12_pow(values[which], EXPONENT) and got != FP12_ONE


def test_one_goes_to_one_and_a_pairing_times_its_inverse_goes_to_one(values):
    assert selftest(FP12_ONE)[:2] == (0, FP12_ONE)
    f = fp12_mul(values[0], values[2])                               # ML(P, Q) ML(-P, Q)
    assert f != FP12_ONE
    rc, got, _ = selftest(f)
    assert rc == 0 and got == FP12_ONE and fp12_pow(f, EXPONENT) == FP12_ONE


def test_zero_takes_the_branch_in_front_of_the_inversion():
    rc, got, _ = selftest((0,) * 12)
    assert rc == 2 and got == (0,) * 12                              # verdict "invalid"; the inverse never saw zero
    rc, _, _ = selftest((P,) + (0,) * 11)
    assert rc == -1


def test_programs_fit_the_interpreter():
    _, _, st = selftest(FP12_ONE)
    progs = {n: st[5 * i:5 * i + 5] for i, n in enumerate(("mul", "sq", "frob", "frob2", "inv1", "inv2"))}
    # [ops, steps, steps with products, products, slots]
    assert progs["mul"][3] == 54 and progs["mul"][2] == 1 and progs["sq"][3] == 36 and progs["sq"][2] == 1
    assert progs["frob"][3] == 15 and progs["frob2"][3] == 10
    assert st[30] == max(p[4] for p in progs.values()) and st[30] <= 1024          # slot numbers are 10 bits
    assert st[31] == 48 * st[30] and st[31] <= 65536                                # LDS of one wavefront's interpreter
