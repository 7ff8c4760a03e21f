"""The kernels that write and read a CRS, each on its own: the parameter-generation kernels of masp_amd/csrc/device/setup.hpp, the MSM tables'
base import (k_msm_import) and the loader's single-point imports, launched unchanged by the test-side unit tests/native/setup_dev.hip
(tests/setup_shim.py) on inputs set directly, and compared with tests/setup_model.py and tests/pyref.py — integers and bytes, so equality,
no tolerance anywhere.  End to end these kernels only ever see random toxic waste and random circuits; here they get tau = 0 and r - 2,
empty and cancelling columns, the scalars 0, 1 and r - 1, sizes on both sides of a block, and bad points at known indices.  No input
leaves a buffer: every index is in range, and the unit refuses what is not.  Run with `-m gpu`."""
import functools
import random

import pytest

import setup_model as M
import setup_shim as S
from pyref import F1, F2, G1, G2, P, R, ec_add, ec_mul, g1_unc, g2_unc
from setup_shim import POISON, ZERO
from verify_ref import PT_BAD_FLAGS, PT_INFINITY, PT_NOT_CANONICAL, PT_OK

pytestmark = pytest.mark.gpu


def _mix(rng, n):
    """n scalars: 0, 1 and r - 1 first and last, random ones between"""
    special = [0, 1, R - 1]
    xs = [special[i % 3] if (i < 3 or i >= n - 3 or i % 7 == 0) else rng.randrange(R) for i in range(n)]
    return xs


# ---- k_setup_lagrange ----
@functools.lru_cache(maxsize=None)
def _lagrange_ref(tau, logm):
    return tuple(M.lagrange_at(tau, logm))


def _lagrange_taus(logm):
    return [0, 2, R - 2, (M.omega(logm) + 1) % R, random.Random(0x1a6 + logm).randrange(2, R)]


@pytest.mark.parametrize("logm", [1, 2, 3, 7, 8])
def test_lagrange(logm):
    """lag[k] = l_k(tau) by the inverse transform of the powers of tau, row k <-> w^k, for tau off the domain"""
    m, w = 1 << logm, M.omega(logm)
    rows = (127, 128, 129) if logm == 8 else sorted({1, m - 1, m})
    for tau in _lagrange_taus(logm):
        assert pow(tau, m, R) != 1
        z_over_m = (pow(tau, m, R) - 1) * pow(m, -1, R) % R
        want = _lagrange_ref(tau, logm)
        for nrows in rows:
            assert S.lagrange(nrows, w, tau, z_over_m) == list(want[:nrows]), (logm, nrows, tau)


# ---- k_setup_qap ----
N_CONSTRAINTS, N_INPUTS = 40, 3


def _qap_columns(rng, nv):
    """column v by v mod 8: empty | one entry | the same row twice | coefficients 0, 1, r - 1 | c and r - c on one row | several | one on
    the last row | r - 1 on row 0.  Column 0 is empty: as an input of A its only contribution is the extra row."""
    cols = []
    for v in range(nv):
        row = lambda: rng.randrange(N_CONSTRAINTS)
        kind = v % 8
        if kind == 0:
            col = []
        elif kind == 1:
            col = [(row(), rng.randrange(1, R))]
        elif kind == 2:
            r0 = row()
            col = [(r0, rng.randrange(1, R)), (r0, rng.randrange(1, R))]
        elif kind == 3:
            col = [(row(), 0), (row(), 1), (row(), R - 1)]
        elif kind == 4:
            r0, c = row(), rng.randrange(1, R)
            col = [(r0, c), (r0, R - c)]
        elif kind == 5:
            col = [(row(), rng.randrange(R)) for _ in range(rng.randint(2, 6))]
        elif kind == 6:
            col = [(N_CONSTRAINTS - 1, 1)]
        else:
            col = [(0, R - 1)]
        cols.append(col)
    return cols


@pytest.mark.parametrize("is_a", [0, 1])
@pytest.mark.parametrize("nv", [1, 127, 128, 129])
def test_qap(nv, is_a):
    rng = random.Random(0x9a9 + nv)
    lag = [rng.randrange(1, R) for _ in range(N_CONSTRAINTS + N_INPUTS)]
    cols = _qap_columns(rng, nv)
    want = []
    for v, col in enumerate(cols):
        acc = sum(c * lag[row] for row, c in col)
        if is_a and v < N_INPUTS:
            acc += lag[N_CONSTRAINTS + v]
        want.append(acc % R)
    got = S.qap(cols, lag, N_INPUTS, N_CONSTRAINTS, is_a)
    assert got == want
    assert got[0] == (lag[N_CONSTRAINTS] if is_a else 0)          # the extra row alone, and only for A
    if nv > 4:
        assert got[4] == 0                                        # the cancelling column
        assert got[1] != 0
    if nv == 1:
        # one column, several entries, as the only lane of the launch
        col = [[(5, 3), (5, R - 3), (7, 1), (39, R - 1), (0, 0)]]
        assert S.qap(col, lag, N_INPUTS, N_CONSTRAINTS, is_a) == [(lag[7] - lag[39] + (lag[N_CONSTRAINTS] if is_a else 0)) % R]


# ---- k_setup_nonzero, k_setup_gather, k_setup_lc ----
SIZES = [1, 255, 256, 257]


@pytest.mark.parametrize("n", SIZES)
def test_nonzero(n):
    rng = random.Random(0x202 + n)
    for xs in (_mix(rng, n), [0] * n, [R - 1] * n, [1] * n):
        assert S.nonzero(xs) == [1 if x else 0 for x in xs]


@pytest.mark.parametrize("n", SIZES)
def test_gather(n):
    rng = random.Random(0x6a7 + n)
    src = _mix(rng, 300)
    for idx in ([299 - (k % 300) for k in range(n)],                   # reversed
                [17] * n,                                               # one source for all
                [k // 2 for k in range(n)],                             # pairs
                [rng.randrange(300) for _ in range(n)],
                [0] * (n - 1) + [299]):
        assert S.gather(src, idx) == [src[i] for i in idx]


@pytest.mark.parametrize("n", SIZES)
def test_lc(n):
    """out = (beta at + alpha bt + ct) scale"""
    rng = random.Random(0x1c + n)
    at, bt, ct = _mix(rng, n), _mix(rng, n)[::-1], [rng.choice((0, 1, R - 1, rng.randrange(R))) for _ in range(n)]
    a, b, s = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
    for alpha, beta, scale in ((a, b, s), (0, b, s), (a, 0, s), (a, b, 1), (0, 0, 1), (R - 1, 1, R - 1)):
        want = [(beta * x + alpha * y + z) * scale % R for x, y, z in zip(at, bt, ct)]
        assert S.lc(at, bt, ct, alpha, beta, scale) == want, (alpha, beta, scale)
    # alpha and beta are not interchangeable: a case where swapping them changes every result
    assert S.lc([1] * n, [0] * n, [0] * n, 5, 7, 1) == [7] * n


# ---- k_setup_h_scalars ----
@pytest.mark.parametrize("n", SIZES)
def test_h_scalars(n):
    """out[i] = tau^i c, with 0^0 = 1: h[0] of tau = 0 is c, every other one 0"""
    rng = random.Random(0x45 + n)
    c = rng.randrange(1, R)
    for tau in (0, 1, R - 1, rng.randrange(2, R)):
        want, cur = [], c
        for _ in range(n):
            want.append(cur)
            cur = cur * tau % R
        assert S.h_scalars(tau, c, n) == want, tau
    assert S.h_scalars(0, c, n) == [c] + [0] * (n - 1)
    assert S.h_scalars(2, 0, n) == [0] * n


# ---- k_setup_fixed_table ----
def _table_by_running_sums(F, gen):
    """table[w][d - 1] = d 2^(8 w) gen: 255 additions per window, 8 doublings between windows"""
    tab, base = [], gen
    for w in range(32):
        row, cur = [], None
        for _ in range(255):
            cur = ec_add(F, cur, base)
            row.append(cur)
        tab.append(row)
        for _ in range(8):
            base = ec_add(F, base, base)
    return tab


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_fixed_table(curve):
    F, gen = (F1, G1) if curve == "g1" else (F2, G2)
    got = S.fixed_table(curve, gen)
    want = _table_by_running_sums(F, gen)
    for w in range(32):
        assert got[w] == want[w], w
    assert got[31][254] == ec_mul(F, gen, 255 << 248)          # beyond r: the table does not reduce, and need not
    assert got[0][0] == gen and got[1][0] == ec_mul(F, gen, 256)


def test_fixed_table_other_base():
    base = ec_mul(F1, G1, 0x1234567)
    assert S.fixed_table("g1", base) == _table_by_running_sums(F1, base)


# ---- k_setup_fixed_mul ----
EVERY_BYTE = int.from_bytes(bytes(range(1, 33)), "little")
ALTERNATING = int.from_bytes(bytes(0 if i % 2 == 0 else 0x11 + i for i in range(32)), "little")
ALTERNATING_ODD = int.from_bytes(bytes(0 if i % 2 else 0x11 + i for i in range(32)), "little")
SPECIAL = [0, 1, 255, 256, 1 << 248, R - 1, EVERY_BYTE, ALTERNATING, ALTERNATING_ODD, 255 << 240, R - 2]
assert all(0 <= k < R for k in SPECIAL) and all(b for b in EVERY_BYTE.to_bytes(32, "little"))


@functools.lru_cache(maxsize=None)
def _scalars(n):
    rng = random.Random(0xf1ed)
    return tuple(SPECIAL + [rng.randrange(R) for _ in range(130 - len(SPECIAL))])[:n]


@functools.lru_cache(maxsize=None)
def _mul_bytes(curve, k):
    return g1_unc(M.g1_mul(k)) if curve == "g1" else g2_unc(M.g2_mul(k))


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("curve,n", [("g1", 1), ("g1", 63), ("g1", 64), ("g1", 65), ("g1", 130), ("g2", 1), ("g2", 64), ("g2", 65)])
def test_fixed_mul(curve, n, mont):
    """out[i] = [k_i] G in the wire form, the scalars given canonical or in Montgomery form"""
    gen = G1 if curve == "g1" else G2
    if n == 1:
        for k in SPECIAL + [_scalars(130)[-1]]:                 # every special scalar as the only lane of a launch
            assert S.fixed_mul(curve, gen, [k], mont) == [_mul_bytes(curve, k)], hex(k)
        assert S.fixed_mul(curve, gen, [0], mont)[0] == b"\x40" + bytes(95 if curve == "g1" else 191)
        return
    ks = _scalars(n)
    assert S.fixed_mul(curve, gen, ks, mont) == [_mul_bytes(curve, k) for k in ks]


# ---- k_msm_import, k_g1_import_one, k_g2_import_one ----
@functools.lru_cache(maxsize=None)
def _points(curve):
    """130 distinct points: G, 2 G, 3 G ..."""
    F, gen = (F1, G1) if curve == "g1" else (F2, G2)
    out, cur = [], None
    for _ in range(130):
        cur = ec_add(F, cur, gen)
        out.append(cur)
    return tuple(out)


def _unc(curve, p):
    return g1_unc(p) if curve == "g1" else g2_unc(p)


def _off_curve(curve, p):
    """canonical coordinates, not on the curve"""
    return (p[0], (p[1] + 1) % P) if curve == "g1" else (p[0], ((p[1][0] + 1) % P, p[1][1]))


@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_msm_import(curve, n):
    """one bad point at a time, at the first and last lane of a wave and of the launch: the status word is exactly that point's PT_* bits,
    its row holds (0, 0), every other row its point"""
    pts = _points(curve)[:n]
    good = [_unc(curve, p) for p in pts]
    rows, status = S.msm_import(curve, good)
    assert (rows, status) == (list(pts), PT_OK)
    for pos in sorted({0, 63, 64, n - 1}):
        if pos >= n:
            continue
        for name, enc, want_status in M.bad_encodings(curve, pts[pos]):
            rows, status = S.msm_import(curve, good[:pos] + [enc] + good[pos + 1:])
            assert status == want_status, (name, pos)
            assert rows == list(pts[:pos]) + [ZERO] + list(pts[pos + 1:]), (name, pos)
        # a point off the curve with canonical coordinates is imported as given: bellman's unchecked read (`Parameters::read(_, false)`)
        # checks neither the curve equation nor the subgroup, and neither does the loader
        q = _off_curve(curve, pts[pos])
        rows, status = S.msm_import(curve, good[:pos] + [_unc(curve, q)] + good[pos + 1:])
        assert (rows, status) == (list(pts[:pos]) + [q] + list(pts[pos + 1:]), PT_OK), pos


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_msm_import_status_is_the_or(curve):
    """several bad points of different kinds in one launch: the OR of their bits, nothing else"""
    pts = _points(curve)
    bad = {name: (enc, st) for name, enc, st in M.bad_encodings(curve, pts[3])}
    for names in (("infinity", "flag 0x80"), ("infinity", "flag 0x20"), ("flag 0x80", "flag 0x20"), ("infinity", "flag 0x80", "flag 0x20")):
        encs = [_unc(curve, p) for p in pts]
        want_rows, want = list(pts), 0
        for j, name in enumerate(names):
            pos = (0, 64, 129)[j]
            encs[pos] = bad[name][0]
            want_rows[pos] = ZERO
            want |= bad[name][1]
        assert S.msm_import(curve, encs) == (want_rows, want), names
    assert PT_INFINITY | PT_BAD_FLAGS | PT_NOT_CANONICAL == 7


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_import_one(curve):
    """the loader's reader of a verifying-key member: the status of the encoding; a good point (on the curve or not) as given, the identity
    as (0, 0)"""
    p = _points(curve)[6]
    assert S.import_one(curve, _unc(curve, p)) == (p, PT_OK)
    q = _off_curve(curve, p)
    assert S.import_one(curve, _unc(curve, q)) == (q, PT_OK)          # unchecked read, as above
    for name, enc, want_status in M.bad_encodings(curve, p):
        slot, status = S.import_one(curve, enc)
        assert status == want_status, name
        assert slot == (ZERO if want_status == PT_INFINITY else POISON), name      # a refused encoding writes nothing
