"""Edge points and scalars for the stage tests of the proof-assembly kernels (tests/test_gpu_groth16_stages.py), built once with
tests/pyref.py alone and checked on the CPU by tests/test_groth16_stage_cases.py.  Points are affine pairs of ints, None the identity."""
import functools
import random

from pyref import F1, F2, G1, G2, P, R, ec_add, ec_mul

# orders of the curves: E(Fp) = H1 * R, E'(Fp2) = H2 * R
H1 = 0x396c8c005555e1568c00aaab0000aaab
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
assert H1 % 3 == 0 and H1 % 11 == 0 and H2 % 169 == 0 and H2 % 23 == 0
U_SQR = 0xd201000000010000 ** 2      # the divisor of the product's endo_split
assert 2 ** 127 < U_SQR < 2 ** 128
B2 = (4, 4)                          # the twist: y^2 = x^3 + 4 (1 + u)


def neg(F, p):
    return None if p is None else (p[0], F.neg(p[1]))


def on_curve(F, p):
    b = 4 if F is F1 else B2
    return p is None or F.mul(p[1], p[1]) == F.add(F.mul(F.mul(p[0], p[0]), p[0]), b)


def fp_sqrt(a):
    """a square root of a in Fp (p = 3 mod 4), or None"""
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def fp2_sqrt(a):
    """a square root of a = (a0, a1) in Fp2 = Fp[u] / (u^2 + 1), or None"""
    if a[1] == 0:
        s = fp_sqrt(a[0])
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a[0] % P)
        return (0, s)
    n = fp_sqrt((a[0] * a[0] + a[1] * a[1]) % P)
    if n is None:
        return None
    half = pow(2, -1, P)
    for t in ((a[0] + n) * half % P, (a[0] - n) * half % P):
        x0 = fp_sqrt(t)
        if x0:
            x = (x0, a[1] * pow(2 * x0, -1, P) % P)
            if F2.mul(x, x) == (a[0] % P, a[1] % P):
                return x
    return None


def g1_with_x(x):
    y = fp_sqrt((x * x * x + 4) % P)
    return None if y is None else (x, y)


def g2_with_x(x):
    y = fp2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), B2))
    return None if y is None else (x, y)


def _first(gen):
    return next(p for p in gen if p is not None)


def of_prime_order(F, n, ell, candidates):
    """A point of order ell exactly, from the first candidate that has a part of ell-power order: the candidate times n / ell^v (n the order of
    the curve, ell^v the whole power of ell in it) has order ell^j, and is multiplied by ell until one more step would give the identity.
    (n / ell alone is not enough where ell^2 divides n and the ell-part of the curve is not cyclic: 11^2 divides H1, and every point times
    H1 R / 11 is the identity.)"""
    m = n
    while m % ell == 0:
        m //= ell
    for p in candidates:
        q = ec_mul(F, p, m) if p is not None else None
        if q is None:
            continue
        while True:
            nxt = ec_mul(F, q, ell)
            if nxt is None:
                return q
            q = nxt
    raise AssertionError("no point of order %d" % ell)


# ---- G1 ----
T3 = (0, 2)                                                      # order 3, x = 0
NEG_T3 = neg(F1, T3)
ORD11 = of_prime_order(F1, H1 * R, 11, (g1_with_x(x) for x in range(1, 200)))


@functools.lru_cache(maxsize=None)
def g1_mul(k):
    return ec_mul(F1, G1, k % R)


@functools.lru_cache(maxsize=None)
def g1_3r(k):
    """k G1 + T3: order 3 r"""
    return ec_add(F1, g1_mul(k), T3)


# ---- G2 ----
G2_OUTSIDE = _first(g2_with_x((x, 1)) for x in range(1, 200))     # a twist point with a small x: outside the subgroup (checked on the CPU)
ORD13 = of_prime_order(F2, H2 * R, 13, (g2_with_x((x, 1)) for x in range(1, 200)))


def _c1_zero_point():
    """x = a + 2 u with 3 a^2 b - b^3 = -4 at b = 2 (the u part of x^3 + 4 (1 + u) vanishes) and a^3 - 3 a b^2 + 4 a square in Fp"""
    b = 2
    a = fp_sqrt((b ** 3 - 4) * pow(3 * b, -1, P) % P)
    assert a is not None
    for a in (a, P - a):
        y0 = fp_sqrt((a ** 3 - 3 * a * b * b + 4) % P)
        if y0:
            return ((a, b), (y0, 0))
    raise AssertionError("no twist point with y.c1 = 0 at b = 2")


G2_C1_ZERO = _c1_zero_point()


@functools.lru_cache(maxsize=None)
def g2_mul(k):
    return ec_mul(F2, G2, k % R)


# ---- scalars ----
def one_byte(window, byte=0x5b):
    """a single non-zero byte, in the given 8-bit window"""
    return byte << (8 * window)


RS_EDGES = [
    (0, 0), (1, 1), (0, 1), (1, 0),
    (R - 1, R - 1),                                              # r s = 1
    (R - 1, 1), (0, R - 1),
    (one_byte(0), one_byte(31, 0x73)),                           # a single non-zero byte in window 0 / in window 31 (0x73 << 248 < R)
    (one_byte(31, 0x01), one_byte(0, 0xff)),
    (one_byte(15), one_byte(15, 0xff)),                          # ... in window 15
    (2 ** 248 - 1, 2 ** 248 - 1),                                # 0xff in every byte below the top
    (int.from_bytes(bytes([0x00, 0xc3] * 15 + [0x00, 0x53]), "little"), int.from_bytes(bytes([0x9d, 0x00] * 16), "little")),   # alternating bytes
]
assert all(0 <= r < R and 0 <= s < R for r, s in RS_EDGES)

SPLIT_EDGES = [0, 1, U_SQR - 1, U_SQR, U_SQR + 1, 2 * U_SQR, (R // U_SQR) * U_SQR, R - 1, 2 ** 128 - 1, 2 ** 128, 2 ** 255 - 1]


def split_scalars():
    """the scalars of the endo_split test: the edges and 200 random k below 2^255"""
    rng = random.Random(1601)
    return SPLIT_EDGES + [rng.randrange(2 ** 255) for _ in range(200)]


def split_model(k):
    return divmod(k, U_SQR)


VAR_SMALL = [0, 1, 2, 3, 15, 16, 17, R - 1]                      # scalars for the points of small order (and a random one per test)


# ---- the fixed-base tables ----
def table_model(F, p):
    """tab[w][d - 1] = d 2^(8 w) p by running sums, w < 32, d = 1 .. 255"""
    tab, base = [], p
    for w in range(32):
        row, cur = [], None
        for _ in range(255):
            cur = ec_add(F, cur, base)
            row.append(cur)
        tab.append(row)
        for _ in range(8):
            base = ec_add(F, base, base)
    return tab


def table_sample(seed):
    """(w, d): every d of windows 0 and 31, d = 1, 2, 255 of every window, 40 random places"""
    rng = random.Random(seed)
    s = [(w, d) for w in (0, 31) for d in range(1, 256)] + [(w, d) for w in range(32) for d in (1, 2, 255)]
    return s + [(rng.randrange(32), rng.randrange(1, 256)) for _ in range(40)]
