"""Plain big-integer references for the stages of the Groth16 batch verifiers (device: masp_amd/csrc/device/pairing.hpp, subgroup.hpp; host:
masp_amd/csrc/host/pairing.h), over tests/pyref.py: square roots and zcash point decompression, what bellman's `Proof::read` says about
the encoding of a point (classify_g1 / classify_g2: the device's PT_* status values), and the Fp12 product.  No shortcut the product
takes is taken here: subgroup membership is r * point = O by double-and-add, the tower is multiplied schoolbook."""
import functools

from pyref import F1, F2, P, R, ec_mul

# status values of the device's point readers (masp_amd/csrc/device/io.hpp)
PT_OK, PT_BAD_FLAGS, PT_NOT_CANONICAL, PT_INFINITY, PT_NOT_IN_SUBGROUP = 0, 1, 2, 4, 8
HALF = (P - 1) // 2


def _sqrt_fp(a):
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a else None


def sqrt_fp2_branch(a):
    """-> (a square root of a in Fp2 or None, how it was found): "zero"; "c1=0 square" / "c1=0 non-square" (the root is (s, 0) or (0, s));
    otherwise, with n = (c0^2 + c1^2)^((p+1)/4), "first" if (c0 + n) / 2 is a square and "second" if only (c0 - n) / 2 is."""
    if a == (0, 0):
        return a, "zero"
    a0, a1 = a
    if a1 == 0:
        s = _sqrt_fp(a0)
        if s is not None:
            return (s, 0), "c1=0 square"
        return (0, _sqrt_fp((-a0) % P)), "c1=0 non-square"         # -1 is a non-square: exactly one of a0, -a0 is a square
    n = _sqrt_fp((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None, "none"
    for sg, name in ((n, "first"), ((-n) % P, "second")):
        d = (a0 + sg) * pow(2, -1, P) % P
        x0 = _sqrt_fp(d)
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, P) % P)
            if F2.mul(r, r) == a:
                return r, name
    return None, "none"


def _sqrt_fp2(a):
    return sqrt_fp2_branch(a)[0]


def g1_rhs(x):
    return (x ** 3 + 4) % P


def g2_rhs(x):
    return F2.add(F2.mul(F2.mul(x, x), x), (4, 4))


def fp2_lex_largest(y):
    return (y[1] > HALF) if y[1] else (y[0] > HALF)


def _g1_decompress(b):
    x = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big")
    y = _sqrt_fp(g1_rhs(x))
    if (y > HALF) != bool(b[0] & 0x20):
        y = P - y
    return (x, y)


def _g2_decompress(b):
    x = (int.from_bytes(b[48:96], "big"), int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big"))
    y = _sqrt_fp2(g2_rhs(x))
    if fp2_lex_largest(y) != bool(b[0] & 0x20):
        y = F2.neg(y)
    return (x, y)


def small_order_points():
    """T1 = (0, 2): order 3 on y^2 = x^3 + 4.  T2: a point of the twist outside G2, times r: its order divides the cofactor."""
    t1 = (0, 2)
    assert ec_mul(F1, t1, 3) is None
    x = (2, 0)
    while True:
        y = _sqrt_fp2(g2_rhs(x))
        if y is not None and ec_mul(F2, (x, y), R) is not None:
            break
        x = (x[0] + 1, 0)
    t2 = ec_mul(F2, (x, y), R)
    return t1, t2


# ---- what Proof::read makes of the encoding of one point ----
def _infinity(b):
    return PT_INFINITY if (b[0] & 0x3f) == 0 and not any(b[1:]) else PT_BAD_FLAGS


@functools.lru_cache(maxsize=None)
def classify_g1(b):
    """48 bytes -> PT_*: flags, the encoding of infinity (clean, or stray bits: refused like bad flags), x < p, on the curve (the device
    reports "not on the curve" as PT_BAD_FLAGS too), then membership of the subgroup of order r"""
    b = bytes(b)
    assert len(b) == 48
    if not b[0] & 0x80:
        return PT_BAD_FLAGS
    if b[0] & 0x40:
        return _infinity(b)
    x = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:], "big")
    if x >= P:
        return PT_NOT_CANONICAL
    if _sqrt_fp(g1_rhs(x)) is None:
        return PT_BAD_FLAGS
    return PT_OK if ec_mul(F1, _g1_decompress(b), R) is None else PT_NOT_IN_SUBGROUP


@functools.lru_cache(maxsize=None)
def classify_g2(b):
    b = bytes(b)
    assert len(b) == 96
    if not b[0] & 0x80:
        return PT_BAD_FLAGS
    if b[0] & 0x40:
        return _infinity(b)
    x1, x0 = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big"), int.from_bytes(b[48:], "big")
    if x0 >= P or x1 >= P:
        return PT_NOT_CANONICAL
    if _sqrt_fp2(g2_rhs((x0, x1))) is None:
        return PT_BAD_FLAGS
    return PT_OK if ec_mul(F2, _g2_decompress(b), R) is None else PT_NOT_IN_SUBGROUP


def classify_proof(proof):
    """the status word k_verify_prepare leaves for a proof: the OR of its three points' values"""
    return classify_g1(proof[:48]) | classify_g2(proof[48:144]) | classify_g1(proof[144:])


# ---- Fp12 = Fp6[w] / (w^2 - v), Fp6 = Fp2[v] / (v^3 - (1 + u)), Fp2 = Fp[u] / (u^2 + 1) ----
XI = (1, 1)
FP12_ONE = (1,) + (0,) * 11


def _fp6_mul(a, b):
    m = F2.mul
    c0 = F2.add(m(a[0], b[0]), m(XI, F2.add(m(a[1], b[2]), m(a[2], b[1]))))
    c1 = F2.add(F2.add(m(a[0], b[1]), m(a[1], b[0])), m(XI, m(a[2], b[2])))
    c2 = F2.add(F2.add(m(a[0], b[2]), m(a[1], b[1])), m(a[2], b[0]))
    return (c0, c1, c2)


def _fp6_add(a, b):
    return tuple(F2.add(x, y) for x, y in zip(a, b))


def _fp6_mul_v(a):
    return (F2.mul(XI, a[2]), a[0], a[1])


def fp12_mul(a, b):
    """12-tuples of ints in the flat coefficient order of masp_host::bls::Fp12 (a.a.a, a.a.b, a.b.a, ...: the Fp6 halves one after the
    other, in each its three Fp2 coefficients, in each c0 then c1) -> their product"""
    split = lambda f: (tuple((f[2 * i], f[2 * i + 1]) for i in range(3)), tuple((f[6 + 2 * i], f[7 + 2 * i]) for i in range(3)))
    (a0, a1), (b0, b1) = split(a), split(b)
    lo = _fp6_add(_fp6_mul(a0, b0), _fp6_mul_v(_fp6_mul(a1, b1)))
    hi = _fp6_add(_fp6_mul(a0, b1), _fp6_mul(a1, b0))
    return tuple(c for half in (lo, hi) for e in half for c in e)


def fp12_product(vals):
    r = vals[0]
    for v in vals[1:]:
        r = fp12_mul(r, v)
    return r
