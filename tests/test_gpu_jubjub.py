"""masp_hip_jubjub_msm (k_redjubjub.hip, device/jubjub.hpp) against libmasp_host's Jubjub: sums at several sizes over scalars and points
that exercise every case of the group law (the identity, P + (-P), P + P, small-order points), the round trip of every canonical
encoding through device decoding and encoding, and the refusals of JPoint::from_bytes with the index of the first bad point.
Run with `-m gpu`."""
import random

import pytest

from masp_amd import host as H
from masp_amd.hip import Context, MaspHipError

pytestmark = pytest.mark.gpu
Q, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
ORDER = 8 * RJ                     # the order of the whole curve group: [ORDER] P = O for every point
IDENTITY = H.JUBJUB_IDENTITY
G = H.point_bytes(*H.generator_uv(4))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _neg(p):
    return H.jubjub_add(IDENTITY, p, subtract=True)


def _decodes(enc):
    try:
        H.point_uv(enc)
        return True
    except ValueError:
        return False


def _order8_point():
    for v in range(2, 1000):
        e = v.to_bytes(32, "little")
        if _decodes(e):
            t = H.jubjub_mul(e, RJ)                     # the torsion component of a curve point
            if H.jubjub_mul(t, 4) != IDENTITY:
                return t
    raise AssertionError("no point of order 8 found")


def _special_points():
    """the identity, (0, -1) of order 2, (+-sqrt(-1), 0) of order 4 (v = 0, both signs), a point of order 8"""
    return [IDENTITY, (Q - 1).to_bytes(32, "little"), (0).to_bytes(32, "little"), (1 << 255).to_bytes(32, "little"), _order8_point()]


def _scalars(rng, n):
    fixed = [0, 1, RJ - 1, (1 << 256) - 1]
    return [fixed[i] if i < len(fixed) else (rng.getrandbits(128) if i % 2 else rng.getrandbits(256)) for i in range(n)]


def _expected(points, scalars):
    """sum over the distinct points of [sum of their scalars mod the group order] P, on the host"""
    per = {}
    for p, k in zip(points, scalars):
        per[p] = (per.get(p, 0) + k) % ORDER
    return H.jubjub_sum([H.jubjub_mul(p, k) for p, k in per.items()])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70000])
def test_msm_matches_the_host(ctx, n):
    rng = random.Random(n)
    pool = [H.jubjub_mul(G, rng.randrange(1, RJ)) for _ in range(min(n, 200))]
    pool += [_neg(pool[0])] + _special_points()          # P and -P, small order, identity
    points = [pool[0]] + [pool[rng.randrange(len(pool))] for _ in range(n - 1)]
    if n >= 8:
        points[1:8] = [pool[0], pool[-6]] + _special_points()        # P + P, P + (-P), every special point
    scalars = _scalars(rng, n)
    assert ctx.jubjub_msm(points, scalars) == _expected(points, scalars)


def test_single_point_scalar_cases(ctx):
    rng = random.Random(3)
    p = H.jubjub_mul(G, rng.randrange(1, RJ))
    for k in [0, 1, 2, RJ - 1, RJ, RJ + 1, rng.getrandbits(128), rng.getrandbits(256), (1 << 256) - 1]:
        assert ctx.jubjub_msm([p], [k]) == H.jubjub_mul(p, k % RJ), k
    assert ctx.jubjub_msm([], []) == IDENTITY
    assert ctx.jubjub_msm([p, _neg(p)], [5, 5]) == IDENTITY


def test_every_canonical_encoding_round_trips(ctx):
    rng = random.Random(4)
    encs = _special_points() + [H.jubjub_mul(G, rng.randrange(1, RJ)) for _ in range(40)]
    encs += [_neg(e) for e in encs]
    v = 2
    while len(encs) < 120:                                # points outside the prime-order subgroup too
        e = v.to_bytes(32, "little")
        if _decodes(e):
            encs += [e, _neg(e)]
        v += 1
    for e in encs:
        assert ctx.jubjub_msm([e], [1]) == e, e.hex()


def _bad_encodings():
    nonsq = next(v for v in range(2, 1000) if not _decodes(v.to_bytes(32, "little")))
    return {"v = q": Q.to_bytes(32, "little"), "v > q": (Q + 7).to_bytes(32, "little"), "non-square": nonsq.to_bytes(32, "little"),
            "negative zero (identity)": (1 | (1 << 255)).to_bytes(32, "little"),
            "negative zero (0, -1)": ((Q - 1) | (1 << 255)).to_bytes(32, "little")}


def test_refusals_name_the_first_bad_point(ctx):
    rng = random.Random(5)
    good = [H.jubjub_mul(G, rng.randrange(1, RJ)) for _ in range(64)]
    for name, bad in _bad_encodings().items():
        assert not _decodes(bad), name                   # the host refuses it too
        for k in (0, 37, 63):
            pts = list(good)
            pts[k] = bad
            with pytest.raises(MaspHipError) as e:
                ctx.jubjub_msm(pts, [1] * len(pts))
            assert e.value.code == 9 and e.value.bad_index == k, (name, k)
    pts = list(good)
    pts[10] = pts[50] = _bad_encodings()["non-square"]
    with pytest.raises(MaspHipError) as e:
        ctx.jubjub_msm(pts, [1] * len(pts))
    assert e.value.bad_index == 10
