"""Inputs of the verifier stage tests (tests/test_verify_ref.py on the CPU, tests/test_gpu_verify_stages.py on the GPU): encodings of
BLS12-381 points crafted to reach every status of the point readers and every branch of the Fp2 square root, the batch of proofs
k_verify_prepare is run on, and proofs of a toy circuit re-encoded with a non-canonical coordinate.  Built once per process."""
import functools
import random

import numpy as np

import oracle_lib as O
import toy_r1cs
from pyref import F1, F2, P, R, ec_add, ec_mul, g1_comp, g1_unc, g2_comp, g2_unc
from verify_ref import (PT_BAD_FLAGS, PT_INFINITY, PT_NOT_CANONICAL, PT_NOT_IN_SUBGROUP, PT_OK, _g1_decompress, _g2_decompress, _sqrt_fp,
                        _sqrt_fp2, classify_g1, classify_g2, fp2_lex_largest, g1_rhs, g2_rhs, small_order_points, sqrt_fp2_branch)

ROOM = (1 << 381) - P          # a coordinate below this can be written as coordinate + p in the 381 bits the encoding has


def fr32(k):
    return np.frombuffer((k % R).to_bytes(32, "little"), np.uint8)


def g1_points(ks):
    """k * G1 as (x, y) through the oracle"""
    raw = O.g1_mul_gen_many(np.stack([fr32(k) for k in ks]))
    return [(int.from_bytes(r[:48].tobytes(), "big"), int.from_bytes(r[48:].tobytes(), "big")) for r in raw]


def g2_points(ks):
    raw = O.g2_mul_gen_many(np.stack([fr32(k) for k in ks]))
    w = lambda r, i: int.from_bytes(r[48 * i:48 * i + 48].tobytes(), "big")
    return [((w(r, 1), w(r, 0)), (w(r, 3), w(r, 2))) for r in raw]


def _enc1(x, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags
    return bytes(b)


def _enc2(x, flags=0x80):
    b = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags
    return bytes(b)


def _clear_flag(b):
    return bytes([b[0] & 0x7f]) + b[1:]


def _infinities(n):
    return [("clean infinity", bytes([0xc0]) + bytes(n - 1), PT_INFINITY), ("infinity with the sort flag", bytes([0xe0]) + bytes(n - 1), PT_BAD_FLAGS),
            ("infinity with a stray low byte", bytes([0xc0]) + bytes(n - 2) + b"\x01", PT_BAD_FLAGS)]


@functools.lru_cache(maxsize=None)
def g1_cases():
    """[(name, 48 bytes, the status the construction aims at or None where only classify_g1 can tell)]"""
    rng = random.Random(41)
    t1, _ = small_order_points()
    pt = next(p for p in g1_points([rng.randrange(1, R) for _ in range(40)]) if p[0] < ROOM)
    good = g1_comp(pt)
    off = pt[0] + 1
    while _sqrt_fp(g1_rhs(off)) is not None:
        off += 1
    near = P - 1
    while _sqrt_fp(g1_rhs(near)) is None:
        near -= 1
    while True:                                                   # a curve point outside G1: the cofactor is ~2^126, so the first one
        x = rng.randrange(P)
        if _sqrt_fp(g1_rhs(x)) is not None and ec_mul(F1, (x, _sqrt_fp(g1_rhs(x))), R) is not None:
            break
    return [("compression flag clear", _clear_flag(good), PT_BAD_FLAGS), ("x not on the curve", _enc1(off), PT_BAD_FLAGS),
            ("x + p", _enc1(pt[0] + P, good[0] & 0xe0), PT_NOT_CANONICAL), ("x = p", _enc1(P), PT_NOT_CANONICAL),
            ("the largest x on the curve", _enc1(near), None)] + _infinities(48) + \
        [("point + T (order 3)", g1_comp(ec_add(F1, pt, t1)), PT_NOT_IN_SUBGROUP), ("random curve point outside G1", _enc1(x, 0xa0), PT_NOT_IN_SUBGROUP)]


def _random_twist_point(rng):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        if _sqrt_fp2(g2_rhs(x)) is not None:
            return x


@functools.lru_cache(maxsize=None)
def g2_cases():
    rng = random.Random(42)
    _, t2 = small_order_points()
    pt = next(q for q in g2_points([rng.randrange(1, R) for _ in range(200)]) if q[0][0] < ROOM and q[0][1] < ROOM)
    good = g2_comp(pt)
    off = (pt[0][0] + 1, pt[0][1])
    while _sqrt_fp2(g2_rhs(off)) is not None:
        off = (off[0] + 1, off[1])
    near = (P - 1, P - 1)
    while _sqrt_fp2(g2_rhs(near)) is None:
        near = (near[0] - 1, near[1])
    x = _random_twist_point(rng)
    assert ec_mul(F2, (x, _sqrt_fp2(g2_rhs(x))), R) is not None
    fl = good[0] & 0xe0
    return [("compression flag clear", _clear_flag(good), PT_BAD_FLAGS), ("x not on the curve", _enc2(off), PT_BAD_FLAGS),
            ("x.c0 + p", _enc2((pt[0][0] + P, pt[0][1]), fl), PT_NOT_CANONICAL), ("x.c1 + p", _enc2((pt[0][0], pt[0][1] + P), fl), PT_NOT_CANONICAL),
            ("x.c0 = p", _enc2((P, pt[0][1]), fl), PT_NOT_CANONICAL), ("x.c1 = p", _enc2((pt[0][0], P), fl), PT_NOT_CANONICAL),
            ("the largest x.c0 on the curve under x.c1 = p - 1", _enc2(near), None)] + _infinities(96) + \
        [("random twist point outside G2", _enc2(x, 0xa0), PT_NOT_IN_SUBGROUP), ("point + T2 (order dividing the cofactor)", g2_comp(ec_add(F2, pt, t2)), PT_NOT_IN_SUBGROUP)]


@functools.lru_cache(maxsize=None)
def g2_sqrt_cases():
    """[(branch of sqrt_fp2_branch, 96 bytes)]: points of the twist (any: the square root comes before the subgroup test) whose y^2
    takes each way through the Fp2 square root, each with both sign flags.  y^2 = x^3 + 4 (1 + u) has c1 = 3 a^2 b - b^3 + 4 at
    x = a + b u, which vanishes for a^2 = (b^3 - 4) / (3 b)."""
    rng = random.Random(43)
    want = {"c1=0 square": 1, "c1=0 non-square": 1, "first": 5, "second": 5}
    xs = []
    while any(want[k] for k in ("c1=0 square", "c1=0 non-square")):
        b = rng.randrange(1, P)
        a = _sqrt_fp((b ** 3 - 4) * pow(3 * b, -1, P) % P)
        if a is None:
            continue
        for x in ((a, b), (P - a, b)):
            rhs = g2_rhs(x)
            assert rhs[1] == 0 and rhs[0] != 0
            kind = sqrt_fp2_branch(rhs)[1]
            if want[kind]:
                want[kind] -= 1
                xs.append((kind, x))
    while want["first"] or want["second"]:
        x = _random_twist_point(rng)
        kind = sqrt_fp2_branch(g2_rhs(x))[1]
        if want.get(kind):
            want[kind] -= 1
            xs.append((kind, x))
    return [(kind, _enc2(x, fl)) for kind, x in xs for fl in (0x80, 0xa0)]


def _neg_comp(p, comp, F):
    return comp((p[0], F.neg(p[1])))


# ---- the batch k_verify_prepare is tested on ----
PREPARE_N = 150
FORCED_BAD = (0, 63, 64, 127, 128, PREPARE_N - 1)      # block edges of the 64-lane launch, the first lane and the last of a partial block


@functools.lru_cache(maxsize=None)
def prepare_batch():
    """-> (proofs, zs, bad): PREPARE_N proofs of 192 bytes, their 16-byte z, and the set of indices whose proof has a crafted point.
    Every crafted point sits in a proof whose other two points are valid, and between two proofs that are valid throughout, except
    where two of FORCED_BAD touch."""
    rng = random.Random(44)
    ks = [rng.randrange(1, R) for _ in range(60)]
    a, b, c = g1_points(ks[:20]), g2_points(ks[20:40]), g1_points(ks[40:])
    valid = [(g1_comp(a[i]) + g2_comp(b[i]) + g1_comp(c[i]), rng.getrandbits(128)) for i in range(20)]
    v0 = valid[0][0]
    valid += [(v0, rng.getrandbits(128) & ~1), (v0, 0), (v0, (1 << 128) - 1)]
    # the other sign of y: every one of the first four triples with its three points negated (valid points again)
    valid += [(_neg_comp(a[i], g1_comp, F1) + _neg_comp(b[i], g2_comp, F2) + _neg_comp(c[i], g1_comp, F1), rng.getrandbits(128)) for i in range(4)]
    assert all(p[0] & 0x20 != q[0] & 0x20 for (p, _), (q, _) in zip(valid[:4], valid[-4:]))
    crafted = []
    for k, (name, enc, _) in enumerate(g1_cases()):
        crafted.append(enc + valid[k % 20][0][48:])                                       # in A
        crafted.append(valid[(k + 7) % 20][0][:144] + enc)                                # in C
    for k, enc in enumerate([e for _, e, _ in g2_cases()] + [e for _, e in g2_sqrt_cases()]):
        p = valid[(k + 3) % 20][0]
        crafted.append(p[:48] + enc + p[144:])                                            # in B
    rng.shuffle(crafted)
    free = [i for i in range(2, PREPARE_N - 2, 2) if i not in FORCED_BAD and i + 1 not in FORCED_BAD and i - 1 not in FORCED_BAD]
    assert len(crafted) <= len(FORCED_BAD) + len(free)
    where = list(FORCED_BAD) + free
    slots = {where[k]: proof for k, proof in enumerate(crafted)}
    proofs, zs, j = [], [], 0
    for i in range(PREPARE_N):
        if i in slots:
            proofs.append(slots[i])
            zs.append(rng.getrandbits(128))
        else:
            proofs.append(valid[j % len(valid)][0])
            zs.append(valid[j % len(valid)][1])
            j += 1
    assert j >= len(valid)
    return proofs, [z.to_bytes(16, "little") for z in zs], frozenset(slots)


@functools.lru_cache(maxsize=None)
def _mul(point, k):
    return ec_mul(F1, point, k)


def prepare_expected(proof, z):
    """-> (status, za, b or None, zc) as k_verify_prepare leaves them: za and zc are (z | 1) times the point wherever A / C decode to a
    curve point (in the subgroup or not) and the identity otherwise; b is the decoded B, or None where B does not decode."""
    k = int.from_bytes(z, "little") | 1
    out = []
    for enc in (proof[:48], proof[144:]):
        out.append(g1_unc(_mul(_g1_decompress(enc), k) if classify_g1(enc) in (PT_OK, PT_NOT_IN_SUBGROUP) else None))
    encb = proof[48:144]
    b = g2_unc(_g2_decompress(encb)) if classify_g2(encb) in (PT_OK, PT_NOT_IN_SUBGROUP) else None
    return classify_g1(proof[:48]) | classify_g2(encb) | classify_g1(proof[144:]), out[0], b, out[1]


# ---- proofs of the toy circuit with a coordinate written as coordinate + p ----
TOY = (5, 8, 40, 300)                          # tests/test_subgroup_checks.py's _toy()
NONCANONICAL_SEED, NONCANONICAL_RANGE = 7, 16   # 16 proofs from this seed hold all four kinds (asserted below; ~23 % of coordinates have room)
COORDS = {"A.x": 0, "B.x.c1": 48, "B.x.c0": 96, "C.x": 144}   # offset of the coordinate's 48 big-endian bytes in the proof


@functools.lru_cache(maxsize=None)
def toy():
    cs, inputs, aux, vals = toy_r1cs.make(*TOY)
    pbuf = O.generate_parameters(cs, toy_r1cs.toxic(TOY[0]))
    return cs, inputs, aux, vals[1:TOY[1]], pbuf


@functools.lru_cache(maxsize=None)
def noncanonical_proofs():
    """-> {coordinate: (a proof that verifies, the same proof with that coordinate re-encoded as coordinate + p, flags kept)}"""
    cs, inputs, aux, _, pbuf = toy()
    params = O.Params(pbuf)
    rng = random.Random(NONCANONICAL_SEED)
    found = {}
    for _ in range(NONCANONICAL_RANGE):
        proof = O.create_proof(params, cs, inputs, aux, rng.randrange(1, R), rng.randrange(1, R))
        for name, off in COORDS.items():
            flags = proof[off] & 0xe0 if off in (0, 48, 144) else 0
            v = int.from_bytes(bytes([proof[off] ^ flags]) + proof[off + 1:off + 48], "big")
            if name not in found and v < ROOM:
                w = bytearray((v + P).to_bytes(48, "big"))
                assert w[0] < 0x20
                w[0] |= flags
                found[name] = (proof, proof[:off] + bytes(w) + proof[off + 48:])
    assert set(found) == set(COORDS), "no proof with room in %s: choose another seed" % sorted(set(COORDS) - set(found))
    return found
