"""masp_amd/csrc/device/bundle_check.hpp on the CPU (tests/native/bundle_check_dev.hip): the per-item steps of
masp_hip_sapling_check_bundles against the host library and the Python mirror (masp_amd/verifier.py) — point classification with the
canonical coordinates, the value-balance terms, bvk of whole bundles, the nullifier's multipacking.  No GPU."""
import bundle_check_cases as K
import bundle_check_shim as S
from masp_amd import host as H
from masp_amd import verifier as V

Q, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
G = H.point_bytes(*H.generator_uv(4))
IDENTITY = H.JUBJUB_IDENTITY


def _order(p):
    for k in (1, 2, 4, 8):
        if H.jubjub_mul(p, k) == IDENTITY:
            return k
    raise AssertionError("not a torsion point")


def _torsion_points():
    """[r_J] P over asset generators (the cofactor is not cleared there) of successive seeds, until every order has been seen"""
    found = {}
    for seed in range(4096):
        try:
            p = H.asset_generator(seed.to_bytes(4, "little") * 8)
        except ValueError:
            continue
        t = H.jubjub_mul(p, RJ)
        found.setdefault(_order(t), t)
        if len(found) == 4:
            break
    return found


def _check(enc, name):
    st, u, v = S.point(enc)
    decodes = V.decodes(enc)
    want = 1 if not decodes else 2 if V.is_small_order(enc) else 0
    assert st == want, (name, st, want)
    if decodes:
        assert (u, v) == H.point_uv(enc), name
    else:
        assert (u, v) == (0, 0), name
    return st


def test_prime_order_points_are_accepted_with_their_coordinates():
    for k in (1, 2, 3, RJ - 1, 0x1234567890abcdef, RJ // 3):
        assert _check(H.jubjub_mul(G, k), k) == 0


def test_every_small_order_point_is_classified_and_mixed_order_points_are_accepted():
    torsion = _torsion_points()
    assert sorted(torsion) == [1, 2, 4, 8]
    for order, t in torsion.items():
        assert _check(t, "order %d" % order) == 2
        for m in range(1, order):                     # every multiple: all eight points of the torsion subgroup come by
            assert _check(H.jubjub_mul(t, m), "order %d x %d" % (order, m)) == 2
    # a prime-order point plus a torsion point decodes and is not of small order: the reference accepts it
    for order in (2, 4, 8):
        mixed = H.jubjub_add(H.jubjub_mul(G, 77), torsion[order])
        assert H.jubjub_mul(mixed, RJ) != IDENTITY
        assert _check(mixed, "prime + order %d" % order) == 0


def test_encodings_that_do_not_decode():
    # v >= r written non-canonically: a point whose v + r still fits the encoding's 255 bits
    for k in range(1, 64):
        u, v = H.point_uv(H.jubjub_mul(G, k))
        if v + Q < 1 << 255:
            enc = ((v + Q) | ((u & 1) << 255)).to_bytes(32, "little")
            assert _check(enc, "v + r") == 1
            break
    else:
        raise AssertionError("no point with room")
    assert _check(Q.to_bytes(32, "little"), "v = r") == 1
    # u = 0 with the sign bit set (ZIP 216), for both points with u = 0
    assert _check((1 | (1 << 255)).to_bytes(32, "little"), "(0, 1) negative zero") == 1
    assert _check(((Q - 1) | (1 << 255)).to_bytes(32, "little"), "(0, -1) negative zero") == 1
    assert _check(IDENTITY, "identity") == 2 and _check(K.SMALL_ORDER, "(0, -1)") == 2
    # off the curve: the first few v for which u^2 is no square
    off = [v for v in range(2, 40) if not V.decodes(v.to_bytes(32, "little"))][:4]
    assert len(off) == 4
    for v in off:
        assert _check(v.to_bytes(32, "little"), "off curve") == 1
        assert _check((v | (1 << 255)).to_bytes(32, "little"), "off curve, sign set") == 1


def test_balance_terms():
    for asset in (K.ASSET, K.ASSET_B):
        g8 = H.jubjub_mul(H.asset_generator(asset), 8)
        for value in (0, 1, -1, 1 << 63, 1 << 64, (1 << 127) - 1, -((1 << 127) - 1)):
            vb = H.jubjub_mul(g8, abs(value))
            want = H.jubjub_add(IDENTITY, vb, subtract=value >= 0)            # what _Inner.bvk adds for this entry
            assert S.balance_term(asset, value) == (0, want), value
        assert S.balance_term(asset, -(1 << 127))[0] == 2
    # identifiers without a generator, found by trying seeds
    bad = []
    for seed in range(64):
        ident = bytes([seed, 0x5a]) * 16
        try:
            H.asset_generator(ident)
            assert S.balance_term(ident, 3)[0] == 0
        except ValueError:
            bad.append(ident)
            assert S.balance_term(ident, 3)[0] == 3
            assert S.balance_term(ident, -(1 << 127))[0] == 2                # the value's range comes first, as in the mirror
    assert len(bad) >= 8


def _flatten(bundles):
    sp, cv, ou = ([d for b in bundles for d in getattr(b, k)] for k in ("spends", "converts", "outputs"))
    en = [e for b in bundles for e in b.value_balance]
    j = lambda items, f: b"".join(V._le32(getattr(d, f)) for d in items)          # noqa: E731
    return ([(len(b.spends), len(b.converts), len(b.outputs), len(b.value_balance)) for b in bundles],
            [j(sp, f) for f in ("cv", "anchor", "nullifier", "rk", "zkproof")], [j(cv, f) for f in ("cv", "anchor", "zkproof")],
            [j(ou, f) for f in ("cv", "cmu", "ephemeral_key", "zkproof")],
            [b"".join(a for a, _ in en), b"".join(int(v).to_bytes(16, "little", signed=True) for _, v in en)])


def _mirror_bvk(b):
    inner = V._Inner()
    for d in b.spends + b.converts:
        inner.cv_sum = H.jubjub_add(inner.cv_sum, d.cv)
    for d in b.outputs:
        inner.cv_sum = H.jubjub_add(inner.cv_sum, d.cv, subtract=True)
    return inner.bvk(b.value_balance)


def test_bvk_of_whole_bundles_and_their_rows():
    empty = V.Bundle([], [], [], [], b"")
    outputs_only = V.Bundle([], [], K.bundle(3).outputs, [(K.ASSET, -9)], b"")
    duplicates = K.bundle(4, value_balance=[(K.ASSET, 4), (K.ASSET, 4), (K.ASSET_B, 1), (K.ASSET, -8)])
    no_balance = K.bundle(5, n=2, value_balance=[])
    bundles = [empty, K.bundle(1), outputs_only, duplicates, no_balance, K.bundle(2, n=1, value_balance=[(K.ASSET, (1 << 127) - 1)]), empty]
    res = S.check_bundles(*_flatten(bundles))
    assert res.bundle_status.tolist() == [0] * len(bundles)
    assert not res.spend_status.any() and not res.convert_status.any() and not res.output_status.any()
    for k, b in enumerate(bundles):
        assert res.bvk[k].tobytes() == _mirror_bvk(b), k
    assert res.bvk[0].tobytes() == IDENTITY
    rows = [V._rows_as_ints(a) for a in (res.spend_inputs, res.convert_inputs, res.output_inputs)]
    assert rows[0] == [V.spend_public_inputs(d.cv, d.anchor, d.nullifier, d.rk) for b in bundles for d in b.spends]
    assert rows[1] == [V.convert_public_inputs(d.cv, d.anchor) for b in bundles for d in b.converts]
    assert rows[2] == [V.output_public_inputs(d.cv, d.cmu, d.ephemeral_key) for b in bundles for d in b.outputs]


def test_statuses_of_the_refusal_list():
    bundles, _, want, where = K.refusal_list()
    res = S.check_bundles(*_flatten(bundles))
    status = {"spend": res.spend_status.tolist(), "convert": res.convert_status.tolist(), "output": res.output_status.tolist()}
    first = {"spend": 0, "convert": 0, "output": 0}
    for k, b in enumerate(bundles):
        n = {"spend": len(b.spends), "convert": len(b.converts), "output": len(b.outputs)}
        for kind in first:
            got = status[kind][first[kind]:first[kind] + n[kind]]
            expect = [0] * n[kind]
            if k in where and where[k][1].startswith(kind):
                expect[where[k][2]] = where[k][0]
            assert got == expect, (k, kind)
            first[kind] += n[kind]
        if k in where:
            assert res.bundle_status[k] == 1 and not res.bvk[k].any()
    codes = res.bundle_status.tolist()
    assert sorted(set(codes)) == [0, 1, 2, 3] and [c == 0 for c in codes] == want
    for a, st in ((res.spend_inputs, res.spend_status), (res.convert_inputs, res.convert_status), (res.output_inputs, res.output_status)):
        assert not a[st != 0].any() and a[st == 0].any(axis=(1, 2)).all()          # a refused description's row is zeros


def test_multipacking():
    for nf in (bytes(32), b"\xff" * 32, bytes(31) + b"\xc0", bytes(31) + b"\x40", bytes(31) + b"\x80", bytes(range(1, 33)), b"\xff" * 31 + b"\x3f"):
        assert S.multipack(nf) == H.multipack(nf), nf.hex()


def test_counts_must_add_up():
    import pytest
    from masp_amd.hip import MaspHipError
    args = list(_flatten([K.bundle(1), K.bundle(2)]))
    args[0] = [(3, 3, 3, 2), (3, 3, 2, 2)]
    with pytest.raises(MaspHipError):
        S.check_bundles(*args)
