"""masp_hip_redjubjub_verify_batch = the AND of per-signature RedJubjub verification (masp_amd.redjubjub.verify, ZIP 216): mixed
spend-authorisation / binding batches, one bad item at the first, middle and last index, and the cofactor cases that both must accept.
Run with `-m gpu`."""
import random

import pytest

from masp_amd import host as H
from masp_amd import redjubjub as RJS
from masp_amd.hip import BINDING, SPEND_AUTH, Context

pytestmark = pytest.mark.gpu
Q, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
GENS = {SPEND_AUTH: H.point_bytes(*H.generator_uv(4)), BINDING: H.point_bytes(*H.generator_uv(3))}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _sign(rng, sk, vk, sighash, kind, torsion=None):
    """RedJubjub signature over vk || sighash with an explicit nonce; torsion: added to R before c is taken (S matches the new R)"""
    g = GENS[kind]
    r = rng.randrange(1, RJ)
    rbar = H.jubjub_mul(g, r)
    if torsion is not None:
        rbar = H.jubjub_add(rbar, torsion)
    s = (r + RJS.h_star(rbar, vk + sighash) * sk) % RJ
    return rbar + s.to_bytes(32, "little")


def _item(rng, kind=None):
    kind = rng.randrange(2) if kind is None else kind
    sk = rng.randrange(1, RJ)
    vk = H.jubjub_mul(GENS[kind], sk)
    sighash = bytes(rng.getrandbits(8) for _ in range(32))
    return (vk, _sign(rng, sk, vk, sighash, kind), sighash, kind), sk


def _single(item):
    vk, sig, sighash, kind = item
    return RJS.verify(vk, vk + sighash, sig, GENS[kind])


def _torsion(order):
    for v in range(2, 1000):
        e = v.to_bytes(32, "little")
        try:
            H.point_uv(e)
        except ValueError:
            continue
        t = H.jubjub_mul(e, RJ)
        if t != H.JUBJUB_IDENTITY and H.jubjub_mul(t, order) == H.JUBJUB_IDENTITY and H.jubjub_mul(t, order // 2) != H.JUBJUB_IDENTITY:
            return t
    raise AssertionError


def _non_canonical(enc):
    v = int.from_bytes(enc, "little") & ((1 << 255) - 1)
    return None if v + Q >= 1 << 255 else ((v + Q) | (int.from_bytes(enc, "little") & (1 << 255))).to_bytes(32, "little")


@pytest.mark.parametrize("n", [1, 2, 64, 65, 4097])
def test_valid_mixed_batches(ctx, n):
    rng = random.Random(n)
    items = [_item(rng, kind=i % 2 if n <= 2 else None)[0] for i in range(n)]
    sample = items if n <= 65 else items[:50] + items[-50:]
    assert all(_single(it) for it in sample)
    assert ctx.redjubjub_verify_batch(items) is True
    assert ctx.redjubjub_verify_batch([]) is True


def _corruptions(rng, item):
    vk, sig, sighash, kind = item
    s = int.from_bytes(sig[32:], "little")
    out = {"wrong sighash": (vk, sig, bytes([sighash[0] ^ 1]) + sighash[1:], kind),
           "wrong kind": (vk, sig, sighash, 1 - kind),
           "s >= r_J": (vk, sig[:32] + (s + RJ).to_bytes(32, "little"), sighash, kind),
           "flipped S": (vk, sig[:32] + bytes([sig[32] ^ 1]) + sig[33:], sighash, kind)}
    while "non-canonical R" not in out or "non-canonical vk" not in out:
        it, _ = _item(rng, kind)
        nr, nv = _non_canonical(it[1][:32]), _non_canonical(it[0])
        if nr is not None and "non-canonical R" not in out:
            out["non-canonical R"] = (it[0], nr + it[1][32:], it[2], kind)
        if nv is not None and "non-canonical vk" not in out:
            out["non-canonical vk"] = (nv, it[1], it[2], kind)
    return out


def test_one_bad_item_at_first_middle_last(ctx):
    rng = random.Random(7)
    items = [_item(rng)[0] for _ in range(65)]
    for name, bad in _corruptions(rng, items[32]).items():
        assert not _single(bad), name
        for k in (0, 32, 64):
            batch = list(items)
            batch[k] = bad
            assert ctx.redjubjub_verify_batch(batch) is False, (name, k)
    assert ctx.redjubjub_verify_batch(items) is True


def test_s_equal_to_the_group_order_is_no_signature(ctx):
    """S = r_J exactly, the smallest S that jubjub::Fr::from_repr refuses (the batch call decides it on the host, the per-item call in
    its kernel), as the middle one of 5 items: the batch call answers all_valid = 0, the per-item call 0 for that item alone."""
    rng = random.Random(9)
    items = [_item(rng)[0] for _ in range(5)]
    vk, sig, sighash, kind = items[2]
    batch = items[:2] + [(vk, sig[:32] + RJ.to_bytes(32, "little"), sighash, kind)] + items[3:]
    want = [_single(it) for it in batch]
    assert want == [True, True, False, True, True]
    assert ctx.redjubjub_verify_batch(batch) is False
    assert ctx.redjubjub_verify_each(batch) == want


def test_cofactor_cases_are_accepted(ctx):
    rng = random.Random(8)
    items = [_item(rng)[0] for _ in range(10)]
    for order in (2, 4, 8):
        t = _torsion(order)
        for kind in (SPEND_AUTH, BINDING):
            sk = rng.randrange(1, RJ)
            vk = H.jubjub_mul(GENS[kind], sk)
            sighash = bytes(rng.getrandbits(8) for _ in range(32))
            r_plus_t = (vk, _sign(rng, sk, vk, sighash, kind, torsion=t), sighash, kind)       # R + T, S from the new c
            vk_t = H.jubjub_add(vk, t)
            vk_plus_t = (vk_t, _sign(rng, sk, vk_t, sighash, kind), sighash, kind)              # vk + T
            for case in (r_plus_t, vk_plus_t):
                assert _single(case), order
                assert ctx.redjubjub_verify_batch(items[:5] + [case] + items[5:]) is True, order
