"""BatchValidator.validate_each (masp_amd/verifier.py) remembers which check_bundle call queued which signature and proof.  Here the
per-item verifiers are stubs that call chosen items bad, and the bundles are shaped on the host alone (points that decode, proofs
`Proof::read` accepts; nothing is proved), so only the bookkeeping is under test — no GPU."""
import oracle_lib as O
from masp_amd import host as H
from masp_amd import verifier as V
from pyref import g1_comp, g2_comp

G = H.point_bytes(*H.generator_uv(4))
SMALL_ORDER = (H.FR_MODULUS - 1).to_bytes(32, "little")          # (0, -1)


def _g1(k):
    u = O.g1_mul_gen(k)[0]
    return (int.from_bytes(u[:48], "big"), int.from_bytes(u[48:], "big"))


def _g2(k):
    u = O.g2_mul_gen(k)[0]
    c = [int.from_bytes(u[48 * i:48 * i + 48], "big") for i in range(4)]
    return ((c[1], c[0]), (c[3], c[2]))


def proof(tag):
    """192 bytes `Proof::read` accepts, different for every tag"""
    p = g1_comp(_g1(3 * tag + 1)) + g2_comp(_g2(3 * tag + 2)) + g1_comp(_g1(3 * tag + 3))
    assert len(p) == 192 and H.proof_read(p)
    return p


def point(k):
    return H.jubjub_mul(G, k)


def sig(tag):
    return bytes([tag]) * 64


def bundle(tag, n_spends=2, small_order_rk_at=None):
    spends = [V.SpendDescription(point(100 * tag + i + 1), 5, bytes([tag, i]) * 16, SMALL_ORDER if i == small_order_rk_at else point(100 * tag + i + 50),
                                 proof(10 * tag + i), sig(10 * tag + i)) for i in range(n_spends)]
    converts = [V.ConvertDescription(point(100 * tag + 70), 6, proof(10 * tag + 5))]
    outputs = [V.OutputDescription(point(100 * tag + 80), 7, point(100 * tag + 81), proof(10 * tag + 6))]
    return V.Bundle(spends, converts, outputs, [], sig(10 * tag + 9))


class StubContext:
    def __init__(self, bad_sigs=()):
        self.bad, self.calls = set(bad_sigs), []

    def redjubjub_verify_each(self, items):
        self.calls.append(len(items))
        return [it[1] not in self.bad for it in items]

    def redjubjub_verify_batch(self, items, randomness=None):
        return all(it[1] not in self.bad for it in items)


class StubKey:
    def __init__(self, bad_proofs=()):
        self.bad, self.seen = set(bad_proofs), []

    def verify_each(self, proofs, public_inputs):
        assert len(proofs) == len(public_inputs)
        self.seen += list(proofs)
        return [0 if p in self.bad else 1 for p in proofs]

    def verify_batch(self, proofs, public_inputs, randomness=None):
        return all(p not in self.bad for p in proofs)


def run(bundles, bad_sigs=(), bad_proofs=()):
    ctx = StubContext(bad_sigs)
    bv = V.BatchValidator(ctx)
    checks = [bv.check_bundle(b, bytes([k]) * 32) for k, b in enumerate(bundles)]
    keys = [StubKey(bad_proofs) for _ in range(3)]
    return bv, ctx, keys, checks, bv.validate_each(*keys)


def test_every_item_counts_against_its_own_bundle_only():
    bundles = [bundle(t) for t in range(1, 6)]
    assert run(bundles)[4] == [True] * 5
    assert run(bundles, bad_sigs=[sig(21)])[4] == [True, False, True, True, True]                       # a spend-auth signature
    assert run(bundles, bad_sigs=[sig(59)])[4] == [True, True, True, True, False]                       # the last binding signature
    assert run(bundles, bad_proofs=[proof(10)])[4] == [False, True, True, True, True]                   # the first spend proof
    assert run(bundles, bad_proofs=[proof(35)])[4] == [True, True, False, True, True]                   # a convert proof
    assert run(bundles, bad_proofs=[proof(46), proof(16)], bad_sigs=[sig(49)])[4] == [False, True, True, False, True]
    bv, ctx, keys, checks, each = run(bundles, bad_proofs=[proof(26)])                                  # an output proof
    assert checks == [True] * 5 and each == [True, False, True, True, True]
    assert bv.validate(*keys) is False and bv.validate_each(*keys) == each                              # validate is as it was; again the same
    assert [len(k.seen) for k in keys] == [2 * 10, 2 * 5, 2 * 5] and ctx.calls == [15, 15]


def test_a_bundle_refused_midway_is_false_and_its_queued_items_touch_no_neighbour():
    refused = bundle(2, small_order_rk_at=1)                     # its first spend is queued (signature and proof), its second refused
    bundles = [bundle(1), refused, bundle(3)]
    bv, ctx, keys, checks, each = run(bundles, bad_sigs=[sig(20)], bad_proofs=[proof(20)])
    assert checks == [True, False, True]
    assert len(bv._signatures) == 3 + 1 + 3 and len(bv._proofs["spend"][0]) == 2 + 1 + 2                # they ARE queued, as in the reference
    assert each == [True, False, True]                           # ... and bad, and count against nobody
    assert proof(20) not in keys[0].seen and ctx.calls == [6]    # what a refused bundle queued is not even verified
    assert bv.validate(*keys) is False                           # validate verifies everything queued: unchanged
    assert run(bundles)[4] == [True, False, True]                # refused stays False when all its items are good
    assert run([refused])[4] == [False]
    assert run([refused, refused, bundle(4)], bad_proofs=[proof(45)])[4] == [False, False, False]


def test_no_bundles_and_empty_bundles():
    bv = V.BatchValidator(StubContext())
    assert bv.validate_each(StubKey(), StubKey(), StubKey()) == [] and bv.validate(StubKey(), StubKey(), StubKey()) is True
    empty = V.Bundle([], [], [], [], sig(1))
    assert run([empty, bundle(1), empty])[4] == [True, True, True]
    assert run([empty, bundle(1), empty], bad_sigs=[sig(1)])[4] == [False, True, False]
