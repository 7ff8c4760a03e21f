"""The references of the verifier stage tests (tests/verify_ref.py) against the host pairing (masp_amd/csrc/host/pairing.h, through the
host wrappers of tests/native/verify_dev.hip and masp_host_proof_read), and non-canonical point coordinates on the host verifier: a
proof whose x is written as x + p decodes, modulo p, to the same point, and bellman's `Proof::read` refuses it.  No GPU: the unit is
cross-compiled and only its _host functions run; tests/test_gpu_verify_stages.py runs the same inputs through the kernels."""
import random

import pytest

import verify_cases as VC
import verify_shim as VS
from pyref import P
from verify_ref import (FP12_ONE, PT_NOT_IN_SUBGROUP, PT_OK, classify_g1, classify_g2, classify_proof, fp12_mul, sqrt_fp2_branch, g2_rhs,
                        _g2_decompress)


def fp12_edge_elements():
    """1, 0, every coefficient p - 1, and the twelve elements with a single non-zero coefficient"""
    units = [tuple(P - 2 if j == i else 0 for j in range(12)) for i in range(12)]
    return [FP12_ONE, (0,) * 12, (P - 1,) * 12] + units


def test_fp12_mul_equals_the_host_tower():
    rng = random.Random(50)
    rand = lambda: tuple(rng.randrange(P) for _ in range(12))
    pairs = [(rand(), rand()) for _ in range(50)]
    edges = fp12_edge_elements()
    pairs += [(a, b) for a in edges for b in (edges[0], edges[2], edges[4], edges[9], rand())]
    for a, b in pairs:
        assert fp12_mul(a, b) == VS.fp12_mul_host(a, b)
    x = rand()
    assert fp12_mul(x, FP12_ONE) == x and fp12_mul(FP12_ONE, x) == x


def test_crafted_points_reach_the_status_they_aim_at():
    for cases, classify in ((VC.g1_cases(), classify_g1), (VC.g2_cases(), classify_g2)):
        for name, enc, want in cases:
            got = classify(enc)
            assert want is None or got == want, name
            assert got != PT_OK, name
    kinds = {}
    for kind, enc in VC.g2_sqrt_cases():
        x = _g2_decompress(enc)[0]
        assert sqrt_fp2_branch(g2_rhs(x))[1] == kind
        assert classify_g2(enc) == PT_NOT_IN_SUBGROUP, kind
        kinds[kind] = kinds.get(kind, 0) + 1
    # every way through the Fp2 square root is present, under both sign flags
    assert kinds["c1=0 square"] >= 2 and kinds["c1=0 non-square"] >= 2 and kinds["first"] >= 10 and kinds["second"] >= 10
    y = [_g2_decompress(enc)[1] for kind, enc in VC.g2_sqrt_cases() if kind == "c1=0 square"]
    assert all(v[1] == 0 for v in y)                          # the sign of such a y comes from c0


def test_classification_agrees_with_the_host_proof_read():
    from masp_amd import host as H
    proofs, _, bad = VC.prepare_batch()
    assert all(i in bad for i in VC.FORCED_BAD)
    seen = set()
    for i, proof in enumerate(proofs):
        st = classify_proof(proof)
        assert (st == PT_OK) == (i not in bad), i
        assert H.proof_read(proof) == (st == PT_OK), i
        # a crafted point alone decides: the other two points of its proof are valid
        parts = (classify_g1(proof[:48]), classify_g2(proof[48:144]), classify_g1(proof[144:]))
        assert sum(1 for s in parts if s != PT_OK) == (1 if i in bad else 0), i
        seen.add(st)
    assert seen == {0, 1, 2, 4, 8}


@pytest.mark.parametrize("coord", sorted(VC.COORDS))
def test_host_verifier_refuses_a_non_canonical_coordinate(coord):
    from masp_amd import host as H
    _, _, _, pub, pbuf = VC.toy()
    found = VC.noncanonical_proofs()                          # asserts that all four kinds occur under the chosen seed
    assert set(found) == set(VC.COORDS)
    proof, bad = found[coord]
    off = VC.COORDS[coord]
    assert bad != proof and bad[:off] == proof[:off] and bad[off + 48:] == proof[off + 48:]
    mask = 0x1f if off != 96 else 0xff
    value = lambda p: int.from_bytes(bytes([p[off] & mask]) + p[off + 1:off + 48], "big")
    assert value(bad) == value(proof) + P and (bad[off] & ~mask) == (proof[off] & ~mask)
    vk = H.PreparedVerifyingKey(pbuf)
    others = [p for p, _ in found.values()][:2]
    assert vk.verify(proof, pub) and vk.verify_batch([others[0], proof, others[1]], [pub] * 3)
    assert not vk.verify(bad, pub)
    assert not vk.verify_batch([bad], [pub])
    assert not vk.verify_batch([others[0], bad, others[1]], [pub] * 3)
    assert not H.proof_read(bad) and H.proof_read(proof)
