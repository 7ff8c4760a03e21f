"""The device half of the GPU Groth16 batch verifier (masp_amd/csrc/device/pairing.hpp, subgroup.hpp), stage by stage: each kernel is
launched on its own through the test-side unit tests/native/verify_dev.hip and compared, as exact integers and bytes, with the plain
references of tests/verify_ref.py (and, for the Miller loop, with masp_amd/csrc/host/pairing.h); then batches beyond one pass of the
kernels' strided loops, and proofs with a non-canonical coordinate, through masp_hip_verify_batch itself.  tests/test_verify_ref.py
checks the references and the same inputs on the CPU.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import oracle_lib as O
import toy_r1cs
import verify_cases as VC
import verify_shim as VS
from pyref import F1, F2, G1, G2, P, R, ec_add, ec_mul, g1_unc, g2_unc
from verify_ref import FP12_ONE, PT_NOT_IN_SUBGROUP, PT_OK, _g2_decompress, classify_g2, fp12_product, g2_rhs, sqrt_fp2_branch

pytestmark = pytest.mark.gpu


# ---- k_verify_prepare ----
@pytest.fixture(scope="module")
def prepared():
    proofs, zs, bad = VC.prepare_batch()
    return proofs, zs, bad, VS.prepare_gpu(proofs, zs)


def test_prepare_statuses_are_exact_and_per_index(prepared):
    proofs, zs, bad, (status, _, _, _) = prepared
    n = len(proofs)
    assert n == VC.PREPARE_N and (n + 63) // 64 == 3 and n % 64 and all(i in bad for i in VC.FORCED_BAD)
    want = [VC.prepare_expected(p, z)[0] for p, z in zip(proofs, zs)]
    assert set(want) == {0, 1, 2, 4, 8} and all((want[i] != PT_OK) == (i in bad) for i in range(n))
    for i in range(n):
        assert status[i] == want[i], (i, status[i], want[i])
    for i in bad:                                              # a refusal stays at its own index
        for j in (i - 1, i + 1):
            if 0 <= j < n and j not in bad:
                assert status[j] == 0, (i, j)


def test_prepare_multiples_and_decoded_points(prepared):
    proofs, zs, bad, (_, za, b, zc) = prepared
    checked_b = 0
    for i, (p, z) in enumerate(zip(proofs, zs)):
        _, want_za, want_b, want_zc = VC.prepare_expected(p, z)
        assert za[i] == want_za, i
        assert zc[i] == want_zc, i
        if want_b is not None:
            assert b[i] == want_b, i
            checked_b += 1
    assert checked_b >= len(proofs) - len(bad) + len(VC.g2_sqrt_cases())
    special = {int.from_bytes(z, "little") for i, z in enumerate(zs) if i not in bad}
    assert 0 in special and (1 << 128) - 1 in special and any(z and not z & 1 for z in special)


def test_prepare_fp2_square_root_branches_and_sign_rule(prepared):
    proofs, _, _, (status, _, b, _) = prepared
    where = {p[48:144]: i for i, p in enumerate(proofs)}
    kinds = {}
    for kind, enc in VC.g2_sqrt_cases():
        i = where[enc]
        x, y = _g2_decompress(enc)
        assert sqrt_fp2_branch(g2_rhs(x))[1] == kind
        if kind == "c1=0 square":
            assert y[1] == 0
        assert b[i] == g2_unc((x, y)), (kind, i)
        assert status[i] == PT_NOT_IN_SUBGROUP == classify_g2(enc), (kind, i)
        kinds.setdefault(kind, set()).add(enc[0] & 0x20)
    assert all(kinds[k] == {0, 0x20} for k in ("c1=0 square", "c1=0 non-square", "first", "second"))


# ---- k_g1_sum_export ----
@pytest.fixture(scope="module")
def multiples():
    rng = random.Random(60)
    return VC.g1_points([rng.randrange(1, R) for _ in range(1000)])


def _sum(points):
    acc = None
    for p in points:
        acc = ec_add(F1, acc, p)
    return acc


def _wire(points):
    return [bytes(96) if p is None else g1_unc(p) for p in points]           # the unit reads an entry of zeros as the identity


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 513, 1000])
def test_g1_sum_of_random_multiples(multiples, n):
    assert VS.g1_sum_gpu(_wire(multiples[:n])) == g1_unc(_sum(multiples[:n]))


def test_g1_sum_exceptional_additions(multiples):
    n = 513
    neg = lambda p: (p[0], P - p[1])
    sparse = [None if i % 4 == 0 else p for i, p in enumerate(multiples[:n])]
    assert VS.g1_sum_gpu(_wire(sparse)) == g1_unc(_sum(sparse))
    same = [multiples[0]] * n                                                # every addition of the tree is a doubling
    assert VS.g1_sum_gpu(_wire(same)) == g1_unc(ec_mul(F1, multiples[0], n))
    pairs = [q for p in multiples[:n // 2] for q in (p, neg(p))]
    assert len(pairs) == n - 1
    assert VS.g1_sum_gpu(_wire(pairs + [multiples[700]])) == g1_unc(multiples[700])
    assert VS.g1_sum_gpu(_wire([multiples[700]] + pairs)) == g1_unc(multiples[700])
    cancel = pairs + [None]
    assert VS.g1_sum_gpu(_wire(cancel)) == g1_unc(None) == b"\x40" + bytes(95)
    far = multiples[:256] + [neg(p) for p in multiples[:256]] + [None]           # lane k adds P_k and, in its second turn, -P_k
    assert VS.g1_sum_gpu(_wire(far)) == g1_unc(None)


# ---- k_miller_pairs ----
PROGRAM_KS = [1, 2, 123456789, (1 << 200) + 7, R - 1]                              # tests/test_pairing_program.py's


@pytest.fixture(scope="module")
def miller():
    """70 pairs in one launch: (k G1, (3k + 1) G2), then (a G1, b G2) and (G1, ab G2) for five (a, b), then a pair with each point at
    infinity -> (pairs, the device's values)"""
    rng = random.Random(61)
    ks = PROGRAM_KS + [rng.randrange(1, R) for _ in range(53)]
    ab = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(5)]
    g1 = O.g1_mul_gen_many(np.stack([VC.fr32(k) for k in ks + [a for a, _ in ab] + [1] * 5]))
    g2 = O.g2_mul_gen_many(np.stack([VC.fr32(3 * k + 1) for k in ks] + [VC.fr32(b) for _, b in ab] + [VC.fr32(a * b) for a, b in ab]))
    pairs = [(p.tobytes(), q.tobytes()) for p, q in zip(g1, g2)]
    pairs += [(g1_unc(None), pairs[0][1]), (pairs[0][0], g2_unc(None))]
    assert len(pairs) == 70
    return pairs, VS.miller_gpu(pairs)


def test_miller_values_equal_the_host_miller_loop(miller):
    pairs, got = miller
    want = VS.miller_host(pairs)
    for i in range(len(pairs)):
        assert got[i] == want[i], i
    assert pairs[0][0] == g1_unc(G1) and pairs[0][1] == g2_unc(ec_mul(F2, G2, 4))   # the oracle's points are the reference's
    assert len(set(got[:68])) == 68 and all(c < P for f in got for c in f)


def test_miller_values_are_bilinear(miller):
    _, got = miller
    for k in range(5):
        left, right = got[58 + k], got[63 + k]                                   # e(a G1, b G2) and e(G1, ab G2)
        assert left != right
        assert VS.final_exp_eq_host(left, right)
        assert not VS.final_exp_is_one_host(left)
    assert not VS.final_exp_eq_host(got[58], got[59])


def test_miller_pair_with_a_point_at_infinity_is_one(miller):
    _, got = miller
    assert got[68] == FP12_ONE and got[69] == FP12_ONE


# ---- k_fp12_product ----
@pytest.fixture(scope="module")
def fp12_values():
    rng = random.Random(62)
    return [tuple(rng.randrange(P) for _ in range(12)) for _ in range(200)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_fp12_product_of_arbitrary_elements(fp12_values, n):
    assert VS.fp12_product_gpu(fp12_values[:n]) == fp12_product(fp12_values[:n])


def test_fp12_product_edge_elements_and_tail(fp12_values):
    n = 129
    units = [tuple(P - 2 if j == i else 0 for j in range(12)) for i in range(12)]
    vals = list(fp12_values[:n])
    for k, e in enumerate([FP12_ONE, (P - 1,) * 12] + units):
        vals[9 * k + 3] = e                                                      # spread over the waves and over both turns
    vals[128] = units[7]
    want = fp12_product(vals)
    assert any(want)
    assert VS.fp12_product_gpu(vals) == want
    for last in (64, 127, 128):                                                  # only one element differs from 1: it must reach the result
        ones = [FP12_ONE] * n
        ones[last] = fp12_values[5]
        assert VS.fp12_product_gpu(ones) == fp12_values[5], last
    assert VS.fp12_product_gpu([FP12_ONE] * n) == FP12_ONE


# ---- through masp_hip_verify_batch ----
@pytest.fixture(scope="module")
def ctx():
    import masp_amd
    c = masp_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def abi(ctx):
    """the toy circuit, 11 proofs of one statement and one of another, the GPU and host verifying keys"""
    from masp_amd import host as H
    cs, inputs, aux, pub, pbuf = VC.toy()
    cs2, inputs2, aux2, vals2 = toy_r1cs.make(*VC.TOY, input_values=[v + 1 for v in pub])
    pub2 = vals2[1:VC.TOY[1]]
    assert pub2 != pub and all((x == y).all() for m, m2 in zip(cs.mats, cs2.mats) for x, y in zip(m, m2))   # the same circuit
    ctx.load_circuit(5, pbuf, cs)
    rng = random.Random(63)
    proofs = ctx.prove_batch([(5, inputs, aux, rng.randrange(R), rng.randrange(R)) for _ in range(11)] + [(5, inputs2, aux2, rng.randrange(R), rng.randrange(R))])
    gvk = ctx.prepare_verifying_key(pbuf)
    hvk = H.PreparedVerifyingKey(pbuf)
    other = proofs.pop()
    assert O.verify_proof(pbuf, other, pub2) == 1 and O.verify_proof(pbuf, other, pub) == 0 and O.verify_proof(pbuf, proofs[0], pub) == 1
    yield proofs, pub, other, pub2, gvk, hvk
    gvk.close()


@pytest.mark.parametrize("n", [64, 65, 128, 129, 257, 513])
def test_batches_beyond_one_pass_of_the_strided_loops(abi, n):
    proofs, pub, other, pub2, gvk, hvk = abi
    rng = random.Random(n)
    batch, pubs = [proofs[i % 11] for i in range(n)], [pub] * n
    z = bytes(rng.getrandbits(8) for _ in range(16 * n))
    assert gvk.verify_batch(batch, pubs)                                         # fresh randomness
    assert gvk.verify_batch(batch, pubs, randomness=z) and hvk.verify_batch(batch, pubs, randomness=z)
    assert gvk.verify_batch([other], [pub2])
    for k in sorted({n - 1} | {k for k in (64, 128, 256) if k < n}):
        wrong = list(batch)
        wrong[k] = other                                                         # a valid proof, of another statement
        assert not gvk.verify_batch(wrong, pubs, randomness=z), k
        assert not gvk.verify_batch(wrong, pubs), k
        assert not hvk.verify_batch(wrong, pubs, randomness=z), k
        right = list(pubs)
        right[k] = pub2                                                          # ... which its own statement accepts there
        assert gvk.verify_batch(wrong, right, randomness=z), k


def test_gpu_verifier_refuses_non_canonical_coordinates(abi):
    _, pub, _, _, gvk, hvk = abi
    found = VC.noncanonical_proofs()
    assert set(found) == set(VC.COORDS)
    good = [p for p, _ in found.values()][:3]
    assert gvk.verify_batch(good, [pub] * 3)
    for coord, (proof, bad) in found.items():
        assert gvk.verify_batch([proof], [pub]), coord
        assert not gvk.verify_batch([bad], [pub]), coord
        assert not gvk.verify_batch([good[0], bad, good[2]], [pub] * 3), coord
        assert not hvk.verify_batch([good[0], bad, good[2]], [pub] * 3), coord
