"""masp_hip_verify_each end to end: the verdict of every proof equals what masp_host_vk_verify says of it alone (1 valid, 0 the pairing
equation fails, 2 `Proof::read` refuses it, 3 an input >= r), on a toy circuit with every kind of bad item and on real Convert and
Spend proofs; verify_batch on the same data agrees (True iff every verdict is 1).  Run with `-m gpu`."""
import random

import pytest

import oracle_lib as O
import toy_r1cs
from pyref import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import masp_amd
    c = masp_amd.Context(0)
    yield c
    c.close()


def host_verdicts(hvk, proofs, pubs):
    out = []
    for p, pi in zip(proofs, pubs):
        rc = hvk._L.masp_host_vk_verify(hvk._h, bytes(p), b"".join(int(x).to_bytes(32, "little") for x in pi), len(pi))
        out.append({1: 1, 0: 0, -2: 2, -3: 3}[rc])
    return out


@pytest.fixture(scope="module")
def toy(ctx):
    from masp_amd import host as H
    cs, inputs, aux, vals = toy_r1cs.make(81, n_inputs=4, n_free=30, n_constraints=200, bool_share=0.6)
    _, inputs2, aux2, vals2 = toy_r1cs.make(81, n_inputs=4, n_free=30, n_constraints=200, bool_share=0.6, input_values=[5, 6, 7])
    params = ctx.generate_parameters(cs, toy_r1cs.toxic(81))
    ctx.load_circuit(3, params, cs)
    rng = random.Random(8)
    proofs = ctx.prove_batch([(3, inputs, aux, rng.randrange(R), rng.randrange(R)) for _ in range(11)])
    other = ctx.prove(3, inputs2, aux2, rng.randrange(R), rng.randrange(R))          # a valid proof of another statement
    assert O.verify_proof(params, other, vals2[1:4]) == 1
    gvk = ctx.prepare_verifying_key(params)
    yield params, proofs, vals[1:4], gvk, H.PreparedVerifyingKey(params), other
    gvk.close()


def _bad_items(proofs, pub, other):
    """name -> (proof, inputs, the verdict it must get)"""
    flag = bytearray(proofs[0])
    flag[0] &= 0x7f
    bump = bytearray(proofs[0])
    bump[47] ^= 1
    return {
        "wrong input": (proofs[4], [pub[0], pub[1], (pub[2] + 1) % R], 0),
        "proof of another statement": (other, pub, 0),
        "mixed halves": (proofs[0][:48] + proofs[1][48:144] + proofs[0][144:], pub, 0),
        "cleared compression flag": (bytes(flag), pub, 2),
        "bumped x": (bytes(bump), pub, None),                       # off the curve (2) or another point (0 or 2): the host decides
        "identity encoding": (bytes([0xc0]) + bytes(47) + proofs[0][48:], pub, 2),
        "input >= r": (proofs[6], [pub[0], R, pub[2]], 3),
        "input 2^256 - 1 and a refused proof": (bytes(flag), [2 ** 256 - 1, pub[1], pub[2]], 2),        # 2 comes before 3
    }


def test_toy_verdicts_equal_the_host_verifier_item_by_item(toy):
    params, proofs, pub, gvk, hvk, other = toy
    assert all(O.verify_proof(params, p, pub) == 1 for p in proofs)                         # independent pairing
    bad = _bad_items(proofs, pub, other)
    batch = [(p, pub) for p in proofs]
    for k, (name, (p, pi, _)) in zip((1, 3, 4, 6, 7, 8, 9, 10), bad.items()):
        batch[k] = (p, pi)
    ps, pis = [b[0] for b in batch], [b[1] for b in batch]
    got = gvk.verify_each(ps, pis)
    assert got == host_verdicts(hvk, ps, pis)
    assert [got[k] for k in (0, 2, 5)] == [1, 1, 1]
    for k, (name, (_, _, want)) in zip((1, 3, 4, 6, 7, 8, 9, 10), bad.items()):
        assert want is None or got[k] == want, name
        assert got[k] != 1, name
    assert set(got) == {0, 1, 2, 3}
    assert gvk.verify_each(ps, pis) == got                                                   # no randomness: the same again
    assert not gvk.verify_batch(ps, pis)


@pytest.mark.parametrize("where", [0, 5, 10])
def test_one_bad_item_among_valid_ones_is_the_only_zero(toy, where):
    params, proofs, pub, gvk, hvk, other = toy
    pis = [list(pub) for _ in proofs]
    pis[where] = [pub[0], pub[1], (pub[2] + 1) % R]
    want = [0 if k == where else 1 for k in range(11)]
    assert gvk.verify_each(proofs, pis) == want == host_verdicts(hvk, proofs, pis)
    assert not gvk.verify_batch(proofs, pis)


def test_sizes_and_shapes(toy, ctx):
    params, proofs, pub, gvk, hvk, other = toy
    assert gvk.verify_each([], []) == []
    for n in (1, 2, 11):
        assert gvk.verify_each(proofs[:n], [pub] * n) == [1] * n
        assert gvk.verify_batch(proofs[:n], [pub] * n)
    with pytest.raises(ValueError):
        gvk.verify_each(proofs[:2], [pub, pub[:-1]])
    import ctypes as C
    out = C.create_string_buffer(1)
    rc = ctx._L.masp_hip_verify_each(ctx._h, gvk._h, 1, proofs[0], b"".join(int(x).to_bytes(32, "little") for x in pub), 2, out)
    assert rc == 3                                                                           # MASP_HIP_E_PARAMS_SHAPE
    assert ctx._L.masp_hip_verify_each(ctx._h, gvk._h, 0, None, None, 3, None) == 0


@pytest.mark.parametrize("kind,n", [("convert", 5), ("spend", 9)])
def test_real_circuit_verdicts_equal_the_host_verifier(ctx, kind, n):
    from masp_amd import host as H
    from masp_amd import workload as W
    from masp_amd.synthetic import toxic_waste
    cs = H.circuit(kind)[0]
    params = ctx.generate_parameters(cs, toxic_waste(60))
    ctx.load_circuit(0, params, cs)
    insts = W.instances(kind, n, first_seed=6000)
    rng = random.Random(9)
    proofs = ctx.prove_batch([(0, i, a, rng.randrange(R), rng.randrange(R)) for i, a in insts])
    pub = [W.public_inputs(i) for i, _ in insts]
    hvk = H.PreparedVerifyingKey(params)
    gvk = ctx.prepare_verifying_key(params)
    try:
        assert gvk.verify_each(proofs, pub) == [1] * n == host_verdicts(hvk, proofs, pub)
        assert gvk.verify_batch(proofs, pub)
        wrong = list(proofs)
        wrong[n // 2] = proofs[0]                                                            # a valid proof of ANOTHER statement
        got = gvk.verify_each(wrong, pub)
        assert got == host_verdicts(hvk, wrong, pub) == [0 if k == n // 2 else 1 for k in range(n)]
        assert not gvk.verify_batch(wrong, pub)
    finally:
        gvk.close()
