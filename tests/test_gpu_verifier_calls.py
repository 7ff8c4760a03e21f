"""The verifier-side calls and the building blocks of a device context next to each other: verify_batch and verify_each under two keys (a
key's mutex each, the two verifier streams), the three Jubjub calls (one mutex, the second verifier stream), prove_batch (the context's lock
shared, like the five before it) and masp_hip_ntt (the context's lock exclusive).  What each call computes is its own file's business; here
every comparison is of a call with itself, made alone beforehand."""
import random
import threading

import numpy as np
import pytest

import masp_amd
import test_gpu_redjubjub_batch as TR
import toy_r1cs
from masp_amd import host as H
from pyref import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def toy(ctx):
    """a toy circuit in slot 3, 8 proofs of one statement, and two keys over the same parameters (one per verifier stream)"""
    cs, inputs, aux, vals = toy_r1cs.make(81, n_inputs=4, n_free=30, n_constraints=200, bool_share=0.6)
    params = ctx.generate_parameters(cs, toy_r1cs.toxic(81))
    ctx.load_circuit(3, params, cs)
    rng = random.Random(12)
    proofs = ctx.prove_batch([(3, inputs, aux, rng.randrange(R), rng.randrange(R)) for _ in range(8)])
    key_a, key_b = ctx.prepare_verifying_key(params), ctx.prepare_verifying_key(params)
    yield params, (inputs, aux), proofs, vals[1:4], key_a, key_b
    key_a.close()
    key_b.close()


def verifier_calls(ctx, toy):
    """[(name, the call)] over inputs built once; no call draws randomness of its own"""
    params, (inputs, aux), proofs, pub, key_a, key_b = toy
    rng = random.Random(13)
    pubs = [list(pub) for _ in proofs]
    one_wrong = [list(pub) for _ in proofs]
    one_wrong[5][2] = (pub[2] + 1) % R
    z_proofs = rng.randbytes(16 * len(proofs))
    sigs = [TR._item(rng)[0] for _ in range(5)]
    vk, sig, sighash, kind = sigs[3]
    one_bad = sigs[:3] + [(vk, sig[:32] + bytes([sig[32] ^ 1]) + sig[33:], sighash, kind)] + sigs[4:]
    z_sigs = rng.randbytes(16 * len(sigs))
    points = [H.jubjub_mul(TR.GENS[k % 2], rng.randrange(1, TR.RJ)) for k in range(3)]
    scalars = [rng.randrange(1 << 256) for _ in range(3)]
    jobs = [(3, inputs, aux, 700 + k, 800 + k) for k in range(2)]
    data = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(16)), np.uint8).reshape(16, 32)
    return [
        ("verify_batch, key A", lambda: key_a.verify_batch(proofs, pubs, randomness=z_proofs)),
        ("verify_each, key B", lambda: key_b.verify_each(proofs, one_wrong)),
        ("redjubjub_verify_batch", lambda: ctx.redjubjub_verify_batch(sigs, randomness=z_sigs)),
        ("redjubjub_verify_each", lambda: ctx.redjubjub_verify_each(one_bad)),
        ("jubjub_msm", lambda: ctx.jubjub_msm(points, scalars)),
        ("prove_batch", lambda: ctx.prove_batch(jobs)),
        ("ntt", lambda: ctx.ntt(data, 4).tobytes()),
    ], (one_wrong, one_bad)


def test_verifier_calls_of_every_kind_at_once(ctx, toy):
    """seven threads, one per call, four rounds each on one context: every result is that of the same call made alone.  The item the host
    verifier refuses gets the only 0 of its call, so the per-item calls have both answers to mix up."""
    calls, (one_wrong, one_bad) = verifier_calls(ctx, toy)
    alone = [call() for _, call in calls]
    hvk = H.PreparedVerifyingKey(toy[0])
    assert alone[0] is True and alone[2] is True
    assert alone[1] == [1 if hvk.verify(p, pi) else 0 for p, pi in zip(toy[2], one_wrong)] == [1, 1, 1, 1, 1, 0, 1, 1]
    assert alone[3] == [TR._single(it) for it in one_bad] == [True, True, True, False, True]
    assert len(alone[4]) == 32 and [len(p) for p in alone[5]] == [192, 192] and len(alone[6]) == 16 * 32
    wrong = [[] for _ in calls]

    def work(t):
        try:
            for rnd in range(4):
                if calls[t][1]() != alone[t]:
                    wrong[t].append((rnd, calls[t][0]))
        except Exception as e:      # (a failure in a thread is not the test's unless it is carried over)
            wrong[t].append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(calls))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert wrong == [[] for _ in calls]


def test_a_key_keeps_the_timing_of_its_own_last_call(ctx, toy):
    """verify_each_last_timing is a key's: a call under key B leaves what key A recorded as it was"""
    params, _, proofs, pub, key_a, key_b = toy
    pubs = [list(pub) for _ in proofs]
    assert key_a.verify_each(proofs, pubs) == [1] * 8
    ms_a = key_a.verify_each_last_timing()
    assert all(t > 0 for t in ms_a.values()), ms_a
    assert key_b.verify_each(proofs[:3], pubs[:3]) == [1] * 3
    assert key_a.verify_each_last_timing() == ms_a
    ms_b = key_b.verify_each_last_timing()
    assert all(t > 0 for t in ms_b.values()), ms_b
