"""BatchValidator (masp_amd/verifier.py) over bundles proved by LocalTxProver: valid bundles pass check_bundle and validate and the
single-transaction mirror; each one-thing-changed bundle gets the mirror's verdict; an empty validator is valid; two threads validate
on one context at once; validation creates no stream.  Run with `-m gpu`."""
import random
import threading

import pytest

from masp_amd import host as H
from masp_amd import prover as P
from masp_amd import redjubjub as RJS
from masp_amd import verifier as V

pytestmark = pytest.mark.gpu
Q, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
G_SPEND = H.point_bytes(*H.generator_uv(4))
IDENT = H.asset_identifier(b"benchmark")
ASSET_A, REWARD = H.asset_identifier(b"asset a"), H.asset_identifier(b"reward")
SMALL_ORDER = (Q - 1).to_bytes(32, "little")          # (0, -1)


def _rb(rng, k):
    return bytes(rng.getrandbits(8) for _ in range(k))


def _path(rng):
    return [rng.randrange(Q) for _ in range(32)], rng.getrandbits(32)


def _prepare_bundle(lp, rng):
    """-> (job list, finish(proofs) -> (Bundle, sighash, proving context)): two Spends, one Convert, two Outputs of one transaction"""
    pc = lp.new_sapling_proving_context()
    sighash = _rb(rng, 32)
    jobs, spend_keys = [], []
    for _ in range(2):
        ask, nsk, ar, rcm, rcv = (rng.randrange(1, RJ) for _ in range(5))
        ak = H.jubjub_mul(G_SPEND, ask)                 # ak = [ask] G_spend, so rsk = ask + ar signs for rk
        sib, pos = _path(rng)
        while True:
            d = _rb(rng, 11)
            try:
                cmu, _ = H.spend_leaf(ak, nsk, d, rcm, IDENT, 1)
                break
            except H.HostError:
                continue
        job = lp.prepare_spend((ak, nsk), d, rcm, ar, IDENT, 1, H.merkle_root(cmu, sib, pos), (sib, pos), rcv)
        job["anchor"] = H.merkle_root(cmu, sib, pos)
        pc._spend_like(rcv, job["cv"])
        jobs.append(job)
        spend_keys.append((ask + ar) % RJ)
    ac = H.AllowedConversion([(ASSET_A, -1), (REWARD, 1)])
    sib, pos = _path(rng)
    rcv = rng.randrange(1, RJ)
    job = lp.prepare_convert(ac, 5, H.merkle_root(ac.cmu(), sib, pos), (sib, pos), rcv)
    job["anchor"] = H.merkle_root(ac.cmu(), sib, pos)
    pc._spend_like(rcv, job["cv"])
    jobs.append(job)
    for _ in range(2):
        pk = H.jubjub_mul(H.point_bytes(*H.generator_uv(0)), rng.randrange(1, RJ))
        while True:
            try:
                rcv = rng.randrange(1, RJ)
                job = lp.prepare_output(rng.randrange(1, RJ), (_rb(rng, 11), pk), rng.randrange(1, RJ), IDENT, 1, rcv)
                break
            except P.ProvingError:
                continue
        pc._output(rcv, job["cv"])
        jobs.append(job)
    value_balance = [(IDENT, 0), (ASSET_A, -5), (REWARD, 5)]

    def finish(proofs):
        spends = []
        for j, rsk, proof in zip(jobs[:2], spend_keys, proofs[:2]):
            spends.append(V.SpendDescription(j["cv"], j["anchor"], j["nf"], j["rk"], proof, RJS.sign(rsk, j["rk"] + sighash, G_SPEND)))
        converts = [V.ConvertDescription(jobs[2]["cv"], jobs[2]["anchor"], proofs[2])]
        outputs = []
        for j, proof in zip(jobs[3:], proofs[3:]):
            pub = [int.from_bytes(j["inputs"][i].tobytes(), "little") for i in range(1, 6)]
            outputs.append(V.OutputDescription(j["cv"], pub[4], H.point_bytes(pub[2], pub[3]), proof))
        return V.Bundle(spends, converts, outputs, value_balance, pc.binding_sig(value_balance, sighash)), sighash, pc
    return jobs, finish


@pytest.fixture(scope="module")
def env():
    lp = P.LocalTxProver.with_synthetic_parameters(seed=11)
    rng = random.Random(12)
    prepared = [_prepare_bundle(lp, rng) for _ in range(8)]
    jobs = [j for js, _ in prepared for j in js]
    proofs = lp.prove_prepared(jobs)
    lp._aux_give(jobs)
    bundles = [finish(proofs[5 * i:5 * i + 5]) for i, (_, finish) in enumerate(prepared)]
    gpu_vks = (lp._gpu_vk["spend"], lp._gpu_vk["convert"], lp._ctx.prepare_verifying_key(lp.parameters["output"]))
    host_vks = (lp.spend_vk, lp.convert_vk, H.PreparedVerifyingKey(lp.parameters["output"]))
    yield lp, bundles, gpu_vks, host_vks
    gpu_vks[2].close()
    lp.close()


def _single(bundle, sighash, host_vks):
    """the whole bundle through SaplingVerificationContext (verifier/single.rs), one check at a time on the host"""
    sc = V.SaplingVerificationContext()
    for s in bundle.spends:
        if not sc.check_spend(s.cv, s.anchor, s.nullifier, s.rk, sighash, s.spend_auth_sig, s.zkproof, host_vks[0]):
            return False
    for c in bundle.converts:
        if not sc.check_convert(c.cv, c.anchor, c.zkproof, host_vks[1]):
            return False
    for o in bundle.outputs:
        if not sc.check_output(o.cv, o.cmu, o.ephemeral_key, o.zkproof, host_vks[2]):
            return False
    return sc.final_check(bundle.value_balance, sighash, bundle.binding_sig)


def test_valid_bundles(env):
    lp, bundles, gpu_vks, host_vks = env
    bv = V.BatchValidator(lp._ctx)
    for b, sighash, _ in bundles:
        assert bv.check_bundle(b, sighash) is True
        assert _single(b, sighash, host_vks) is True
    assert bv.validate(*gpu_vks) is True


def _replace(b, **kw):
    return V.Bundle(**{**b.__dict__, **kw})


def _mutations(bundles):
    (b, sighash, pc), (b2, _, _) = bundles[0], bundles[1]
    s0, s1 = b.spends
    flip = s0.spend_auth_sig[:32] + bytes([s0.spend_auth_sig[32] ^ 1]) + s0.spend_auth_sig[33:]
    o0 = b.outputs[0]
    return {
        # name: (bundle, what check_bundle must say)
        "flipped spend-auth signature": (_replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "spend_auth_sig": flip}), s1]), True),
        "binding signature over another sighash": (_replace(b, binding_sig=pc.binding_sig(b.value_balance, bytes(32))), True),
        "value balance off by one": (_replace(b, value_balance=[(IDENT, 1)] + b.value_balance[1:]), True),
        "two spend proofs swapped": (_replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "zkproof": s1.zkproof}),
                                                         V.SpendDescription(**{**s1.__dict__, "zkproof": s0.zkproof})]), True),
        "output proof in a spend slot": (_replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "zkproof": o0.zkproof}), s1]), True),
        "small-order rk": (_replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "rk": SMALL_ORDER}), s1]), False),
        "small-order cv": (_replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "cv": SMALL_ORDER}), s1]), False),
        "non-canonical epk": (_replace(b, outputs=[V.OutputDescription(**{**o0.__dict__, "ephemeral_key": Q.to_bytes(32, "little")}),
                                                   b.outputs[1]]), False),
        "i128::MIN balance": (_replace(b, value_balance=b.value_balance + [(IDENT, -(1 << 127))]), False),
    }, sighash


def test_one_change_gets_the_single_context_verdict(env):
    lp, bundles, gpu_vks, host_vks = env
    muts, sighash = _mutations(bundles)
    for name, (mb, check_ok) in muts.items():
        bv = V.BatchValidator(lp._ctx)
        assert bv.check_bundle(bundles[2][0], bundles[2][1]) is True      # a valid bundle in the same batch
        got_check = bv.check_bundle(mb, sighash)
        got = got_check and bv.validate(*gpu_vks)
        assert got_check is check_ok, name
        assert got == _single(mb, sighash, host_vks) == False, name     # noqa: E712


def test_empty_validator_is_valid(env):
    lp, _, gpu_vks, _ = env
    assert V.BatchValidator(lp._ctx).validate(*gpu_vks) is True


def test_two_threads_validate_on_one_context(env):
    lp, bundles, gpu_vks, _ = env
    n_streams = lp._ctx.stream_concurrency()[0]
    muts, sighash = _mutations(bundles)
    bad = muts["flipped spend-auth signature"][0]
    results = {}

    def run(name, items, rounds=3):
        out = []
        for _ in range(rounds):
            bv = V.BatchValidator(lp._ctx)
            out.append(all([bv.check_bundle(b, s) for b, s in items]) and bv.validate(*gpu_vks))
        results[name] = out

    ta = threading.Thread(target=run, args=("good", [(b, s) for b, s, _ in bundles[:4]]))
    tb = threading.Thread(target=run, args=("bad", [(b, s) for b, s, _ in bundles[4:7]] + [(bad, sighash)]))
    ta.start()
    tb.start()
    ta.join()
    tb.join()
    assert results == {"good": [True] * 3, "bad": [False] * 3}
    assert lp._ctx.stream_concurrency()[0] == n_streams
