"""BatchValidator.validate_each on the GPU: six bundles proved by LocalTxProver and built as tests/test_gpu_batch_validator.py builds
them, four of them broken each in its own way; the per-bundle verdicts are those of SaplingVerificationContext run over each bundle,
while validate() on the same validator can only say False.  Run with `-m gpu`."""
import random

import pytest

import test_gpu_batch_validator as TB
from masp_amd import host as H
from masp_amd import prover as P
from masp_amd import verifier as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    lp = P.LocalTxProver.with_synthetic_parameters(seed=11)
    rng = random.Random(13)
    prepared = [TB._prepare_bundle(lp, rng) for _ in range(6)]
    jobs = [j for js, _ in prepared for j in js]
    proofs = lp.prove_prepared(jobs)
    lp._aux_give(jobs)
    bundles = [finish(proofs[5 * i:5 * i + 5]) for i, (_, finish) in enumerate(prepared)]
    gpu_vks = (lp._gpu_vk["spend"], lp._gpu_vk["convert"], lp._ctx.prepare_verifying_key(lp.parameters["output"]))
    host_vks = (lp.spend_vk, lp.convert_vk, H.PreparedVerifyingKey(lp.parameters["output"]))
    yield lp, bundles, gpu_vks, host_vks
    gpu_vks[2].close()
    lp.close()


def _six(bundles):
    """-> [(bundle, sighash, what check_bundle must say)]: good, bad spend-auth signature, bad binding signature, good, a proof of another
    statement, one check_bundle refuses"""
    out = []
    for k, (b, sighash, pc) in enumerate(bundles):
        s0, s1 = b.spends
        if k == 1:
            flip = s0.spend_auth_sig[:32] + bytes([s0.spend_auth_sig[32] ^ 1]) + s0.spend_auth_sig[33:]
            b = TB._replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "spend_auth_sig": flip}), s1])
        elif k == 2:
            b = TB._replace(b, binding_sig=pc.binding_sig(b.value_balance, bytes(32)))
        elif k == 4:
            b = TB._replace(b, spends=[V.SpendDescription(**{**s0.__dict__, "zkproof": s1.zkproof}),
                                       V.SpendDescription(**{**s1.__dict__, "zkproof": s0.zkproof})])
        elif k == 5:
            b = TB._replace(b, spends=[s0, V.SpendDescription(**{**s1.__dict__, "rk": TB.SMALL_ORDER})])     # refused after s0 was queued
        out.append((b, sighash, k != 5))
    return out


def test_validate_each_names_the_bad_bundles(env):
    lp, bundles, gpu_vks, host_vks = env
    six = _six(bundles)
    bv = V.BatchValidator(lp._ctx)
    for b, sighash, check_ok in six:
        assert bv.check_bundle(b, sighash) is check_ok
    want = [TB._single(b, sighash, host_vks) for b, sighash, _ in six]
    assert want == [True, False, False, True, False, False]
    assert bv.validate_each(*gpu_vks) == want
    assert bv.validate(*gpu_vks) is False
    assert bv.validate_each(*gpu_vks) == want
    good = V.BatchValidator(lp._ctx)
    for k in (0, 3):
        assert good.check_bundle(six[k][0], six[k][1]) is True
    assert good.validate_each(*gpu_vks) == [True, True] and good.validate(*gpu_vks) is True
    assert V.BatchValidator(lp._ctx).validate_each(*gpu_vks) == []
