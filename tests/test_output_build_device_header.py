"""masp_amd/csrc/device/output_build.hpp compiled for the host (tests/native/output_build_dev.hip): the seal step alone against the
reference's note encryption vectors, the fixed-base table of G_vcr against the host's scalar multiplication, and all steps on the
130-plan batch against output_build_ref.  CPU only; bytes."""
import json
import os
import random

import output_build_ref as R
import output_build_shim as S
from masp_amd import host as H

RJ = H.JUBJUB_ORDER
G_VCR = H.point_bytes(*H.generator_uv(3))     # value_commitment_randomness
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_seal_step_alone_against_the_vectors():
    k = json.load(open(os.path.join(GOLDEN, "note_encryption_vectors.json")))
    h = bytes.fromhex
    assert len(k["vectors"]) == 10
    for tv in k["vectors"]:
        enc, cout = S.seal(h(tv["k_enc"]), h(tv["p_enc"]), h(tv["ovk"]), h(tv["cv"]), h(tv["cmu"]), h(tv["epk"]), h(tv["default_pk_d"]), h(tv["esk"]))
        assert (enc.hex(), cout.hex()) == (tv["c_enc"], tv["c_out"])
        if h(tv["memo"]) == R.NE.EMPTY_MEMO:     # the made-up empty memo is the uploaded one
            assert S.seal(h(tv["k_enc"]), h(tv["p_enc"]), h(tv["ovk"]), h(tv["cv"]), h(tv["cmu"]), h(tv["epk"]), h(tv["default_pk_d"]), h(tv["esk"]),
                          use_memo=False)[0].hex() == tv["c_enc"]


def test_the_seal_step_without_an_ovk_and_without_a_memo():
    for seed in (31, 32):
        p = R.good_plan(seed, lead=2, ovk=False, memo=False)
        _, cv, cmu, epk, enc, cout = R.reference(p)
        _, esk = R.scalars(p)
        k_enc = R.seal(p, cv, cmu, esk)[1]
        for use_memo in (True, False):
            assert S.seal(k_enc, R.plaintext(p), None, cv, cmu, epk, p["pk_d"], esk, out_random=p["out_random"], use_memo=use_memo) == (enc, cout)


def test_g_vcr_table_products():
    rng = random.Random(63)
    # (every digit 15 is 2^252 - 1, past r_J - 1: the table serves it all the same)
    for k in [0, 1, 15, 16, RJ - 1, 9 << (4 * 62), (1 << 252) - 1] + [rng.randrange(RJ) for _ in range(30)]:
        assert S.table_mul(k) == H.jubjub_mul(G_VCR, R._le(k)), k


def test_all_steps_on_the_batch_against_the_reference():
    plans, want = R.batch(130)
    arrays = R.arrays(plans)
    block = S.stage_host(0, arrays, S.new_block(130))
    R.check(S.results(block, 130), want)
    # stage after stage is the same as all at once, and a refused plan's parts stay zeros
    step = S.new_block(130)
    for k in range(1, 8):
        step = S.stage_host(k, arrays, step)
    assert step.tobytes() == block.tobytes()


def test_every_status_and_no_memos_through_the_steps():
    cases, want = R.references("status", lambda: [p for c, b, _ in R.status_plans() for p in (c, b)])
    R.check(S.results(S.stage_host(0, R.arrays(cases), S.new_block(len(cases))), len(cases)), want)
    plans = [R.good_plan(1300 + i, lead=2, ovk=True, memo=False) for i in range(3)]
    want = [R.reference(p) for p in plans]
    for memos, flags in ((False, True), (True, False), (False, False)):
        R.check(S.results(S.stage_host(0, R.arrays(plans, memos=memos, flags=flags), S.new_block(3)), 3), want)
