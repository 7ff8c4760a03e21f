"""Output descriptions without their proofs on the host (masp_host_sapling_build_outputs, note_encryption.batch.build_outputs with
ctx=None) against output_build_ref's composition of vector-pinned primitives; that composition against the reference's own note
encryption vectors and value commitments; and the results against the Output circuit's public inputs.  CPU only; every comparison is of
bytes."""
import ctypes
import json
import os

import output_build_ref as R
from masp_amd import host as H
from masp_amd import note_encryption as NE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_IN, N_OUT = 12, 6


def vector_plans():
    """the ten note encryption vectors as plans (lead byte 1: rcm and esk are given; the vectors carry no rcv)"""
    k = json.load(open(os.path.join(GOLDEN, "note_encryption_vectors.json")))
    h = bytes.fromhex
    return [(dict(asset=h(k["asset_identifier"]), value=tv["v"], d=h(tv["default_d"]), pk_d=h(tv["default_pk_d"]), lead=k["lead_byte"], rseed=h(tv["rcm"]),
                  esk=h(tv["esk"]), rcv=R._le(1), memo=h(tv["memo"]), ovk=h(tv["ovk"]), out_random=None), tv) for tv in k["vectors"]]


def test_the_reference_reproduces_the_note_encryption_vectors():
    vectors = vector_plans()
    assert len(vectors) == 10
    for p, tv in vectors:
        assert R.status_of(p) == 0 and R.plaintext(p).hex() == tv["p_enc"]
        rcm, esk = R.scalars(p)
        cmu = H.note_cmu(p["asset"], p["value"], p["d"], p["pk_d"], rcm)
        epk, k_enc, enc, ock, cout = R.seal(p, bytes.fromhex(tv["cv"]), cmu, esk)     # (ock and c_out from the vector's cv)
        assert (epk.hex(), k_enc.hex(), enc.hex(), cmu.hex()) == (tv["epk"], tv["k_enc"], tv["c_enc"], tv["cmu"])
        assert (ock.hex(), cout.hex()) == (tv["ock"], tv["c_out"])


def test_the_reference_and_the_host_twin_reproduce_the_value_commitments():
    k = json.load(open(os.path.join(GOLDEN, "value_commitments.json")))
    base = R.good_plan(5)
    plans = [dict(base, asset=bytes.fromhex(k["asset_identifier"]), value=i, rcv=R._le(1000 * (i + 1))) for i in range(10)]
    want = [R.reference(p) for p in plans]
    assert [H.point_uv(w[1]) for w in want] == [(int(u), int(v)) for u, v in zip(k["u"], k["v"])]
    R.check(H.build_outputs(*R.arrays(plans), threads=1), want)


def test_the_random_batch_has_everything():
    plans, want = R.batch(130)
    assert {w[0] for w in want} == {0, 1, 2, 3, 4, 5, 6}
    good = [p for p, w in zip(plans, want) if w[0] == 0]
    assert {p["lead"] for p in good} == {1, 2} and {p["ovk"] is None for p in good} == {True, False} and {p["memo"] is None for p in good} == {True, False}


def test_sizes_and_threads_against_the_reference():
    for n in (0, 1, 2, 17, 130):
        plans, want = R.batch(n)
        for threads in (1, 4):
            got = H.build_outputs(*R.arrays(plans), threads=threads)
            assert [a.shape for a in got] == [(n,), (n, 32), (n, 32), (n, 32), (n, 612), (n, 80)]
            R.check(got, want)


def test_every_status_next_to_its_control():
    cases, want = R.references("status", lambda: [p for c, b, _ in R.status_plans() for p in (c, b)])
    assert [w[0] for w in want] == [s for _, _, st in R.status_plans() for s in (0, st)]
    R.check(H.build_outputs(*R.arrays(cases), threads=1), want)
    doubles = R.double_plans()
    got = H.build_outputs(*R.arrays([b for b, _ in doubles]), threads=1)
    assert got[0].tolist() == [s for _, s in doubles]
    zero = R.zero_esk_plan()     # a zero esk is not refused: epk = [0] g_d, the identity
    got = H.build_outputs(*R.arrays([zero]), threads=1)
    R.check(got, [R.reference(zero)])
    assert int(got[0][0]) == 0 and got[3][0].tobytes() == R._le(1)


def test_a_bad_plan_between_two_good_ones():
    a, b = R.good_plan(1201), R.good_plan(1202)
    alone = H.build_outputs(*R.arrays([a, b]), threads=1)
    for s in range(1, 7):
        bad = R.spoil(R.good_plan(1203), s)
        got = H.build_outputs(*R.arrays([a, bad, b]), threads=1)
        assert got[0].tolist() == [0, s, 0]
        for k in range(1, 6):
            assert got[k][0].tobytes() == alone[k][0].tobytes() and got[k][2].tobytes() == alone[k][1].tobytes()
            assert not got[k][1].any()


def _call(L, n, args, res, threads=1, drop=()):
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return L.masp_host_sapling_build_outputs(n, *ptrs, threads)


def test_argument_rules():
    L = H.load_library()
    plans = [R.good_plan(1300 + i, lead=2, ovk=True, memo=False) for i in range(3)]
    args, res = R.arrays(plans), H.build_output_results(3)
    want = [R.reference(p) for p in plans]
    assert args[6] is None and args[11] is None                       # no lead byte 1: no esks; every ovk present: no out_randoms
    assert _call(L, 0, [None] * N_IN, [None] * N_OUT) == 0            # n = 0 reads nothing
    assert _call(L, 3, args, res) == 0
    R.check(res, want)
    # memos NULL = explicit empty memos, ovk_flags NULL = all-ones flags
    for drop in ((8,), (10,), (8, 10)):
        res2 = H.build_output_results(3)
        assert _call(L, 3, args, res2, drop=drop) == 0
        R.check(res2, want)
    # any other NULL array: MASP_HOST_E_INVALID (1), nothing written
    for i in [0, 1, 2, 3, 4, 5, 7, 9] + list(range(N_IN, N_IN + N_OUT)):
        res2 = H.build_output_results(3)
        assert _call(L, 3, args, res2, drop=(i,)) == 1, i
        assert not any(a.any() for a in res2)
    # esks NULL with a lead byte 1, out_randoms NULL with a flag 0
    lead1 = [R.good_plan(1310, lead=1, ovk=True)] + plans[:2]
    a1 = list(R.arrays(lead1))
    assert a1[6] is not None and _call(L, 3, a1, H.build_output_results(3)) == 0
    assert _call(L, 3, a1, H.build_output_results(3), drop=(6,)) == 1
    no_ovk = [R.good_plan(1311, lead=2, ovk=False)] + plans[:2]
    a2 = list(R.arrays(no_ovk))
    assert a2[11] is not None and _call(L, 3, a2, H.build_output_results(3)) == 0
    assert _call(L, 3, a2, H.build_output_results(3), drop=(11,)) == 1
    assert _call(L, 3, a2, H.build_output_results(3), drop=(10, 11)) == 0          # flags NULL: every ovk present, the randoms are not needed
    # n above 2^20 (refused before anything is read)
    assert _call(L, (1 << 20) + 1, args, res) == 1


def test_batch_build_outputs_round_trips_on_the_host():
    import masp_amd
    assert masp_amd.note_encryption.batch.build_outputs is NE.batch.build_outputs and set(NE.BUILD_OUTPUT_STATUS) == {1, 2, 3, 4, 5, 6}
    assert NE.batch.build_outputs([], None) == []
    plans = []
    for i in range(8):
        p = R.good_plan(1400 + i, lead=1 + i % 2, ovk=i % 4 != 3)
        ivk = R._le(1000 + i)
        p = dict(p, pk_d=H.jubjub_mul(H.diversifier_base(p["d"]), ivk), out_random=None)      # an address of a known ivk; os.urandom for ovk = None
        plans.append((p, ivk))
    plans.append((R.spoil(plans[0][0], 6), plans[0][1]))
    outs = NE.batch.build_outputs(R.as_plans([p for p, _ in plans]), None, threads=2)
    assert len(outs) == 9 and outs[8] is None
    other_ovk = bytes(range(32))
    for (p, ivk), out in zip(plans[:8], outs):
        assert isinstance(out, NE.OutputDescription)
        memo = p["memo"] if p["memo"] is not None else NE.EMPTY_MEMO
        note, to, got_memo = NE.try_sapling_note_decryption(ivk, NE.ShieldedOutput(out.epk, out.cmu, out.enc_ciphertext), p["lead"])
        assert (note.asset_identifier, note.value, note.pk_d, tuple(note.rseed), to.diversifier, got_memo) == \
            (p["asset"], p["value"], p["pk_d"], (p["lead"], p["rseed"]), p["d"], memo)
        if p["ovk"] is not None:
            assert NE.try_sapling_output_recovery(p["ovk"], out, p["lead"]) == (note, to, got_memo)
            want = R.reference(p)
            assert tuple(out) == want[1:]
        assert NE.try_sapling_output_recovery(other_ovk, out, p["lead"]) is None
        if p["ovk"] is None:
            assert NE.try_sapling_output_recovery(bytes(32), out, p["lead"]) is None
    # a given out_random makes the ovk-absent output a function of its inputs
    p = dict(plans[3][0], out_random=bytes(range(96)))
    assert p["ovk"] is None
    a, b = NE.batch.build_outputs(R.as_plans([p, p]), None)
    assert a == b and tuple(a) == R.reference(p)[1:]


def test_the_results_are_the_output_circuits_public_inputs():
    """cv, epk and cmu of the batch call are what the Output circuit exposes for the same secrets: its assignment's inputs are 1, cv.u, cv.v,
    epk.u, epk.v, cmu, and the synthesis (check=True) finds every constraint satisfied"""
    le = lambda x: int(x).to_bytes(32, "little")
    for seed in (1501, 1502, 1503):
        p = R.good_plan(seed, lead=1 + seed % 2)
        rcm, esk = R.scalars(p)
        status, cvs, cmus, epks, _, _ = H.build_outputs(*R.arrays([p]), threads=1)
        assert int(status[0]) == 0
        inputs, _, cv = H.output_assignment(esk, p["d"], p["pk_d"], rcm, p["asset"], p["value"], p["rcv"], check=True)
        assert cv == cvs[0].tobytes()
        want = [le(1)] + [le(c) for c in H.point_uv(cvs[0].tobytes())] + [le(c) for c in H.point_uv(epks[0].tobytes())] + [cmus[0].tobytes()]
        assert [row.tobytes() for row in inputs] == want
