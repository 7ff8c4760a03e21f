"""Spend descriptions without their proofs and RedJubjub signatures on the host (masp_host_sapling_build_spends,
masp_host_redjubjub_sign_batch, note_encryption.batch.build_spends, redjubjub.sign_batch and spend_sigs with ctx=None) against
spend_build_ref's composition of vector-pinned primitives.  CPU only; every comparison is of bytes."""
import ctypes

import numpy as np

import spend_build_ref as R
from masp_amd import host as H
from masp_amd import note_encryption as NE
from masp_amd import prover as P
from masp_amd import redjubjub as RJS


# ---- signatures ----
def test_sign_edges_and_a_random_batch():
    items, want = R.references("edge_items", R.edge_items, R.sign_reference)
    assert [w[0] for w in want] == [0] * len(items)
    R.check_signs(H.redjubjub_sign_batch(*R.sign_arrays(items), threads=1), want)
    items, want = R.sign_batch(130)
    assert {w[0] for w in want} == {0, 1, 2}
    one = H.redjubjub_sign_batch(*R.sign_arrays(items), threads=1)
    R.check_signs(one, want)
    many = H.redjubjub_sign_batch(*R.sign_arrays(items), threads=16)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))
    R.check_signs(H.redjubjub_sign_batch(*R.sign_arrays(items), threads=2, want_vks=False), want)


def test_sign_every_status_next_to_its_control():
    cases = R.status_items()
    assert {s for _, _, s in cases} == {1, 2}
    flat = [it for b, bad, _ in cases for it in (b, bad)]
    got = H.redjubjub_sign_batch(*R.sign_arrays(flat), threads=1)
    assert got[0].tolist() == [x for _, _, s in cases for x in (0, s)]
    R.check_signs(got, [R.sign_reference(it) for it in flat])
    doubles = R.double_items()
    assert H.redjubjub_sign_batch(*R.sign_arrays([d for d, _ in doubles]), threads=1)[0].tolist() == [s for _, s in doubles]


def test_sign_a_refused_item_between_two_good_ones():
    a, b = R.good_item(1201), R.good_item(1202)
    alone = H.redjubjub_sign_batch(*R.sign_arrays([a, b]), threads=1)
    for s in (1, 2):
        got = H.redjubjub_sign_batch(*R.sign_arrays([a, R.spoil_item(R.good_item(1203), s), b]), threads=1)
        assert got[0].tolist() == [0, s, 0]
        for k in (1, 2):
            assert got[k][0].tobytes() == alone[k][0].tobytes() and got[k][2].tobytes() == alone[k][1].tobytes() and not got[k][1].any()


def test_sign_without_alphas_is_the_binding_signatures_case():
    items = [R.good_item(1300 + i, kind=i % 2, alpha=False) for i in range(5)]
    want = [R.sign_reference(it) for it in items]
    R.check_signs(H.redjubjub_sign_batch(*R.sign_arrays(items, alphas=False), threads=1), want)
    R.check_signs(H.redjubjub_sign_batch(*R.sign_arrays(items), threads=1), want)       # explicit zero alphas: the same
    # kind 1 against SaplingProvingContext.binding_sig's key and signature
    ctx = P.SaplingProvingContext()
    ctx._bsk_add(R._le(123456789))
    ctx.cv_sum = RJS.public_key(ctx.bsk, R.G_VCR)            # (a transaction whose values balance: bvk = [bsk] G_vcr)
    sighash, T = bytes(range(32)), bytes(range(80))
    sig = ctx.binding_sig([], sighash, rng=lambda n: T[:n])
    status, vks, sigs = H.redjubjub_sign_batch(R._le(ctx.bsk), None, sighash, [1], T, threads=1)
    assert (int(status[0]), vks[0].tobytes(), sigs[0].tobytes()) == (0, ctx.cv_sum, sig)


def _sign_call(L, n, args, res, threads=1, drop=()):
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return L.masp_host_redjubjub_sign_batch(n, *ptrs, threads)


def _sign_results(n):
    return np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)


def test_sign_argument_rules():
    L = H.load_library()
    items = [R.good_item(1400 + i) for i in range(3)]
    args, want = R.sign_arrays(items), [R.sign_reference(it) for it in items]
    assert _sign_call(L, 0, [None] * 5, [None] * 3) == 0            # n = 0 reads nothing
    res = _sign_results(3)
    assert _sign_call(L, 3, args, res) == 0
    R.check_signs(res, want)
    res = _sign_results(3)
    assert _sign_call(L, 3, args, res, drop=(6,)) == 0               # vks_out NULL
    R.check_signs((res[0], None, res[2]), want)
    for i in (0, 2, 3, 4, 5, 7):                                    # any other NULL array: MASP_HOST_E_INVALID (1), nothing written
        res = _sign_results(3)
        assert _sign_call(L, 3, args, res, drop=(i,)) == 1, i
        assert not any(a.any() for a in res)
    bad = list(args)
    bad[3] = np.array([0, 2, 1], np.uint8)                          # kind 2
    res = _sign_results(3)
    assert _sign_call(L, 3, bad, res) == 1 and not any(a.any() for a in res)
    assert _sign_call(L, (1 << 20) + 1, args, res) == 1


# ---- spends ----
def test_spend_edges_and_a_random_batch():
    spends, want = R.references("edge_spends", R.edge_spends)
    assert [w[0] for w in want] == [0] * len(spends)
    R.check(H.build_spends(*R.arrays(spends), threads=2), want)
    spends, want = R.batch(130)
    assert {w[0] for w in want} == set(range(10))
    one = H.build_spends(*R.arrays(spends), threads=1)
    R.check(one, want)
    many = H.build_spends(*R.arrays(spends), threads=16)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))
    R.check(H.build_spends(*R.arrays(spends), threads=2, want_cmus=False, want_nks=False), want)


def test_spend_every_status_next_to_its_control_and_in_its_order():
    cases = R.status_spends()
    assert {s for _, _, s in cases} == set(range(1, 10))
    flat = [p for b, bad, _ in cases for p in (b, bad)]
    got = H.build_spends(*R.arrays(flat), threads=1)
    assert got[0].tolist() == [x for _, _, s in cases for x in (0, s)]
    R.check(got, [R.reference(p) for p in flat])
    doubles = R.double_spends()
    assert H.build_spends(*R.arrays([d for d, _ in doubles]), threads=1)[0].tolist() == [s for _, s in doubles]


def test_spend_a_refused_one_between_two_good_ones():
    a, b = R.good_spend(1501), R.good_spend(1502)
    alone = H.build_spends(*R.arrays([a, b]), threads=1)
    for s in range(1, 10):
        got = H.build_spends(*R.arrays([a, R.spoil(R.good_spend(1503), s), b]), threads=1)
        assert got[0].tolist() == [0, s, 0]
        for k in range(1, 6):
            assert got[k][0].tobytes() == alone[k][0].tobytes() and got[k][2].tobytes() == alone[k][1].tobytes() and not got[k][1].any()


def _spend_call(L, n, args, res, threads=1, drop=()):
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return L.masp_host_sapling_build_spends(n, *ptrs, threads)


def test_spend_argument_rules():
    L = H.load_library()
    spends = [R.good_spend(1600 + i) for i in range(3)]
    args, want = R.arrays(spends), [R.reference(p) for p in spends]
    assert _spend_call(L, 0, [None] * 11, [None] * 6) == 0          # n = 0 reads nothing
    res = H.build_spend_results(3)
    assert _spend_call(L, 3, args, res) == 0
    R.check(res, want)
    for drop in ((15,), (16,), (15, 16)):                           # cmus_out, nks_out NULL
        res = H.build_spend_results(3)
        assert _spend_call(L, 3, args, res, drop=drop) == 0
        R.check([None if 11 + k in drop else a for k, a in enumerate(res)], want)
    for i in range(15):                                             # any other NULL array: MASP_HOST_E_INVALID (1), nothing written
        res = H.build_spend_results(3)
        assert _spend_call(L, 3, args, res, drop=(i,)) == 1, i
        assert not any(a.any() for a in res)
    assert _spend_call(L, (1 << 20) + 1, args, res) == 1


# ---- the Python surface ----
def test_batch_calls_on_the_host():
    import masp_amd
    assert masp_amd.sign_batch is RJS.sign_batch and masp_amd.spend_sigs is RJS.spend_sigs
    assert NE.batch.build_spends([], None) == [] and RJS.sign_batch([], None) == [] and RJS.spend_sigs([], [], bytes(32), None) == []
    spends, want = R.batch(24)
    got = NE.batch.build_spends(R.as_plans(spends), None, threads=2)
    assert [None if w[0] else tuple(w[1:]) for w in want] == got and any(g is None for g in got) and any(g for g in got)
    items, want = R.sign_batch(24)
    draws = iter([it["T"] for it in items])
    got = RJS.sign_batch([(it["sk"], it["alpha"], it["sighash"], it["kind"]) for it in items], None, threads=2, rng=lambda n: next(draws)[:n])
    assert [None if w[0] else (w[1], w[2]) for w in want] == got and any(g is None for g in got)
    # the builder's loop: one sighash, a spend's ask randomised by its ar; the rk is build_spends' rk for ak = [ask] G_spend
    rng = __import__("random").Random(7)
    asks, ars, sighash = [rng.randrange(R.RJ) for _ in range(5)], [R._le(rng.randrange(R.RJ)) for _ in range(5)], rng.randbytes(32)
    sigs = RJS.spend_sigs(asks, ars, sighash, None, threads=1)
    for ask, ar, (rk, sig) in zip(asks, ars, sigs):
        spend = dict(R.good_spend(1700), ak=H.jubjub_mul(R.G_SPEND, ask), ar=ar)
        assert R.reference(spend)[2] == rk and RJS.verify(rk, rk + sighash, sig, R.G_SPEND)
    assert RJS.spend_sigs([R.RJ], [0], sighash, None) == [None]
