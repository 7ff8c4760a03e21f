"""Spend descriptions without their proofs on the GPU (masp_hip_sapling_build_spends, k_spend_build.hip) through the C ABI, against the
host twin (masp_host_sapling_build_spends) and spend_build_ref's composition of vector-pinned primitives; the product's kernels one by one
through the test-side shim against the header's CPU result for the same step; and the chain from notes to signed spend descriptions on
one context.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import masp_amd
import spend_build_ref as R
import spend_build_shim as S
from masp_amd import host as H
from masp_amd import note_encryption as NE
from masp_amd import redjubjub as RJS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def _same(got, want):
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def _refused_at(spends, want, positions):
    """the spends with those at `positions` refused, the nine statuses in turn from `first`"""
    spends, want = list(spends), list(want)
    for j, i in enumerate(sorted({p for p in positions if 0 <= p < len(spends)})):
        spends[i] = R.spoil(R.good_spend(2000 + i), 1 + (i + 2 * j) % 9, j)
        want[i] = R.reference(spends[i])
    return spends, want


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_against_the_host_twin_and_the_reference(ctx, n):
    spends, want = _refused_at(*R.batch(n), (0, 63, 64, n - 1) if n > 1 else ())
    assert {p["lead"] for p in spends} >= {1, 2} or n == 1       # (a refused spend may carry any lead byte)
    arrays = R.arrays(spends)
    got = ctx.build_spends(*arrays)
    assert [a.shape for a in got] == [(n,)] + [(n, 32)] * 5
    _same(got, H.build_spends(*arrays, threads=4))
    R.check(got, want)
    assert len(ctx.build_spends_last_timing()) == 3


def test_chunks_give_the_same_bytes(ctx):
    spends, want = _refused_at(*R.batch(130), (0, 63, 64, 129))
    arrays = R.arrays(spends)
    whole = ctx.build_spends(*arrays)
    R.check(whole, want)
    for chunk in (64, 1, 128):
        ctx.build_spends_configure(chunk)     # 64: three chunks, the last partial
        try:
            _same(ctx.build_spends(*arrays), whole)
        finally:
            ctx.build_spends_configure(0)
    with pytest.raises(masp_amd.MaspHipError):
        ctx.build_spends_configure((1 << 16) + 1)     # above the default


def test_edge_scalars_and_every_status(ctx):
    spends, want = R.references("edge_spends", R.edge_spends)
    R.check(ctx.build_spends(*R.arrays(spends)), want)
    cases = [p for b, bad, _ in R.status_spends() for p in (b, bad)]
    want = [R.reference(p) for p in cases]
    assert {w[0] for w in want} == set(range(10))
    R.check(ctx.build_spends(*R.arrays(cases)), want)
    doubles = R.double_spends()
    assert ctx.build_spends(*R.arrays([d for d, _ in doubles]))[0].tolist() == [s for _, s in doubles]
    R.check(ctx.build_spends(*R.arrays(cases), want_cmus=False, want_nks=False), want)


def _call(ctx, n, args, res, drop=()):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return ctx._L.masp_hip_sapling_build_spends(ctx._h, n, *ptrs)


def test_argument_rules(ctx):
    spends = [R.good_spend(1600 + i) for i in range(3)]
    args, want = R.arrays(spends), [R.reference(p) for p in spends]
    assert _call(ctx, 0, [None] * 11, [None] * 6) == 0              # n = 0 reads nothing
    res = H.build_spend_results(3)
    assert _call(ctx, 3, args, res) == 0
    R.check(res, want)
    for drop in ((15,), (16,), (15, 16)):                           # cmus_out, nks_out NULL
        res = H.build_spend_results(3)
        assert _call(ctx, 3, args, res, drop=drop) == 0
        R.check([None if 11 + k in drop else a for k, a in enumerate(res)], want)
    for i in range(15):                                             # MASP_HIP_E_INVALID_ARG, nothing written
        res = H.build_spend_results(3)
        assert _call(ctx, 3, args, res, drop=(i,)) == 1, i
        assert not any(a.any() for a in res)
    assert _call(ctx, (1 << 20) + 1, args, res) == 1
    assert NE.batch.build_spends([], ctx) == []


def test_each_kernel_alone_against_the_headers_step():
    spends, want = _refused_at(*R.batch(130), (0, 63, 64, 129))
    arrays = R.arrays(spends)
    block = S.spend.new_block(130)
    for k, name in enumerate(S.SPEND_STAGES, 1):
        cpu = S.spend.stage_host(k, arrays, block)
        gpu = S.spend.stage_gpu(k, arrays, block)     # the kernel alone, fed the CPU's result of the steps before it
        a, b = S.spend.parts(gpu, 130)[0], S.spend.parts(cpu, 130)[0]
        differ = [part for part in S.SPEND_PARTS if a[part].tobytes() != b[part].tobytes()]
        assert not differ, (name, differ)
        assert cpu.tobytes() != block.tobytes(), name     # every step leaves something
        block = cpu
    R.check(S.spend_results(block, 130), want)
    R.check(S.spend_results(S.spend.stage_gpu(0, arrays, S.spend.new_block(130)), 130), want)     # and the five in the product's order


def test_notes_to_signed_spend_descriptions(ctx):
    """65 notes of one spending key: build_spends, spend_sigs, SpendDescriptions whose rk and signature verify on the same context"""
    rng = __import__("random").Random(9)
    ask, nsk, sighash = rng.randrange(R.RJ), R._le(rng.randrange(R.RJ)), rng.randbytes(32)
    ak = H.jubjub_mul(R.G_SPEND, ask)
    spends = [dict(R.good_spend(2200 + i), ak=ak, nsk=nsk) for i in range(65)]
    built = NE.batch.build_spends(R.as_plans(spends), ctx)
    assert built == [R.reference(p)[1:] for p in spends] and all(b[4] == H.jubjub_mul(R.G_PGK, nsk) for b in built)
    sigs = RJS.spend_sigs([ask] * 65, [p["ar"] for p in spends], sighash, ctx)
    descs = [masp_amd.SpendDescription(cv, bytes(32), nf, rk, bytes(192), sig) for (cv, rk, nf, _, _), (rk2, sig) in zip(built, sigs) if rk == rk2]
    assert len(descs) == 65
    assert ctx.redjubjub_verify_each([(d.rk, d.spend_auth_sig, sighash, 0) for d in descs]) == [True] * 65
    assert all(RJS.verify(d.rk, d.rk + sighash, d.spend_auth_sig, R.G_SPEND) for d in descs[:3])
    items = [(NE.Note(p["asset"], p["value"], p["pk_d"], NE.Rseed(p["lead"], p["rseed"])), NE.PaymentAddress(p["d"], p["pk_d"]), b[4], p["position"])
             for p, b in zip(spends, built)]
    assert NE.batch.note_nullifiers(items, ctx) == [(b[3], b[2]) for b in built]
