"""Output descriptions without their proofs on the GPU (masp_hip_sapling_build_outputs, k_output_build.hip) through the C ABI, against
the host twin (masp_host_sapling_build_outputs) and output_build_ref's composition of vector-pinned primitives; the product's kernels one
by one through the test-side shim against the header's CPU result for the same step; and the outputs read back by the three scans on the
same context.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import masp_amd
import output_build_ref as R
import output_build_shim as S
from masp_amd import host as H
from masp_amd import note_encryption as NE

pytestmark = pytest.mark.gpu
N_IN, N_OUT = 12, 6


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def _same(got, want):
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_sizes_against_the_host_twin_and_the_reference(ctx):
    for n in (0, 1, 7, 63, 64, 65, 130, 257):
        plans, want = R.batch(n)
        arrays = R.arrays(plans)
        got = ctx.build_outputs(*arrays)
        assert [a.shape for a in got] == [(n,), (n, 32), (n, 32), (n, 32), (n, 612), (n, 80)]
        _same(got, H.build_outputs(*arrays, threads=4))
        R.check(got, want)
    assert len(ctx.build_outputs_last_timing()) == 3


def test_chunks_give_the_same_bytes(ctx):
    plans, want = R.batch(257)
    arrays = R.arrays(plans)
    whole = ctx.build_outputs(*arrays)
    for chunk in (64, 1, 128):
        ctx.build_outputs_configure(chunk)     # 64: five chunks, the last partial
        try:
            chunked = ctx.build_outputs(*arrays)
        finally:
            ctx.build_outputs_configure(0)
        R.check(chunked, want)
        _same(chunked, whole)


def test_null_memos_and_null_flags(ctx):
    plans = [R.good_plan(1300 + i, lead=2, ovk=True, memo=False) for i in range(70)]
    want = [R.reference(p) for p in plans]
    for memos, flags in ((True, True), (False, True), (True, False), (False, False)):
        R.check(ctx.build_outputs(*R.arrays(plans, memos=memos, flags=flags)), want)


def test_every_status_next_to_its_control(ctx):
    cases, want = R.references("status", lambda: [p for c, b, _ in R.status_plans() for p in (c, b)])
    R.check(ctx.build_outputs(*R.arrays(cases)), want)
    doubles = R.double_plans()
    assert ctx.build_outputs(*R.arrays([b for b, _ in doubles]))[0].tolist() == [s for _, s in doubles]
    zero = R.zero_esk_plan()
    R.check(ctx.build_outputs(*R.arrays([zero])), [R.reference(zero)])


def test_a_thousand_plans_one_in_ten_refused(ctx):
    plans, want = R.batch(1000)
    bad = [i for i, w in enumerate(want) if w[0]]
    assert 50 < len(bad) < 200 and {want[i][0] for i in bad} == {1, 2, 3, 4, 5, 6}
    got = ctx.build_outputs(*R.arrays(plans))
    for i in bad:
        assert not any(got[k][i].any() for k in range(1, 6))
    R.check(got, want)     # the neighbours are intact


def _call(ctx, n, args, res, drop=()):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return ctx._L.masp_hip_sapling_build_outputs(ctx._h, n, *ptrs)


def test_argument_rules(ctx):
    plans = [R.good_plan(1300 + i, lead=2, ovk=True, memo=False) for i in range(3)]
    args, res = R.arrays(plans), H.build_output_results(3)
    assert _call(ctx, 0, [None] * N_IN, [None] * N_OUT) == 0            # n = 0 reads nothing
    assert _call(ctx, 3, args, res) == 0
    R.check(res, [R.reference(p) for p in plans])
    for i in [0, 1, 2, 3, 4, 5, 7, 9] + list(range(N_IN, N_IN + N_OUT)):     # MASP_HIP_E_INVALID_ARG, nothing written
        res2 = H.build_output_results(3)
        assert _call(ctx, 3, args, res2, drop=(i,)) == 1, i
        assert not any(a.any() for a in res2)
    a1 = list(R.arrays([R.good_plan(1310, lead=1, ovk=True)] + plans[:2]))
    assert _call(ctx, 3, a1, H.build_output_results(3)) == 0 and _call(ctx, 3, a1, H.build_output_results(3), drop=(6,)) == 1
    a2 = list(R.arrays([R.good_plan(1311, lead=2, ovk=False)] + plans[:2]))
    assert _call(ctx, 3, a2, H.build_output_results(3)) == 0 and _call(ctx, 3, a2, H.build_output_results(3), drop=(11,)) == 1
    assert _call(ctx, 3, a2, H.build_output_results(3), drop=(10, 11)) == 0
    assert _call(ctx, (1 << 20) + 1, args, res) == 1
    with pytest.raises(masp_amd.MaspHipError):
        ctx.build_outputs_configure((1 << 16) + 1)     # above the default
    assert NE.batch.build_outputs([], ctx) == []


def test_each_kernel_alone_against_the_headers_step():
    plans, want = R.batch(130)
    arrays = R.arrays(plans)
    block = S.new_block(130)
    for k, name in enumerate(S.STAGES, 1):
        cpu = S.stage_host(k, arrays, block)
        gpu = S.stage_gpu(k, arrays, block)     # the kernel alone, fed the CPU's result of the steps before it
        a, b = S.parts(gpu, 130), S.parts(cpu, 130)
        differ = [part for part in S.PARTS if a[part].tobytes() != b[part].tobytes()]
        assert not differ, (name, differ)
        assert cpu.tobytes() != block.tobytes(), name     # every step leaves something
        block = cpu
    R.check(S.results(block, 130), want)
    R.check(S.results(S.stage_gpu(0, arrays, S.new_block(130)), 130), want)     # and the seven in the product's order


def test_built_outputs_are_found_by_the_three_scans(ctx):
    """64 outputs for 4 recipients and 3 ovks, built on the GPU, read back on the same context"""
    ivks = [R._le(7000 + 13 * r) for r in range(4)]
    ovks = [bytes([0x40 + k]) * 32 for k in range(3)]
    plans, owner = [], []
    for i in range(64):
        p = R.good_plan(1600 + i, lead=2, ovk=True)
        r, k = i % 5, i % 4                       # r = 4: nobody's; k = 3: an ovk outside the list
        ivk = ivks[r] if r < 4 else R._le(99991)
        p = dict(p, pk_d=H.jubjub_mul(H.diversifier_base(p["d"]), ivk), ovk=ovks[k] if k < 3 else bytes([0x77]) * 32)
        if i % 16 == 9:
            p = dict(p, ovk=None, out_random=bytes([i]) * 96)
            k = 3
        plans.append(p)
        owner.append((r if r < 4 else None, k if k < 3 else None))
    outs = NE.batch.build_outputs(R.as_plans(plans), ctx)
    assert all(isinstance(o, NE.OutputDescription) for o in outs)
    assert [tuple(o) for o in outs] == [R.reference(p)[1:] for p in plans]
    expect = lambda p: (NE.Note(p["asset"], p["value"], p["pk_d"], NE.Rseed(2, p["rseed"])), NE.PaymentAddress(p["d"], p["pk_d"]),
                        p["memo"] if p["memo"] is not None else NE.EMPTY_MEMO)
    full = NE.batch.try_note_decryption(ivks, [NE.ShieldedOutput(o.epk, o.cmu, o.enc_ciphertext) for o in outs], ctx)
    compact = NE.batch.try_compact_note_decryption(ivks, [NE.compact_output(o) for o in outs], ctx)
    recovered = NE.batch.try_output_recovery(ovks, outs, ctx)
    for p, (r, k), f, c, v in zip(plans, owner, full, compact, recovered):
        assert f == (None if r is None else (expect(p), r))
        assert c == (None if r is None else (expect(p)[:2], r))
        assert v == (None if k is None else (expect(p), k))
    assert sum(f is not None for f in full) == 52 and sum(v is not None for v in recovered) > 40
