"""RedJubjub signatures on the GPU (masp_hip_redjubjub_sign_batch, k_spend_build.hip) through the C ABI, against the host twin
(masp_host_redjubjub_sign_batch) and spend_build_ref's composition of vector-pinned primitives; the product's kernels one by one through
the test-side shim against the header's CPU result for the same step; and the signatures read back by the two verifiers on the same
context.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import masp_amd
import spend_build_ref as R
import spend_build_shim as S
from masp_amd import host as H
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


def _refused_at(items, want, positions):
    """the items with those at `positions` refused, status 1 and 2 in turn"""
    items, want = list(items), list(want)
    for j, i in enumerate(sorted({p for p in positions if 0 <= p < len(items)})):
        items[i] = R.spoil_item(R.good_item(2000 + i), 1 + j % 2, j)
        want[i] = R.sign_reference(items[i])
    return items, want


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_against_the_host_twin_and_the_reference(ctx, n):
    items, want = _refused_at(*R.sign_batch(n), (0, 63, 64, n - 1) if n > 1 else ())
    arrays = R.sign_arrays(items)
    got = ctx.redjubjub_sign_batch(*arrays)
    assert [a.shape for a in got] == [(n,), (n, 32), (n, 64)]
    _same(got, H.redjubjub_sign_batch(*arrays, threads=4))
    R.check_signs(got, want)
    assert len(ctx.redjubjub_sign_last_timing()) == 3


def test_chunks_give_the_same_bytes(ctx):
    items, want = _refused_at(*R.sign_batch(130), (0, 63, 64, 129))
    arrays = R.sign_arrays(items)
    whole = ctx.redjubjub_sign_batch(*arrays)
    R.check_signs(whole, want)
    for chunk in (64, 1, 128):
        ctx.redjubjub_sign_configure(chunk)     # 64: three chunks, the last partial
        try:
            _same(ctx.redjubjub_sign_batch(*arrays), whole)
        finally:
            ctx.redjubjub_sign_configure(0)
    with pytest.raises(masp_amd.MaspHipError):
        ctx.redjubjub_sign_configure((1 << 16) + 1)     # above the default


def test_edge_scalars_and_every_status(ctx):
    items, want = R.references("edge_items", R.edge_items, R.sign_reference)
    R.check_signs(ctx.redjubjub_sign_batch(*R.sign_arrays(items)), want)
    cases = [it for b, bad, _ in R.status_items() for it in (b, bad)] + [d for d, _ in R.double_items()]
    R.check_signs(ctx.redjubjub_sign_batch(*R.sign_arrays(cases)), [R.sign_reference(it) for it in cases])
    plain = [R.good_item(1800 + i, kind=i % 2, alpha=False) for i in range(5)]
    R.check_signs(ctx.redjubjub_sign_batch(*R.sign_arrays(plain, alphas=False), want_vks=False), [R.sign_reference(it) for it in plain])


def _call(ctx, n, args, res, drop=()):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ptrs = [vp(a) for a in list(args) + list(res)]
    for i in drop:
        ptrs[i] = None
    return ctx._L.masp_hip_redjubjub_sign_batch(ctx._h, n, *ptrs)


def _results(n):
    return np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)


def test_argument_rules(ctx):
    items = [R.good_item(1400 + i) for i in range(3)]
    args, want = R.sign_arrays(items), [R.sign_reference(it) for it in items]
    assert _call(ctx, 0, [None] * 5, [None] * 3) == 0               # n = 0 reads nothing
    res = _results(3)
    assert _call(ctx, 3, args, res) == 0
    R.check_signs(res, want)
    res = _results(3)
    assert _call(ctx, 3, args, res, drop=(6,)) == 0                  # vks_out NULL
    R.check_signs((res[0], None, res[2]), want)
    for i in (0, 2, 3, 4, 5, 7):                                    # MASP_HIP_E_INVALID_ARG, nothing written
        res = _results(3)
        assert _call(ctx, 3, args, res, drop=(i,)) == 1, i
        assert not any(a.any() for a in res)
    bad = list(args)
    bad[3] = np.array([0, 2, 1], np.uint8)                          # kind 2
    res = _results(3)
    assert _call(ctx, 3, bad, res) == 1 and not any(a.any() for a in res)
    assert _call(ctx, (1 << 20) + 1, args, res) == 1
    assert RJS.sign_batch([], ctx) == []


def test_each_kernel_alone_against_the_headers_step():
    items, want = _refused_at(*R.sign_batch(130), (0, 63, 64, 129))
    arrays = R.sign_arrays(items)
    block = S.sign.new_block(130)
    for k, name in enumerate(S.SIGN_STAGES, 1):
        cpu = S.sign.stage_host(k, arrays, block)
        gpu = S.sign.stage_gpu(k, arrays, block)     # the kernel alone, fed the CPU's result of the steps before it
        a, b = S.sign.parts(gpu, 130)[0], S.sign.parts(cpu, 130)[0]
        differ = [part for part in S.SIGN_PARTS if a[part].tobytes() != b[part].tobytes()]
        assert not differ, (name, differ)
        assert cpu.tobytes() != block.tobytes(), name     # every step leaves something
        block = cpu
    R.check_signs(S.sign_results(block, 130), want)
    R.check_signs(S.sign_results(S.sign.stage_gpu(0, arrays, S.sign.new_block(130)), 130), want)     # and the four in the product's order


def test_signatures_round_trip_through_the_device_verifiers(ctx):
    items = [R.good_item(2100 + i) for i in range(65)]
    draws = iter([it["T"] for it in items])
    signed = RJS.sign_batch([(it["sk"], it["alpha"], it["sighash"], it["kind"]) for it in items], ctx, rng=lambda n: next(draws)[:n])
    assert signed == [R.sign_reference(it)[1:] for it in items]
    checks = [(vk, sig, it["sighash"], it["kind"]) for it, (vk, sig) in zip(items, signed)]
    assert ctx.redjubjub_verify_each(checks) == [True] * 65
    assert ctx.redjubjub_verify_batch(checks, randomness=bytes(range(1, 17)) * 65)
    flip = lambda b, bit: bytes(x ^ (1 << (bit % 8)) if j == bit // 8 else x for j, x in enumerate(b))
    bad = list(checks)
    bad[3] = (bad[3][0], flip(bad[3][1], 256 + 5), bad[3][2], bad[3][3])       # one bit of an S
    bad[40] = (bad[40][0], flip(bad[40][1], 17), bad[40][2], bad[40][3])       # one bit of an Rbar
    bad[64] = (bad[64][0], bad[64][1], flip(bad[64][2], 100), bad[64][3])      # one bit of a sighash
    assert ctx.redjubjub_verify_each(bad) == [i not in (3, 40, 64) for i in range(65)]
    assert not ctx.redjubjub_verify_batch(bad, randomness=bytes(range(1, 17)) * 65)
