"""A conversion tree's leaves on the GPU (masp_hip_sapling_allowed_conversions, k_conversion.hip) through the C ABI, against the host twin
(masp_host_allowed_conversions) and conversion_ref's composition of vector-pinned primitives; the product's kernels for both lane widths
through the test-side shim; the Convert circuit as judge of the whole path.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import conversion_ref as R
import conversion_shim as S
import masp_amd
import nullifier_ref as NR
from masp_amd import FrozenCommitmentTree
from masp_amd import host as H
from masp_amd.convert import AllowedConversion, batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def _same(got, want):
    for x, y in zip(got, want):
        assert (x is None and y is None) or np.array_equal(x, y)


def test_sizes_against_the_host_twin_and_the_reference(ctx):
    convs, want = R.references("random130")
    status = [w[0] for w in want]
    assert status.count(0) >= 40 and status.count(1) >= 10 and status.count(2) >= 5
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 130):
        arrays = R.arrays(convs[:n])
        host = H.allowed_conversions(*arrays, threads=4)
        got = ctx.allowed_conversions(*arrays)
        _same(got, host)
        R.check(got, want[:n])
        status, gens, cmus = ctx.allowed_conversions(*arrays, want_generators=False)      # generators_out = NULL
        assert gens is None
        _same((status, cmus), (host[0], host[2]))


def test_edge_list(ctx):
    convs, want = R.references("edges")
    status, gens, cmus = ctx.allowed_conversions(*R.arrays(convs))
    R.check((status, gens, cmus), want)
    assert gens[R.edge("empty")].tobytes() == H.JUBJUB_IDENTITY == gens[R.edge("cancels")].tobytes()
    assert gens[R.edge("order 1")].tobytes() == gens[R.edge("order 2")].tobytes() and cmus[R.edge("order 1")].tobytes() == cmus[R.edge("order 2")].tobytes()
    assert gens[R.edge("bit 255")][31] & 0x80


def test_forced_lane_widths_give_the_same_bytes(ctx):
    convs, want = R.references("random130")
    arrays = R.arrays(convs + [t for _, t in R.edge_conversions()][-3:])           # ... and the conversions of 3, 17 and 300 terms
    first = ctx.allowed_conversions(*arrays)
    R.check(tuple(a[:130] for a in first), want)
    try:
        for lanes in (1, 8):
            ctx.allowed_conversions_configure(lanes)
            _same(ctx.allowed_conversions(*arrays), first)
    finally:
        ctx.allowed_conversions_configure(0)
    up, kernels, down = ctx.allowed_conversions_last_timing()
    assert kernels > 0 and up >= 0 and down >= 0


@pytest.mark.parametrize("n", [1, 7, 9, 65])
def test_the_kernels_alone_for_both_lane_widths(n):
    convs, want = R.references("random130")
    arrays = R.arrays(convs[3:3 + n])
    one, eight = S.run_gpu(*arrays, 1), S.run_gpu(*arrays, 8)
    _same(one, eight)
    R.check(one, want[3:3 + n])


def test_the_kernels_alone_on_the_edges():
    convs, want = R.references("edges")
    for lanes in (1, 8):
        R.check(S.run_gpu(*R.arrays(convs), lanes), want)


def test_chunks(ctx):
    convs, _ = R.references("random130")
    edges = dict(R.edge_conversions())
    arrays = R.arrays(convs + [edges["17 terms"]])
    whole = ctx.allowed_conversions(*arrays)
    try:
        # chunks of at most 5 conversions and 17 terms: the 17-term conversion fills one to the brim.  (A limit of 16 terms, one fewer,
        # refuses that conversion by the call's own rule: below.)
        ctx.allowed_conversions_configure(0, 5, 17)
        _same(ctx.allowed_conversions(*arrays), whole)
        # one conversion of 300 terms, or of 17, against a chunk of 16: refused before any work, nothing written
        ctx.allowed_conversions_configure(0, 5, 16)
        for long in ("300 terms", "17 terms"):
            off, ids, vals = R.arrays(convs[:4] + [edges[long]])
            out = [np.full(5, 0xee, np.uint8), np.full((5, 32), 0xee, np.uint8), np.full((5, 32), 0xee, np.uint8)]
            p = [a.ctypes.data_as(C.c_void_p) for a in (off, ids, vals, *out)]
            assert ctx._L.masp_hip_sapling_allowed_conversions(ctx._h, 5, p[0], ids.shape[0], *p[1:]) == 1
            assert all((o == 0xee).all() for o in out)
        _same(ctx.allowed_conversions(*R.arrays(convs)), tuple(a[:130] for a in whole))   # (conversions of up to 5 terms: served)
    finally:
        ctx.allowed_conversions_configure(0, 0, 0)
    _same(ctx.allowed_conversions(*arrays), whole)                                  # the defaults again, the context still usable
    got = ctx.allowed_conversions(*R.arrays([edges["300 terms"]]))
    R.check(got, [R.reference(edges["300 terms"])])


def test_arguments(ctx):
    L, h = ctx._L, ctx._h
    call = L.masp_hip_sapling_allowed_conversions
    assert call(h, 0, None, 0, None, None, None, None, None) == 0                   # no conversions: nothing is read
    off, ids, vals = R.arrays([[(R.A, 1)], [(R.B, 2), (R.A, 3)]])
    out = [np.full(2, 0xee, np.uint8), np.full((2, 32), 0xee, np.uint8), np.full((2, 32), 0xee, np.uint8)]
    p = [a.ctypes.data_as(C.c_void_p) for a in (off, ids, vals, *out)]
    for k in (0, 1, 2, 3, 5):                                                       # every array but generators_out
        q = [None if i == k else x for i, x in enumerate(p)]
        assert call(h, 2, q[0], 3, *q[1:]) == 1, k
    for bad in ([1, 1, 3], [0, 2, 1], [0, 1, 2], [0, 4, 3]):                       # not from 0, decreasing, not to n_terms
        o = np.array(bad, np.uint64)
        assert call(h, 2, o.ctypes.data_as(C.c_void_p), 3, *p[1:]) == 1, bad
    assert call(h, (1 << 22) + 1, p[0], 3, *p[1:]) == 1
    assert all((o == 0xee).all() for o in out)                                      # nothing was written
    for bad in ((4, 0, 0), (2, 0, 0), (-1, 0, 0), (0, (1 << 19) + 1, 0), (0, 0, (1 << 20) + 1)):
        with pytest.raises(masp_amd.MaspHipError):
            ctx.allowed_conversions_configure(*bad)
    assert L.masp_hip_allowed_conversions_last_timing(h, None) == 1
    # conversions without terms: identifiers and values may be NULL
    status, gens, cmus = ctx.allowed_conversions([0, 0, 0], np.zeros((0, 32), np.uint8), np.zeros((0, 16), np.uint8))
    assert status.tolist() == [0, 0] and [g.tobytes() for g in gens] == [H.JUBJUB_IDENTITY] * 2
    assert cmus[0].tobytes() == R.reference([])[2] == cmus[1].tobytes()
    assert batch.allowed_conversions([], ctx) == []


def test_a_refused_conversion_between_two_good_ones(ctx):
    a, b = [(R.A, 5), (R.B, -6)], [(R.C3, 1 << 70)]
    alone = ctx.allowed_conversions(*R.arrays([a, b]))
    R.check(alone, [R.reference(a), R.reference(b)])
    for s, bad in ((1, [(R.A, 1), (R.BAD_ASSET, 2)]), (2, [(R.A, R.I128_MIN), (R.B, 2)])):
        status, gens, cmus = ctx.allowed_conversions(*R.arrays([a, bad, b]))
        assert status.tolist() == [0, s, 0]
        assert not gens[1].any() and not cmus[1].any()
        assert np.array_equal(gens[[0, 2]], alone[1]) and np.array_equal(cmus[[0, 2]], alone[2])


def test_next_to_the_nullifiers_and_the_trees(ctx):
    """the calls share the Pedersen table and the wallet's stream: one of each before and after still gives its known result"""
    notes, want_nf = NR.references("edges", NR.edge_notes)
    convs, want = R.references("random130")
    leaves = [w[2] for w in want if w[0] == 0][:21]
    root = FrozenCommitmentTree(leaves).root()
    for _ in range(2):
        NR.check(ctx.note_nullifiers(*NR.arrays(notes)), want_nf)
        assert FrozenCommitmentTree(leaves, ctx).root() == root
        R.check(ctx.allowed_conversions(*R.arrays(convs)), want)
    NR.check(ctx.note_nullifiers(*NR.arrays(notes)), want_nf)
    assert FrozenCommitmentTree(leaves, ctx).root() == root


def test_from_value_sums_to_a_satisfied_convert_circuit(ctx):
    sums = [[(R.ASSETS[k], 1 + k), (R.ASSETS[k + 1], -(2 + k)), (R.ASSETS[k + 2], (1 << 64) + k)] for k in range(11)]
    convs = batch.allowed_conversions(sums, ctx)
    assert all(isinstance(c, AllowedConversion) for c in convs)
    assert [(c.generator, c.cmu()) for c in convs] == [(c.generator, c.cmu()) for c in batch.allowed_conversions(sums, None)]
    tree = batch.conversion_tree(convs, ctx)
    assert tree.root() == batch.conversion_tree(convs, None).root()
    for pos in (0, 5, 10):
        path = tree.path(pos)
        inputs, _, _ = H.convert_assignment(convs[pos].generator, 900 + pos, tree.root(), path.siblings, pos, 31 + pos, check=True)
        assert inputs[3].tobytes() == tree.root()
    blobs = [c.write() for c in convs]
    tampered = blobs[4][:-32] + convs[5].generator
    got = batch.read_allowed_conversions(blobs + [tampered], ctx)
    assert [g.write() for g in got[:-1]] == blobs and [g.cmu() for g in got[:-1]] == [c.cmu() for c in convs]
    assert isinstance(got[-1], ValueError)
    mixed = batch.allowed_conversions([sums[0], [(R.BAD_ASSET, 1)], [(R.A, R.I128_MIN)]], ctx)
    assert mixed[0].generator == convs[0].generator and [m.status for m in mixed[1:]] == [1, 2]
