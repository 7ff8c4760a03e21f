"""A block of leaves at an arbitrary offset on the GPU (masp_hip_merkle_tree_append, k_merkle.hip) through the C ABI, against the host twin
(masp_host_merkle_tree_append) over the same blocks and, for the small ones, against the definition in tests/incremental_ref.py; and
advance(..., ctx) on top of it against advance(ctx=None).  Every comparison is of bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import incremental_ref as IR
import masp_amd
import merkle_ref as R
from masp_amd import CommitmentTree, FrozenCommitmentTree, advance
from masp_amd import host as H
from masp_amd.merkle_tree import MT_BLOCK, MT_TOP_PARENTS     # the level kernels' workgroup size B and the hand-over T to the one-wave kernel

pytestmark = pytest.mark.gpu

Q = R.Q
B, T = MT_BLOCK, MT_TOP_PARENTS
FULL = 1 << 32
STARTS = [0, 1, 2, 3, 6, 7, (1 << 20) + 3]       # even and odd; 7: frontier entries 0, 1, 2; 2^20 + 3: entries 0, 1 and 20
COUNTS = [0, 1, 2, 3, 5, 37,
          2 * B, 2 * B + 1, 2 * B + 2,           # a parent row that exactly fills, and just overflows, one workgroup of k_mt_append_level
          2 * T, 2 * T + 2,                      # the widest level k_mt_append_top takes, and the narrowest that needs one k_mt_append_level
          4097]
GRID = [(s, n) for s in STARTS for n in COUNTS] + \
       [(FULL - 4, n) for n in (0, 1, 2, 3, 4)] + [(FULL - 1, 1)]    # the carry chain up to level 32, start + n = 2^32; every entry used
NOT_CANONICAL = Q.to_bytes(32, "little")


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def arr(nodes):
    return np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 32) if nodes else np.zeros((0, 32), np.uint8)


_host = {}


def host_block(start, n):
    """(frontier, row, the host twin's nodes), computed once; the unused frontier entries are bytes no node may have: they are never read"""
    if (start, n) not in _host:
        rng = random.Random(8000 + start % 1009 + n)
        frontier = [rng.randrange(Q).to_bytes(32, "little") if (start >> h) & 1 else b"\xff" * 32 for h in range(32)]
        row = R.random_nodes(n, 8100 + start % 1009 + n)
        _host[start, n] = (frontier, row, H.merkle_tree_append(start, arr(frontier), arr(row)))
    return _host[start, n]


@pytest.mark.parametrize("start,n", GRID)
def test_blocks_against_the_host_twin(ctx, start, n):
    frontier, row, want = host_block(start, n)
    got = ctx.merkle_tree_append(start, arr(frontier), arr(row))
    assert got.shape == want.shape == (H.merkle_append_node_count(start, n), 32)
    assert (got == want).all()
    if n <= 37:                                  # not only against new host code
        assert R.as_list(got) == IR.block_nodes(start, frontier, row)


def _raw(ctx, start, frontier, row, capacity, marker=0x5A):
    """the C call with the output pre-filled with a marker byte -> (rc, n_nodes, bad_index, nodes)"""
    f, r = arr(frontier), arr(row)
    nodes = np.full((max(capacity, 1), 32), marker, np.uint8)
    nn, bad = C.c_size_t(12345), C.c_int64(777)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.masp_hip_merkle_tree_append(ctx._h, start, vp(f), r.shape[0], vp(r) if r.shape[0] else None, vp(nodes), capacity, C.byref(nn),
                                            C.byref(bad))
    return rc, nn.value, bad.value, nodes


def test_nodes_that_are_not_canonical(ctx):
    start, n = 7, 2 * B + 2
    frontier, good, want = host_block(start, n)
    need = want.shape[0]
    bad_ff = b"\xff" * 32
    for places, first in (([0], 0), ([B - 1, B, n - 1], B - 1), ([B, 300], B), ([n - 1], n - 1)):     # behind canonical ones, a workgroup boundary
        row = list(good)
        for i, p in enumerate(places):
            row[p] = bad_ff if i % 2 else NOT_CANONICAL
        rc, nn, bad, nodes = _raw(ctx, start, frontier, row, need)
        assert rc == 1 and bad == first, (places, rc, bad)
        assert (nodes == 0x5A).all()
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.merkle_tree_append(start, arr(frontier), arr(row))
        assert e.value.code == 1 and e.value.bad_index == first
        with pytest.raises(ValueError) as e2:
            H.merkle_tree_append(start, arr(frontier), arr(row))
        assert e2.value.bad_index == first
    for h in (0, 1, 2):                          # a used frontier entry
        fr = list(frontier)
        fr[h] = NOT_CANONICAL
        fr[2] = NOT_CANONICAL if h < 2 else fr[2]
        rc, nn, bad, nodes = _raw(ctx, start, fr, good, need)
        assert rc == 1 and bad == -2 - h and (nodes == 0x5A).all()
        with pytest.raises(ValueError) as e2:
            H.merkle_tree_append(start, arr(fr), arr(good))
        assert e2.value.bad_index == -2 - h
    # an entry that is not used is not looked at (every unused one of `frontier` is 0xff..ff), and the context goes on
    rc, nn, bad, nodes = _raw(ctx, start, frontier, good, need)
    assert rc == 0 and nn == need and bad == -1 and (nodes[:need] == want).all()
    # beyond the tree
    rc, nn, bad, nodes = _raw(ctx, FULL - 4, host_block(FULL - 4, 4)[0], good[:5], 64)
    assert rc == 1 and bad == -1 and (nodes == 0x5A).all()


def test_capacity(ctx):
    start, n = (1 << 20) + 3, 37
    frontier, row, want = host_block(start, n)
    need = want.shape[0]
    rc, nn, bad, nodes = _raw(ctx, start, frontier, row, need - 1)
    assert rc == 10 and nn == need and bad == -1           # MASP_HIP_E_CAPACITY
    assert (nodes == 0x5A).all()
    rc, nn, bad, nodes = _raw(ctx, start, frontier, row, nn)
    assert rc == 0 and (nodes[:need] == want).all()
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.merkle_tree_append(start, arr(frontier), arr(row), nodes_capacity=3)
    assert e.value.code == 10 and e.value.needed == need
    up, kernels, down = ctx.merkle_last_timing()           # the last call of either kind
    assert up > 0 and kernels > 0 and down > 0


def _run(leaves, ctx):
    tree = CommitmentTree.empty()
    ws = advance(tree, [], leaves[:37], track=(0, 35, 36), ctx=ctx)
    states = [[tree.write()] + [w.write() for w in ws]]
    ws += advance(tree, ws, leaves[37:337], track=(0, 1, 298, 299), ctx=ctx)
    states.append([tree.write()] + [w.write() for w in ws])
    ws += advance(tree, ws, leaves[337:], ctx=ctx)
    states.append([tree.write()] + [w.write() for w in ws])
    return tree, ws, states


def test_advance_end_to_end(ctx):
    leaves = R.random_nodes(338, 8200)
    tree, ws, states = _run(leaves, ctx)
    host_tree, host_ws, host_states = _run(leaves, None)
    assert states == host_states
    positions = [w.position() for w in ws]
    assert positions == [0, 35, 36, 37, 38, 335, 336] and tree.size() == 338
    root, paths = FrozenCommitmentTree.paths(leaves, positions, ctx)
    assert tree.root() == root
    for w, path in zip(ws, paths):
        assert w.path() == path
        assert w.path().root(leaves[w.position()]) == tree.root()
    # a node that is not canonical: refused with its index in the block, nothing changed
    before = [tree.write()] + [w.write() for w in ws]
    block = R.random_nodes(5, 8201)
    block[3] = NOT_CANONICAL
    with pytest.raises(ValueError) as e:
        advance(tree, ws, block, track=(0,), ctx=ctx)
    assert e.value.bad_index == 3 and [tree.write()] + [w.write() for w in ws] == before


def test_frozen_and_append_calls_alternate_on_one_context(ctx):
    start, n = (1 << 20) + 3, 2 * T + 2
    frontier, row, want = host_block(start, n)
    leaves = R.random_nodes(2 * B + 2, 8300)
    pos = [0, 2 * B + 1]
    frozen = ctx.merkle_tree_complete(arr(leaves), 0, pos)
    block = ctx.merkle_tree_append(start, arr(frontier), arr(row))
    for _ in range(2):                           # they share the table, the stream and the scratch
        f = ctx.merkle_tree_complete(arr(leaves), 0, pos)
        b = ctx.merkle_tree_append(start, arr(frontier), arr(row))
        assert (f[0] == frozen[0]).all() and f[1] == frozen[1] and (f[2] == frozen[2]).all()
        assert (b == block).all()
    assert (block == want).all()
    host = H.merkle_tree_complete(arr(leaves), 0, pos)
    assert (frozen[0] == host[0]).all() and frozen[1] == host[1] and (frozen[2] == host[2]).all()
