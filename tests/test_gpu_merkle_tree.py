"""Frozen commitment trees on the GPU (masp_hip_merkle_tree_complete, k_merkle.hip) through the C ABI, against the host path
(masp_host_merkle_tree_complete) over the same rows and, for the small rows, against the plain-Python transcription of the reference
(tests/merkle_ref.py).  Every comparison is of bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import compact_notes as CN
import masp_amd
import merkle_ref as R
from masp_amd import FrozenCommitmentTree
from masp_amd import host as H
from masp_amd.merkle_tree import MT_BLOCK, MT_TOP_PARENTS     # k_mt_level's workgroup size B and the hand-over to k_mt_top, as k_merkle.hip
                                                              # defines them (tests/test_merkle_tree_host.py compares them with the source)

pytestmark = pytest.mark.gpu

Q = R.Q
B = MT_BLOCK
WIDTHS = [0, 1, 2, 3,                                  # the degenerate top
          5, 37,                                       # odd rows at several levels
          2 * B, 2 * B + 2,                            # a parent row that exactly fills, and just overflows, one workgroup of k_mt_level
          2 * MT_TOP_PARENTS, 2 * MT_TOP_PARENTS + 2,  # the widest row k_mt_top takes whole, and the narrowest that needs one k_mt_level first
          4097]                                        # odd rows at many levels


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def arr(nodes):
    return np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 32) if nodes else np.zeros((0, 32), np.uint8)


def sample_positions(n, seed):
    if n == 0:
        return []
    last_even = (n - 1) & ~1                 # the last position that is a left child (its sibling may be the row's padding)
    return sorted({0, n - 1, last_even} | set(random.Random(seed).sample(range(n), min(n, 5))))


_host = {}


def host_tree(n, height0=0, seed=None):
    key = (n, height0, seed)
    if key not in _host:
        row = R.random_nodes(n, 2000 + n if seed is None else seed)
        pos = sample_positions(n, n)
        _host[key] = (row, pos) + H.merkle_tree_complete(arr(row), height0, pos)
    return _host[key]


@pytest.mark.parametrize("n", WIDTHS)
def test_row_widths(ctx, n):
    row, pos, want_nodes, want_root, want_paths = host_tree(n)
    nodes, root, paths = ctx.merkle_tree_complete(arr(row), 0, pos)
    assert nodes.shape == want_nodes.shape == (H.merkle_node_count(n), 32)
    assert (nodes == want_nodes).all()
    assert root == want_root
    assert paths.shape == (len(pos), 32, 32) and (paths == want_paths).all()
    if n <= 37:                              # not only against new host code
        ref = R.new(row)
        assert R.as_list(nodes) == ref and root == R.root(ref)
        for k, p in enumerate(pos):
            assert [bytes(s) for s in paths[k]] == [x for x, _ in R.path(ref, n, p)]


@pytest.mark.parametrize("height0,n", [(3, 37), (3, 2 * MT_TOP_PARENTS + 5), (31, 1), (31, 2), (32, 1), (32, 0)])
def test_rows_above_the_leaves(ctx, height0, n):
    row, pos, want_nodes, want_root, want_paths = host_tree(n, height0, seed=2100 + height0)
    nodes, root, paths = ctx.merkle_tree_complete(arr(row), height0, pos)
    assert (nodes == want_nodes).all() and nodes.shape == want_nodes.shape
    assert root == want_root
    assert paths.shape == (len(pos), 32 - height0, 32) and (paths == want_paths).all()
    if n <= 37:
        assert R.as_list(nodes) == R.complete(row, 0, n, height0)


def test_without_the_node_vector(ctx):
    row, pos, want_nodes, want_root, want_paths = host_tree(2 * B + 2)
    nodes, root, paths = ctx.merkle_tree_complete(arr(row), 0, pos, want_nodes=False)
    assert nodes is None and root == want_root and (paths == want_paths).all()
    root2, only = FrozenCommitmentTree.paths(row, pos, ctx)
    assert root2 == want_root
    for k, p in enumerate(pos):
        assert only[k].position == p and only[k].siblings == [bytes(s) for s in want_paths[k]]
    assert only[-1].root(row[pos[-1]]) == want_root


def test_edge_leaves(ctx):
    edge = [(0).to_bytes(32, "little"), (1).to_bytes(32, "little"), (Q - 1).to_bytes(32, "little"), ((1 << 254) + 12345).to_bytes(32, "little"),
            ((1 << 254) - 1).to_bytes(32, "little")]
    assert (Q - 1) >> 254 == 1
    row = edge + edge[::-1] + [edge[2]] * 3
    ref = R.new(row)
    nodes, root, paths = ctx.merkle_tree_complete(arr(row), 0, range(len(row)))
    assert R.as_list(nodes) == ref and root == ref[-1]
    for p in range(len(row)):
        assert [bytes(s) for s in paths[p]] == [x for x, _ in R.path(ref, len(row), p)]


def _raw(ctx, row, capacity, positions, marker=0x5A):
    """the C call with buffers pre-filled with a marker byte -> (rc, n_nodes, bad_index, nodes, root, paths)"""
    row = arr(row)
    n = row.shape[0]
    nodes = np.full((max(capacity, 1), 32), marker, np.uint8)
    root = np.full(32, marker, np.uint8)
    pos = np.asarray(positions, np.uint64)
    paths = np.full((max(len(positions), 1), 32, 32), marker, np.uint8)
    nn, bad = C.c_size_t(12345), C.c_int64(777)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.masp_hip_merkle_tree_complete(ctx._h, 0, n, vp(row) if n else None, vp(nodes), capacity, C.byref(nn), vp(root), len(positions),
                                              vp(pos) if len(positions) else None, vp(paths), C.byref(bad))
    return rc, nn.value, bad.value, nodes, root, paths


def test_nodes_that_are_not_canonical(ctx):
    n = 2 * B + 37
    good = R.random_nodes(n, 2200)
    need = H.merkle_node_count(n)
    bad_q, bad_ff = Q.to_bytes(32, "little"), b"\xff" * 32
    for places, first in (([0], 0), ([B - 1, B, n - 1], B - 1), ([B, 300], B), ([n - 1], n - 1)):     # first lane, a workgroup boundary, the last index
        row = list(good)
        for i, p in enumerate(places):
            row[p] = bad_ff if i % 2 else bad_q
        rc, nn, bad, nodes, root, paths = _raw(ctx, row, need, [0, n - 1])
        assert rc == 1 and bad == first, (places, rc, bad)
        assert (nodes == 0x5A).all() and (root == 0x5A).all() and (paths == 0x5A).all()
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.merkle_tree_complete(arr(row))
        assert e.value.code == 1 and e.value.bad_index == first
        with pytest.raises(ValueError) as e2:
            FrozenCommitmentTree(row, ctx)
        assert e2.value.bad_index == first
    # ... and the context goes on
    want = H.merkle_tree_complete(arr(good), 0, [0, n - 1])
    rc, nn, bad, nodes, root, paths = _raw(ctx, good, need, [0, n - 1])
    assert rc == 0 and nn == need and bad == -1
    assert (nodes[:need] == want[0]).all() and bytes(root) == want[1] and (paths[:2] == want[2]).all()


def test_capacity_and_positions(ctx):
    row, pos, want_nodes, want_root, want_paths = host_tree(37)
    need = want_nodes.shape[0]
    rc, nn, bad, nodes, root, paths = _raw(ctx, row, need - 1, [36])
    assert rc == 10 and nn == need and bad == -1           # MASP_HIP_E_CAPACITY
    assert (nodes == 0x5A).all() and (root == 0x5A).all() and (paths == 0x5A).all()
    rc, nn, bad, nodes, root, paths = _raw(ctx, row, nn, [36])
    assert rc == 0 and (nodes[:need] == want_nodes).all() and bytes(root) == want_root
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.merkle_tree_complete(arr(row), nodes_capacity=3)
    assert e.value.code == 10 and e.value.needed == need
    for positions in ([37], [0, 1 << 40]):
        rc, nn, bad, nodes, root, paths = _raw(ctx, row, need, positions)
        assert rc == 1 and bad == -1
        assert (nodes == 0x5A).all() and (root == 0x5A).all() and (paths == 0x5A).all()


def test_two_calls_give_the_same_bytes(ctx):
    row, pos, want_nodes, want_root, want_paths = host_tree(2 * MT_TOP_PARENTS + 2)
    a = ctx.merkle_tree_complete(arr(row), 0, pos)
    b = ctx.merkle_tree_complete(arr(row), 0, pos)
    assert (a[0] == b[0]).all() and a[1] == b[1] and (a[2] == b[2]).all()
    assert (a[0] == want_nodes).all()
    up, kernels, down = ctx.merkle_last_timing()
    assert up > 0 and kernels > 0 and down > 0


def _compact_vectors(c):
    ivks = [tv["ivk"] for tv in CN.VECTORS]
    epks, cmus, encs = CN.rows_to_arrays([(tv["epk"], tv["cmu"], tv["c_enc"]) for tv in CN.VECTORS])
    status, ho, hi, hp, hk, cand = c.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 1)
    assert status.tolist() == [0] * 10
    assert ho.tolist() == list(range(10)) and hi.tolist() == list(range(10))
    assert [p.tobytes() for p in hp] == [tv["p_enc"][:84] for tv in CN.VECTORS]
    assert [p.tobytes() for p in hk] == [tv["default_pk_d"] for tv in CN.VECTORS]


def _tree_of_37(c):
    row, pos, want_nodes, want_root, want_paths = host_tree(37)
    nodes, root, paths = c.merkle_tree_complete(arr(row), 0, pos)
    assert (nodes == want_nodes).all() and root == want_root and (paths == want_paths).all()


def test_the_tree_and_the_compact_scan_share_the_table():
    """each uploads the table if the other has not: a fresh context per order"""
    for first, second in ((_tree_of_37, _compact_vectors), (_compact_vectors, _tree_of_37)):
        c = masp_amd.Context(0)
        try:
            first(c)
            second(c)
            first(c)
        finally:
            c.close()


def test_merge_on_the_gpu(ctx):
    leaves = R.random_nodes(64 + 64 + 5, 2300)
    parts = [leaves[:64], leaves[64:128], leaves[128:]]
    want = FrozenCommitmentTree.merge([FrozenCommitmentTree(p) for p in parts])
    got = FrozenCommitmentTree.merge([FrozenCommitmentTree(p, ctx) for p in parts], ctx)
    assert got.size() == want.size() == 133
    assert (got.nodes == want.nodes).all() and got.root() == want.root()
    whole = FrozenCommitmentTree(leaves, ctx)
    assert whole.root() == got.root()
    for p in (0, 63, 64, 127, 128, 132):
        assert got.path(p) == whole.path(p) and got.path(p).root(leaves[p]) == got.root()
