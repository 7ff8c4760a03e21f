"""masp_host_merkle_tree_complete and the ctx=None path of masp_amd.merkle_tree against the plain-Python transcription of the reference's
FrozenCommitmentTree (tests/merkle_ref.py, built on host.merkle_hash alone).  Every comparison is of bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merkle_ref as R
from masp_amd import FrozenCommitmentTree, MerklePath, empty_root
from masp_amd import host as H
from masp_amd import merkle_tree as MT

Q = R.Q
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 37)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arr(nodes):
    return np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 32) if nodes else np.zeros((0, 32), np.uint8)


def test_empty_roots():
    got = H.merkle_empty_roots()
    assert got.shape == (33, 32)
    assert [bytes(r) for r in got] == [R.empty_root(h) for h in range(33)]
    assert empty_root(0) == (1).to_bytes(32, "little") and empty_root(32) == R.empty_root(32)
    assert empty_root(0) == H.AllowedConversion.uncommitted().to_bytes(32, "little")


def test_the_kernel_geometry_the_module_states_is_the_source_s():
    src = open(os.path.join(ROOT, "masp_amd", "csrc", "k_merkle.hip")).read()
    assert int(re.search(r"constexpr uint32_t MT_BLOCK = (\d+);", src).group(1)) == MT.MT_BLOCK
    assert int(re.search(r"constexpr uint32_t MT_TOP_PARENTS = (\d+);", src).group(1)) == MT.MT_TOP_PARENTS


@pytest.mark.parametrize("n", SIZES)
def test_new_against_the_transcription(n):
    leaves = R.random_nodes(n, 1300 + n)
    want = R.new(leaves)
    nodes, root, paths = H.merkle_tree_complete(arr(leaves), 0, list(range(n)), threads=3)
    assert R.as_list(nodes) == want and nodes.shape[0] == H.merkle_node_count(n)
    assert root == R.root(want)
    assert paths.shape == (n, 32, 32)
    for p in range(n):
        assert [bytes(s) for s in paths[p]] == [node for node, _ in R.path(want, n, p)]
    t = FrozenCommitmentTree(leaves)
    assert t.size() == n and t.root() == R.root(want) and R.as_list(t.nodes) == want
    if n:
        assert t.path(n - 1).auth_path == R.path(want, n, n - 1) and t.path(0).auth_path == R.path(want, n, 0)
    if n == 0:
        assert t.nodes.shape == (0, 32) and t.root() == empty_root(32)


@pytest.mark.parametrize("height0,sizes", [(3, SIZES), (31, (0, 1, 2)), (32, (0, 1))])
def test_rows_above_the_leaves(height0, sizes):
    for n in sizes:
        row = R.random_nodes(n, 1400 + 40 * height0 + n)
        want = R.complete(row, 0, n, height0)
        nodes, root, paths = H.merkle_tree_complete(arr(row), height0, list(range(n)))
        assert R.as_list(nodes) == want, (height0, n)
        assert root == (want[-1] if want else R.empty_root(32))
        assert paths.shape == (n, 32 - height0, 32)
        for p in range(n):
            assert [bytes(s) for s in paths[p]] == [node for node, _ in R.path(want, n, p, height0)]
    if height0 >= 31:      # one node more than a row of that level can hold
        with pytest.raises(ValueError):
            H.merkle_tree_complete(arr(R.random_nodes((1 << (32 - height0)) + 1, 5)), height0)
    with pytest.raises(ValueError):
        H.merkle_tree_complete(arr([]), 33)


def test_every_path_of_37_leaves():
    n = 37
    leaves = R.random_nodes(n, 1337)
    want = R.new(leaves)
    t = FrozenCommitmentTree(leaves)
    root, only = FrozenCommitmentTree.paths(leaves, range(n))
    assert root == t.root() == R.root(want)
    for p in range(n):
        path = t.path(p)
        assert isinstance(path, MerklePath) and path.position == p
        assert path.auth_path == R.path(want, n, p)
        assert [r for _, r in path.auth_path] == [bool(p >> i & 1) for i in range(32)]
        assert path.root(leaves[p]) == root
        assert only[p] == path
        siblings, position = path                      # the form prover.spend_proof / convert_proof take
        assert H.merkle_root(leaves[p], siblings, position) == root
    # the last node of an odd row has that level's empty root beside it: the rows are 37, 19, 10, 5, 3, 2, 1 wide, so the last leaf's
    # ancestor is alone at levels 0, 1, 3, 4 and from 6 up
    last = t.path(n - 1).auth_path
    widths = [37, 19, 10, 5, 3, 2, 1]
    for level, w in enumerate(widths):
        if w % 2 == 1:
            assert last[level] == (empty_root(level), False), level
        else:
            assert last[level][1] is True and last[level][0] != empty_root(level)
    for level in range(7, 32):
        assert last[level] == (empty_root(level), False)
    with pytest.raises(ValueError):
        t.path(n)
    with pytest.raises(ValueError):
        t.path(-1)
    with pytest.raises(ValueError):
        FrozenCommitmentTree.paths(leaves, [n])


@pytest.mark.parametrize("sizes", [(4, 4, 3), (4, 4, 4), (8, 1), (5,)])
def test_merge(sizes):
    leaves = R.random_nodes(sum(sizes), 1500 + sum(sizes) + len(sizes))
    parts, at = [], 0
    for s in sizes:
        parts.append(leaves[at:at + s])
        at += s
    want, want_size = R.merge([(R.new(p), len(p)) for p in parts])
    got = FrozenCommitmentTree.merge([FrozenCommitmentTree(p) for p in parts])
    assert got.size() == want_size == len(leaves)
    assert R.as_list(got.nodes) == want
    whole = FrozenCommitmentTree(leaves)
    assert got.root() == whole.root() == R.root(R.new(leaves))
    for p in range(len(leaves)):
        assert got.path(p) == whole.path(p)
        assert got.path(p).root(leaves[p]) == whole.root()


def test_merge_of_nothing_and_its_asserts():
    e = FrozenCommitmentTree.merge([])
    assert e.size() == 0 and e.nodes.shape == (0, 32) and e.root() == empty_root(32)
    T = lambda n, seed: FrozenCommitmentTree(R.random_nodes(n, seed))
    with pytest.raises(AssertionError):
        FrozenCommitmentTree.merge([T(3, 1), T(2, 2)])            # not a power of two
    with pytest.raises(AssertionError):
        FrozenCommitmentTree.merge([T(4, 1), T(2, 2), T(1, 3)])   # the full subtrees differ
    with pytest.raises(AssertionError):
        FrozenCommitmentTree.merge([T(2, 1), T(4, 2)])            # the last is larger


def _raw(height0, row, capacity, positions, with_nodes=True, marker=0xA5):
    """the C call with buffers pre-filled with a marker byte -> (rc, n_nodes, bad_index, nodes, root, paths)"""
    L = H.load_library()
    row = arr(row)
    n, depth = row.shape[0], 32 - height0
    nodes = np.full((max(capacity, 1), 32), marker, np.uint8)
    root = np.full(32, marker, np.uint8)
    pos = np.asarray(positions, np.uint64)
    paths = np.full((max(len(positions), 1), max(depth, 1), 32), marker, np.uint8)
    nn, bad = C.c_size_t(12345), C.c_int64(777)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.masp_host_merkle_tree_complete(height0, n, vp(row) if n else None, vp(nodes) if with_nodes else None, capacity, C.byref(nn), vp(root),
                                          len(positions), vp(pos) if len(positions) else None, vp(paths), C.byref(bad), 2)
    return rc, nn.value, bad.value, nodes, root, paths


@pytest.mark.parametrize("where", [0, 18, 36])
def test_a_node_that_is_not_canonical(where):
    leaves = R.random_nodes(37, 1600)
    leaves[where] = Q.to_bytes(32, "little")
    if where == 18:
        leaves[30] = ((1 << 256) - 1).to_bytes(32, "little")      # a later one too: the smallest index is reported
    rc, nn, bad, nodes, root, paths = _raw(0, leaves, 200, [0, 36])
    assert rc == 1 and bad == where
    assert (nodes == 0xA5).all() and (root == 0xA5).all() and (paths == 0xA5).all()
    with pytest.raises(ValueError) as e:
        FrozenCommitmentTree(leaves)
    assert e.value.bad_index == where


def test_capacity_protocol_and_positions():
    leaves = R.random_nodes(9, 1700)
    want = R.new(leaves)
    need = len(want)
    rc, nn, bad, nodes, root, paths = _raw(0, leaves, need - 1, [8])
    assert rc == H.E_CAPACITY == 6 and nn == need and bad == -1
    assert (nodes == 0xA5).all() and (root == 0xA5).all() and (paths == 0xA5).all()
    rc, nn, bad, nodes, root, paths = _raw(0, leaves, nn, [8])
    assert rc == 0 and nn == need and bad == -1
    assert R.as_list(nodes[:need]) == want and bytes(root) == want[-1]
    assert [bytes(s) for s in paths[0]] == [x for x, _ in R.path(want, 9, 8)]
    # no node vector wanted: the same root and path, whatever the capacity says
    rc, nn, bad, nodes, root2, paths2 = _raw(0, leaves, 0, [8], with_nodes=False)
    assert rc == 0 and nn == need and (nodes == 0xA5).all() and (root2 == root).all() and (paths2 == paths).all()
    # a position beyond the row is refused, and nothing is written
    for positions in ([9], [0, 1 << 40], [8, 9]):
        rc, nn, bad, nodes, root, paths = _raw(0, leaves, need, positions)
        assert rc == 1 and bad == -1
        assert (nodes == 0xA5).all() and (root == 0xA5).all() and (paths == 0xA5).all()
    rc, nn, bad, nodes, root, paths = _raw(0, [], 0, [0])
    assert rc == 1
    # n = 0: an empty vector and empty_root(32)
    rc, nn, bad, nodes, root, paths = _raw(0, [], 0, [])
    assert rc == 0 and nn == 0 and bytes(root) == R.empty_root(32) and (nodes == 0xA5).all()
    # more nodes than a row of that level can have
    assert _raw(31, R.random_nodes(3, 1), 100, [])[0] == 1
    assert _raw(32, R.random_nodes(2, 1), 100, [])[0] == 1


def test_threads_do_not_change_the_bytes():
    leaves = R.random_nodes(300, 1800)          # rows of 150 and 75 parents are dealt to the threads, the narrower ones are not
    a = H.merkle_tree_complete(arr(leaves), 0, [0, 299, 150], threads=1)
    b = H.merkle_tree_complete(arr(leaves), 0, [0, 299, 150], threads=7)
    assert (a[0] == b[0]).all() and a[1] == b[1] and (a[2] == b[2]).all()
    for k, p in enumerate((0, 299, 150)):
        assert MerklePath([(bytes(s), bool(p >> i & 1)) for i, s in enumerate(a[2][k])], p).root(leaves[p]) == a[1]
