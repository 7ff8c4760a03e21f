"""CommitmentTree, IncrementalWitness and advance(ctx=None) of masp_amd.merkle_tree, and masp_host_merkle_tree_append under them: against
the reference's own vectors (tests/golden/merkle_tree_vectors.json, the data of its test_sapling_tree) and against the plain-Python
transcription of its one-by-one append (tests/incremental_ref.py, built on host.merkle_hash alone).  Every comparison is of bytes."""
import json
import os
import random

import numpy as np
import pytest

import incremental_ref as IR
import merkle_ref as R
from masp_amd import CommitmentTree, FrozenCommitmentTree, IncrementalWitness, advance, empty_root
from masp_amd import host as H
from masp_amd.merkle_tree import MT_BLOCK, MT_TOP_PARENTS

Q = R.Q
HERE = os.path.dirname(os.path.abspath(__file__))
V = json.load(open(os.path.join(HERE, "golden", "merkle_tree_vectors.json")))
CMUS = [bytes.fromhex(x) for x in V["commitments"]]
D = V["depth"]
NOT_CANONICAL = Q.to_bytes(32, "little")


def arr(nodes):
    return np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 32) if nodes else np.zeros((0, 32), np.uint8)


def witness_vector(round_, j):
    """witness_ser of witness j (made from the tree of j leaves) after round `round_`'s append: the vectors run round by round"""
    assert j <= round_
    return bytes.fromhex(V["witness_ser"][round_ * (round_ + 1) // 2 + j])


def test_the_fixture_is_the_reference_s_data():
    assert [len(V[k]) for k in ("commitments", "roots", "tree_ser", "paths", "witness_ser")] == [16, 16, 16, 120, 136] and D == 4


def test_one_by_one_append_replays_the_reference_s_vectors():
    tree = CommitmentTree.empty()
    assert tree.size() == 0 and tree.root() == empty_root(32) and tree.write() == b"\x00\x00\x00"
    with pytest.raises(ValueError):
        IncrementalWitness.from_tree(tree)          # the documented difference: the reference's first witness can never form a path
    witnesses, last, paths_i, ser_i, compared = [], None, 0, 0, 0
    for i, cmu in enumerate(CMUS):
        witnesses.append((IncrementalWitness.from_tree(tree) if i else None, last))
        tree.append(cmu, depth=D)
        assert tree.size() == i + 1
        assert tree.root(depth=D).hex() == V["roots"][i]
        assert tree.write().hex() == V["tree_ser"][i]
        assert CommitmentTree.read(bytes.fromhex(V["tree_ser"][i])).write().hex() == V["tree_ser"][i]
        assert CommitmentTree.read(tree.write()) == tree
        for w, leaf in witnesses:
            if w is None:                           # the vectors of the witness made from the empty tree are left out
                ser_i += 1
                continue
            w.append(cmu, depth=D)
            path = w.path(depth=D)
            assert IR.path_ser(path.auth_path, path.position).hex() == V["paths"][paths_i]
            assert path.root(leaf) == w.root(depth=D)
            paths_i += 1
            assert w.write().hex() == V["witness_ser"][ser_i]
            assert IncrementalWitness.read(bytes.fromhex(V["witness_ser"][ser_i])).write().hex() == V["witness_ser"][ser_i]
            assert IncrementalWitness.read(w.write()) == w
            ser_i += 1
            compared += 1
            assert w.root(depth=D) == tree.root(depth=D)
        last = cmu
    assert (compared, paths_i, ser_i) == (120, 120, 136)
    before = tree.write()
    with pytest.raises(ValueError):
        tree.append(empty_root(0), depth=D)         # the 17th
    assert tree.write() == before
    for w, _ in witnesses[1:]:
        with pytest.raises(ValueError):
            w.append(empty_root(0), depth=D)


SPLITS = [[c, 16 - c] for c in range(1, 16)] + [[b] * (16 // b) + ([16 % b] if 16 % b else []) for b in (1, 2, 3, 5, 16)]


@pytest.mark.parametrize("blocks", SPLITS, ids=lambda b: "x".join(map(str, b)) if len(b) < 4 else "%dx%d" % (len(b), b[0]))
def test_advance_replays_the_reference_s_vectors(blocks):
    assert sum(blocks) == 16
    tree, witnesses, at, compared = CommitmentTree.empty(), {}, 0, 0
    for size in blocks:
        old = sorted(witnesses)
        made = advance(tree, [witnesses[j] for j in old], CMUS[at:at + size], track=range(size))
        for k, w in enumerate(made):                # tracked leaf at + k is witness at + k + 1 of the reference's loop
            witnesses[at + k + 1] = w
        at += size
        assert tree.size() == at and tree.write().hex() == V["tree_ser"][at - 1] and tree.root(depth=D).hex() == V["roots"][at - 1]
        for j, w in witnesses.items():
            assert w.position() == j - 1
            if j <= at - 1:
                assert w.write() == witness_vector(at - 1, j)
                compared += 1
            else:                                   # made behind the block's last leaf: the reference serialises it a round later
                assert j == at and w.write() == IncrementalWitness.from_tree(tree).write()
            assert w.root(depth=D) == tree.root(depth=D)
    assert compared == sum(sum(blocks[:i + 1]) - 1 for i in range(len(blocks)))
    assert [witnesses[j].write() for j in range(1, 16)] == [witness_vector(15, j) for j in range(1, 16)]


_grown = {}


def grown(size):
    """the transcription's tree of `size` random leaves and its witnesses at the first, a middle and the last position; never modified"""
    if size not in _grown:
        leaves = R.random_nodes(size, 7100 + size)
        tree, ws = IR.Tree(), {}
        for i, leaf in enumerate(leaves):
            tree.append(leaf)
            for w in ws.values():
                w.append(leaf)
            if i in (0, size // 2, size - 1):
                ws[i] = IR.Witness(tree)
        _grown[size] = (leaves, tree.write(), {p: w.write() for p, w in ws.items()})
    return _grown[size]


@pytest.mark.parametrize("block", (1, 2, 3, 64, 129))
@pytest.mark.parametrize("size", (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65))
def test_advance_against_the_transcription(size, block):
    leaves, tree_ser, wit_ser = grown(size)
    nodes = R.random_nodes(block, 7300 + 131 * size + block)
    track = sorted({0, block // 2, block - 1})
    # the product's state comes from the transcription's bytes, not from the product's own append
    tree = CommitmentTree.read(tree_ser)
    ws = [IncrementalWitness.read(wit_ser[p]) for p in sorted(wit_ser)]
    ref_tree, ref_ws, ref_made = IR.Tree.read(tree_ser), [IR.Witness.read(wit_ser[p]) for p in sorted(wit_ser)], []
    for k, node in enumerate(nodes):
        assert ref_tree.append(node)
        for w in ref_ws + ref_made:
            assert w.append(node)
        if k in track:
            ref_made.append(IR.Witness(ref_tree))
    made = advance(tree, ws, nodes, track)
    assert tree.size() == size + block and tree.write() == ref_tree.write() and tree.root() == ref_tree.root()
    assert [w.write() for w in ws] == [w.write() for w in ref_ws]
    assert [w.write() for w in made] == [w.write() for w in ref_made]
    assert [w.position() for w in made] == [size + k for k in track]
    for w, r in zip(ws + made, ref_ws + ref_made):
        auth, position = r.path()
        path = w.path()
        assert (path.auth_path, path.position) == (auth, position)
        assert w.root() == tree.root()
        assert IncrementalWitness.read(w.write()) == w
        if w.cursor is not None:
            assert w.cursor_depth == r.cursor_depth


def test_extend_is_advance_without_witnesses():
    nodes = R.random_nodes(70, 7001)
    a, b = CommitmentTree.empty(), IR.Tree()
    a.extend(nodes[:33])
    a.extend([])
    a.extend(arr(nodes[33:]))
    for x in nodes:
        b.append(x)
    assert a.write() == b.write()


def fabricated(seed):
    """the serialisation of a tree of 2^32 - 4 leaves: a full pair and every parent but the one of 4 leaves, all random"""
    rng = random.Random(seed)
    node = lambda: rng.randrange(Q).to_bytes(32, "little")
    ser = b"\x01" + node() + b"\x01" + node() + bytes([31]) + b"".join(b"\x00" if k == 1 else b"\x01" + node() for k in range(31))
    assert IR.Tree.read(ser).size() == (1 << 32) - 4
    return ser


def test_the_last_four_leaves_of_the_depth_32_tree():
    ser = fabricated(7400)
    tree = CommitmentTree.read(ser)
    assert tree.size() == (1 << 32) - 4 and tree.write() == ser
    w = IncrementalWitness.from_tree(tree)
    ref_tree = IR.Tree.read(ser)
    ref_w = IR.Witness(ref_tree)
    nodes = R.random_nodes(5, 7401)
    # one too many: refused, nothing changed
    with pytest.raises(ValueError):
        advance(tree, [w], nodes, track=(0,))
    assert tree.write() == ser and w.write() == ref_w.write()
    for node in nodes[:4]:
        assert ref_tree.append(node) and ref_w.append(node)
    made = advance(tree, [w], nodes[:4], track=(3,))
    assert tree.size() == 1 << 32 and tree.write() == ref_tree.write() and w.write() == ref_w.write()
    assert made[0].write() == IR.Witness(ref_tree).write() and made[0].position() == (1 << 32) - 1
    assert w.root() == tree.root() == ref_tree.root() == made[0].root()
    assert not ref_tree.append(nodes[4]) and not ref_w.append(nodes[4])         # full, as the reference has it
    full = tree.write()
    with pytest.raises(ValueError):
        advance(tree, [w], nodes[4:])
    with pytest.raises(ValueError):
        tree.append(nodes[4])
    with pytest.raises(ValueError):
        w.append(nodes[4])
    assert tree.write() == full and w.write() == ref_w.write()
    # the native call there: the block's nodes reach level 32, the last of them the root
    frontier = arr([empty_root(0)] + [p or empty_root(0) for p in IR.Tree.read(ser).parents])
    pair = [IR.Tree.read(ser).left, IR.Tree.read(ser).right]
    got = H.merkle_tree_append((1 << 32) - 6, frontier, arr(pair + nodes[:4]))
    assert got.shape[0] == H.merkle_append_node_count((1 << 32) - 6, 6) and bytes(got[-1]) == tree.root()
    assert R.as_list(got) == IR.block_nodes((1 << 32) - 6, R.as_list(frontier), pair + nodes[:4])


@pytest.mark.parametrize("size", (0, 1, 2, 5, 8))
def test_a_node_that_is_not_canonical_changes_nothing(size):
    _, tree_ser, wit_ser = grown(size)
    tree = CommitmentTree.read(tree_ser)
    ws = [IncrementalWitness.read(wit_ser[p]) for p in sorted(wit_ser)]
    nodes = R.random_nodes(9, 7500 + size)
    nodes[6] = NOT_CANONICAL
    nodes[8] = NOT_CANONICAL
    with pytest.raises(ValueError) as e:
        advance(tree, ws, nodes, track=(0, 7))
    assert e.value.bad_index == 6
    assert tree.write() == tree_ser and [w.write() for w in ws] == [wit_ser[p] for p in sorted(wit_ser)]
    with pytest.raises(ValueError):
        tree.append(NOT_CANONICAL)
    assert tree.write() == tree_ser


def test_witnesses_of_another_tree_are_refused():
    _, tree_ser, wit_ser = grown(7)
    _, other_ser, _ = grown(8)
    tree = CommitmentTree.read(other_ser)
    ws = [IncrementalWitness.read(wit_ser[p]) for p in sorted(wit_ser)]
    with pytest.raises(ValueError):
        advance(tree, ws, R.random_nodes(3, 7600))
    assert tree.write() == other_ser and [w.write() for w in ws] == [wit_ser[p] for p in sorted(wit_ser)]
    with pytest.raises(ValueError):
        advance(tree, [], R.random_nodes(3, 7600), track=(3,))
    assert tree.write() == other_ser


def test_read_refuses_what_is_no_tree():
    ok = CommitmentTree.read(bytes.fromhex(V["tree_ser"][6]))
    assert ok.size() == 7
    with pytest.raises(ValueError):
        CommitmentTree.read(b"\x01" + CMUS[0] + b"\x00" + bytes([33]) + b"\x00" * 33)        # 33 parents
    assert CommitmentTree.read(b"\x01" + CMUS[0] + b"\x00" + bytes([32]) + b"\x00" * 32).size() == 1
    with pytest.raises(ValueError):
        CommitmentTree.read(b"\x01" + NOT_CANONICAL + b"\x00\x00")
    with pytest.raises(ValueError):
        CommitmentTree.read(b"\x01" + CMUS[0] + b"\x00\x01\x01" + NOT_CANONICAL)
    with pytest.raises(ValueError):
        CommitmentTree.read(bytes.fromhex(V["tree_ser"][6])[:-1])
    with pytest.raises(ValueError):
        IncrementalWitness.read(b"\x00\x00\x00" + b"\x00\x00")                                # the witness of the empty tree
    with pytest.raises(ValueError):
        IncrementalWitness.read(bytes.fromhex(V["tree_ser"][6]) + b"\x01" + NOT_CANONICAL + b"\x00")


def test_paths_agree_with_the_frozen_tree():
    leaves = R.random_nodes(338, 7700)
    tree = CommitmentTree.empty()
    ws = advance(tree, [], leaves[:37], track=(0, 35, 36))
    ws += advance(tree, ws, leaves[37:337], track=(0, 1, 298, 299))
    ws += advance(tree, ws, leaves[337:], track=(0,))
    positions = [w.position() for w in ws]
    assert positions == [0, 35, 36, 37, 38, 335, 336, 337]
    root, paths = FrozenCommitmentTree.paths(leaves, positions)
    assert tree.root() == root
    for w, path in zip(ws, paths):
        assert w.path() == path and w.root() == root


# ---- the native call under advance ----
B, T = MT_BLOCK, MT_TOP_PARENTS
STARTS = (0, 1, 2, 3, 6, 7, (1 << 20) + 3, (1 << 32) - 4)
COUNTS = (0, 1, 2, 3, 5, 37, 2 * T, 2 * T + 2)


def block_case(start, n):
    rng = random.Random(7800 + start % 1000 + n)
    frontier = [rng.randrange(Q).to_bytes(32, "little") if (start >> h) & 1 else bytes([0xff]) * 32 for h in range(32)]   # unused: never read
    return frontier, R.random_nodes(n, 7900 + start % 1000 + n)


@pytest.mark.parametrize("start,n", [(s, n) for s in STARTS for n in COUNTS if s + n <= 1 << 32])
def test_the_host_call_against_the_definition(start, n):
    frontier, row = block_case(start, n)
    got = H.merkle_tree_append(start, arr(frontier), arr(row), threads=3)
    assert got.shape == (H.merkle_append_node_count(start, n), 32)
    assert R.as_list(got) == IR.block_nodes(start, frontier, row)


def test_the_host_call_refuses():
    L = H.load_library()
    import ctypes as C
    frontier, row = block_case(7, 5)
    row[3] = NOT_CANONICAL
    row[4] = NOT_CANONICAL
    with pytest.raises(ValueError) as e:
        H.merkle_tree_append(7, arr(frontier), arr(row))
    assert e.value.bad_index == 3
    frontier, row = block_case(7, 5)
    frontier[2] = NOT_CANONICAL
    with pytest.raises(ValueError) as e:
        H.merkle_tree_append(7, arr(frontier), arr(row))
    assert e.value.bad_index == -2 - 2
    frontier[3] = NOT_CANONICAL                     # bit 3 of 7 is clear: ignored
    frontier[2] = row[0]
    assert H.merkle_tree_append(7, arr(frontier), arr(row)).shape[0] == H.merkle_append_node_count(7, 5)
    with pytest.raises(ValueError):
        H.merkle_tree_append((1 << 32) - 4, arr(frontier), arr(row))            # start + n > 2^32
    # too little room: the count, and not a byte written
    need = H.merkle_append_node_count(7, 5)
    out = np.full((need, 32), 0xa5, np.uint8)
    nn, bad = C.c_size_t(0), C.c_int64(0)
    f, r = arr(frontier), arr(row)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.masp_host_merkle_tree_append(7, vp(f), 5, vp(r), vp(out), need - 1, C.byref(nn), C.byref(bad), 2)
    assert rc == H.E_CAPACITY and nn.value == need and bad.value == -1 and (out == 0xa5).all()
    r2 = arr(row[:4] + [NOT_CANONICAL])
    rc = L.masp_host_merkle_tree_append(7, vp(f), 5, vp(r2), vp(out), need, C.byref(nn), C.byref(bad), 2)
    assert rc == 1 and bad.value == 4 and (out == 0xa5).all()
    rc = L.masp_host_merkle_tree_append(7, vp(f), 5, vp(r), vp(out), need, C.byref(nn), C.byref(bad), 2)
    assert rc == 0 and R.as_list(out) == IR.block_nodes(7, frontier, row)
