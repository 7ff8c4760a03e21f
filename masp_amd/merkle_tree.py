"""Frozen commitment trees: `FrozenCommitmentTree` and `MerklePath` of masp_primitives/src/merkle_tree.rs:105-256 over the depth-32 Sapling
tree.  The hashing is one native call per tree: masp_hip_merkle_tree_complete on a `Context` (k_merkle.hip, every row one launch), or
masp_host_merkle_tree_complete on host threads with ctx=None.  Nodes are 32-byte little-endian canonical scalars (`Node::read`)."""
import numpy as np

from . import host

DEPTH = host.TREE_DEPTH
# k_merkle.hip's geometry, for callers that size their tests by it (tests/test_merkle_tree_host.py compares them with the source)
MT_BLOCK = 256            # lanes (parents) per workgroup of k_mt_level
MT_TOP_PARENTS = 64       # a row of at most this many parents is finished by k_mt_top, one wave over the remaining levels

_empty = None


def empty_root(level):
    """Node::empty_root(level), 32 bytes: level 0 is the uncommitted leaf 1 (Node::blank)"""
    global _empty
    if _empty is None:
        _empty = [r.tobytes() for r in host.merkle_empty_roots()]
    return _empty[level]


def _rows(leaves):
    if isinstance(leaves, np.ndarray):
        return np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
    leaves = list(leaves)
    for x in leaves:
        if len(bytes(x)) != 32:
            raise ValueError("a node is 32 bytes")
    return np.frombuffer(b"".join(bytes(x) for x in leaves), np.uint8).reshape(-1, 32)


def _complete(row, height0, positions, want_nodes, ctx):
    if ctx is None:
        return host.merkle_tree_complete(row, height0, positions, want_nodes)
    try:
        return ctx.merkle_tree_complete(row, height0, positions, want_nodes)
    except Exception as e:
        if getattr(e, "bad_index", -1) >= 0:       # as the host path reports it
            err = ValueError(str(e))
            err.bad_index = e.bad_index
            raise err from e
        raise


class MerklePath:
    """MerklePath { auth_path: Vec<(Node, bool)>, position }: per level the sibling and whether the path's own node is the RIGHT child there
    (bit i of the position).  Unpacks as (siblings, position), the form prover.spend_proof / convert_proof take."""

    def __init__(self, auth_path, position):
        self.auth_path = [(bytes(node), bool(is_right)) for node, is_right in auth_path]
        self.position = int(position)

    @property
    def siblings(self):
        return [node for node, _ in self.auth_path]

    def __iter__(self):
        return iter((self.siblings, self.position))

    def root(self, leaf):
        """the root this path gives the leaf (MerklePath::root)"""
        cur = bytes(leaf)
        for i, (node, is_right) in enumerate(self.auth_path):
            cur = host.merkle_hash(i, node, cur) if is_right else host.merkle_hash(i, cur, node)
        return cur

    def __eq__(self, other):
        return isinstance(other, MerklePath) and self.auth_path == other.auth_path and self.position == other.position

    def __repr__(self):
        return "MerklePath(position=%d, %d siblings)" % (self.position, len(self.auth_path))


def _path_of(siblings, position, height0=0):
    return MerklePath([(bytes(siblings[i]), bool((position >> i) & 1)) for i in range(DEPTH - height0)], position)


class FrozenCommitmentTree:
    """FrozenCommitmentTree<Node>(Vec<Node>, usize): every row of the depth-32 tree over `leaves`, each padded to an even width with
    empty_root(level), one behind the other, the root last.  ctx: a masp_amd.Context (the rows are hashed on the GPU) or None (host threads)."""

    def __init__(self, leaves=(), ctx=None):
        row = _rows(leaves)
        self.nodes, self._root, _ = _complete(row, 0, (), True, ctx)
        self._size = row.shape[0]

    @classmethod
    def _of(cls, nodes, size):
        t = cls.__new__(cls)
        t.nodes = np.ascontiguousarray(nodes, dtype=np.uint8).reshape(-1, 32)
        t._size = size
        t._root = t.nodes[-1].tobytes() if t.nodes.shape[0] else empty_root(DEPTH)
        return t

    def size(self):
        return self._size

    def root(self):
        return self._root

    def path(self, pos):
        """the Merkle path of leaf `pos` out of the node vector (merkle_tree.rs:214-251); pos >= size() raises ValueError (the reference
        returns a path of padding there: an artefact, not a witness)"""
        pos = int(pos)
        if not 0 <= pos < self._size:
            raise ValueError("position %d is not in a tree of %d leaves" % (pos, self._size))
        auth, position, start, width = [], pos, 0, self._size
        for height in range(DEPTH):
            width += width & 1
            sib = pos ^ 1
            node = self.nodes[start + sib].tobytes() if sib < width else empty_root(height)
            auth.append((node, bool(pos & 1)))
            start += width
            width //= 2
            pos //= 2
        return MerklePath(auth, position)

    @classmethod
    def paths(cls, leaves, positions, ctx=None):
        """root and paths only: (root, [MerklePath]) for `positions` of a tree over `leaves`, the node vector never leaving the device"""
        positions = [int(p) for p in positions]
        row = _rows(leaves)
        for p in positions:
            if not 0 <= p < row.shape[0]:
                raise ValueError("position %d is not in a tree of %d leaves" % (p, row.shape[0]))
        _, root, sib = _complete(row, 0, positions, False, ctx)
        return root, [_path_of([s.tobytes() for s in sib[k]], p) for k, p in enumerate(positions)]

    @classmethod
    def merge(cls, subtrees, ctx=None):
        """FrozenCommitmentTree::merge (merkle_tree.rs:123-175): all subtrees but the last are full and of one power-of-two size, the last is
        no larger.  Their rows are stitched up to the height where the full ones end; ONE complete call hashes the rest from that row."""
        subtrees = list(subtrees)
        if not subtrees:
            return cls._of(np.zeros((0, 32), np.uint8), 0)
        if len(subtrees) == 1:
            return cls._of(subtrees[0].nodes.copy(), subtrees[0].size())
        size = subtrees[0].size()
        assert size > 0 and size & (size - 1) == 0, "the full subtrees' size is a power of two"
        for t in subtrees[:-1]:
            assert t.size() == size, "all subtrees but the last have one size"
        last = subtrees[-1]
        # (the reference asks no more; a larger last subtree would give a tree that is none)
        assert last.size() <= size, "the last subtree is no larger than the full ones"
        height, first_start, first_width, last_start, last_width = 0, 0, size, 0, last.size()
        prev_start, prev_width = 0, (len(subtrees) - 1) * size + last_width
        leafs = prev_width
        rows = []
        while True:
            if last_width % 2 == 1 and first_width > 1:      # the parent's right child must be there
                last_width += 1
                prev_width += 1
            for t in subtrees[:-1]:
                rows.append(t.nodes[first_start:first_start + first_width])
            rows.append(last.nodes[last_start:last_start + last_width])
            if first_width == 1:
                break
            first_start += first_width
            first_width //= 2
            last_start += last_width
            last_width //= 2
            prev_start += prev_width
            prev_width //= 2
            height += 1
        stitched = np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8)
        assert stitched.shape[0] == prev_start + prev_width
        top, _, _ = _complete(stitched[prev_start:], height, (), True, ctx)
        return cls._of(np.concatenate([stitched[:prev_start], top]), leafs)
