"""Commitment trees of masp_primitives/src/merkle_tree.rs over the depth-32 Sapling tree.  Nodes are 32-byte little-endian canonical
scalars (`Node::read`).

Frozen: `FrozenCommitmentTree` and `MerklePath` (:105-256).  The hashing is one native call per tree: masp_hip_merkle_tree_complete on a
`Context` (k_merkle.hip, every row one launch), or masp_host_merkle_tree_complete on host threads with ctx=None.

Incremental: `CommitmentTree` and `IncrementalWitness` (:271-723), the state a wallet keeps between two syncs, in the reference's byte
format.  `append` is the reference's one hash chain per leaf; `advance` takes a whole block through the tree and all of its witnesses with
one native call (masp_hip_merkle_tree_append on a `Context`, masp_host_merkle_tree_append with ctx=None) and index arithmetic."""
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


# ---- the incremental tree: CommitmentTree, IncrementalWitness (merkle_tree.rs:271-723) and advance ----
def _node(x):
    x = bytes(x)
    if len(x) != 32:
        raise ValueError("a node is 32 bytes")
    if int.from_bytes(x, "little") >= host.FR_MODULUS:
        raise ValueError("a node is a canonical scalar")
    return x


class _Filler:
    """PathFiller (merkle_tree.rs:87-103): the nodes a root or a path still lacks, then empty roots"""

    def __init__(self, queue=()):
        self.queue = list(queue)

    def next(self, level):
        return self.queue.pop(0) if self.queue else empty_root(level)


class _Reader:
    def __init__(self, data):
        self.data, self.at = bytes(data), 0

    def take(self, n):
        if self.at + n > len(self.data):
            raise ValueError("the serialisation ends early")
        self.at += n
        return self.data[self.at - n:self.at]

    def compact_size(self):
        b = self.take(1)[0]
        return b if b < 253 else int.from_bytes(self.take({253: 2, 254: 4, 255: 8}[b]), "little")

    def flag(self):
        b = self.take(1)[0]
        if b > 1:
            raise ValueError("an Optional's first byte is 0 or 1")
        return b

    def optional_node(self):
        return _node(self.take(32)) if self.flag() else None

    def end(self):
        if self.at != len(self.data):
            raise ValueError("%d bytes behind the serialisation" % (len(self.data) - self.at))


def _compact_size(n):
    return bytes([n]) if n < 253 else b"\xfd" + n.to_bytes(2, "little")


def _optional(node):
    return b"\x00" if node is None else b"\x01" + node


class CommitmentTree:
    """CommitmentTree { left, right, parents }: the frontier of the tree, at most 33 nodes.  The state is the reference's lazy one: a full
    pair (left, right) is folded into `parents` only by the next append, `parents` is never trimmed, and a slot that was used once stays
    (as None).  parents[k] is the root of a complete subtree of 2^(k+1) leaves; size() reads their occupation as a binary number."""

    def __init__(self):
        self.left, self.right, self.parents = None, None, []

    @classmethod
    def empty(cls):
        return cls()

    def copy(self):
        t = CommitmentTree()
        t.left, t.right, t.parents = self.left, self.right, list(self.parents)
        return t

    def size(self):
        return (self.left is not None) + (self.right is not None) + sum(1 << (i + 1) for i, p in enumerate(self.parents) if p is not None)

    def _is_complete(self, depth):
        if depth == 0:
            return self.left is not None and self.right is None and not self.parents
        return self.left is not None and self.right is not None and len(self.parents) >= depth - 1 and \
            all(p is not None for p in self.parents[:depth - 1])

    def append(self, node, depth=DEPTH):
        """append_inner: one leaf; folding a full pair is one hash per level it carries through.  A full tree raises ValueError."""
        node = _node(node)
        if self._is_complete(depth):
            raise ValueError("the tree is full")
        if self.left is None:
            self.left = node
        elif self.right is None:
            self.right = node
        else:
            combined = host.merkle_hash(0, self.left, self.right)
            self.left, self.right = node, None
            for i in range(depth):
                if i < len(self.parents):
                    if self.parents[i] is not None:
                        combined = host.merkle_hash(i + 1, self.parents[i], combined)
                        self.parents[i] = None
                    else:
                        self.parents[i] = combined
                        break
                else:
                    self.parents.append(combined)
                    break

    def extend(self, nodes, ctx=None):
        """every node of `nodes` appended, as one block: advance(self, [], nodes, (), ctx)"""
        advance(self, [], nodes, (), ctx)

    def root(self, depth=DEPTH, _filler=None):
        """root_inner: the root of the tree of `depth` levels, what is missing on the right filled with empty roots"""
        assert depth > 0
        filler = _filler or _Filler()
        left = self.left if self.left is not None else filler.next(0)
        right = self.right if self.right is not None else filler.next(0)
        root = host.merkle_hash(0, left, right)
        for i in range(depth - 1):
            p = self.parents[i] if i < len(self.parents) else None
            root = host.merkle_hash(i + 1, p, root) if p is not None else host.merkle_hash(i + 1, root, filler.next(i + 1))
        return root

    def write(self):
        """the reference's serialisation, the format wallets store: Optional(left) Optional(right) Vector(Optional(parent))"""
        return _optional(self.left) + _optional(self.right) + _compact_size(len(self.parents)) + b"".join(_optional(p) for p in self.parents)

    @classmethod
    def _read_from(cls, r):
        t = cls()
        t.left, t.right = r.optional_node(), r.optional_node()
        count = r.compact_size()
        if count > DEPTH:
            raise ValueError("a tree of depth %d has at most %d parents, not %d" % (DEPTH, DEPTH, count))
        t.parents = [r.optional_node() for _ in range(count)]
        if t.left is None and (t.right is not None or any(p is not None for p in t.parents)):
            raise ValueError("a tree without a left leaf is empty")      # (no sequence of appends leaves such a state)
        return t

    @classmethod
    def read(cls, data):
        """CommitmentTree::read of exactly `data`; a node that is not canonical, more than 32 parents, a state that no appends reach and
        bytes left over raise ValueError"""
        r = _Reader(data)
        t = cls._read_from(r)
        r.end()
        return t

    def __eq__(self, other):
        return isinstance(other, CommitmentTree) and (self.left, self.right, self.parents) == (other.left, other.right, other.parents)

    def __repr__(self):
        return "CommitmentTree(size=%d)" % self.size()


class IncrementalWitness:
    """IncrementalWitness { tree, filled, cursor_depth, cursor }: `tree` is the tree as it was when its last leaf, the witnessed one, was
    appended; `filled` the roots of the complete subtrees to its right that its path needs, lowest first; `cursor` the lazy tree of the
    first such subtree that is begun and not complete, `cursor_depth` its level."""

    def __init__(self, tree):
        self.tree, self.filled, self.cursor_depth, self.cursor = tree, [], 0, None

    @classmethod
    def from_tree(cls, tree):
        """the witness of the leaf appended last.  The empty tree raises ValueError (the reference builds a witness there that can never
        form a path)."""
        if tree.left is None:
            raise ValueError("the empty tree has no leaf to witness")
        return cls(tree.copy())

    def position(self):
        return self.tree.size() - 1

    def _filler(self):
        queue = list(self.filled)
        if self.cursor is not None:
            queue.append(self.cursor.root(self.cursor_depth))
        return _Filler(queue)

    def next_depth(self):
        """the level of the next subtree that `filled` lacks"""
        skip = len(self.filled)
        for missing in (self.tree.left is None, self.tree.right is None):
            if missing:
                if skip == 0:
                    return 0
                skip -= 1
        d = 1
        for p in self.tree.parents:
            if p is None:
                if skip == 0:
                    return d
                skip -= 1
            d += 1
        return d + skip

    def append(self, node, depth=DEPTH):
        """append_inner: one leaf that the tree has been given too.  A full tree raises ValueError."""
        node = _node(node)
        if self.cursor is not None:
            self.cursor.append(node, depth)
            if self.cursor._is_complete(self.cursor_depth):
                self.filled.append(self.cursor.root(self.cursor_depth))
                self.cursor = None
        else:
            cursor_depth = self.next_depth()
            if cursor_depth >= depth:
                raise ValueError("the tree is full")
            self.cursor_depth = cursor_depth
            if cursor_depth == 0:
                self.filled.append(node)
            else:
                self.cursor = CommitmentTree()
                self.cursor.append(node, depth)

    def root(self, depth=DEPTH):
        return self.tree.root(depth, self._filler())

    def path(self, depth=DEPTH):
        """path_inner: the witnessed leaf's MerklePath in the tree as it is now"""
        filler = self._filler()
        t = self.tree
        auth = [(t.left, True) if t.right is not None else (filler.next(0), False)]
        for i in range(depth - 1):
            p = t.parents[i] if i < len(t.parents) else None
            auth.append((p, True) if p is not None else (filler.next(i + 1), False))
        return MerklePath(auth, self.position())

    def write(self):
        """the reference's serialisation: the tree, Vector(filled), Optional(cursor)"""
        out = self.tree.write() + _compact_size(len(self.filled)) + b"".join(self.filled)
        return out + (b"\x00" if self.cursor is None else b"\x01" + self.cursor.write())

    @classmethod
    def read(cls, data):
        r = _Reader(data)
        tree = CommitmentTree._read_from(r)
        if tree.left is None:
            raise ValueError("the empty tree has no leaf to witness")
        w = cls(tree)
        count = r.compact_size()
        if count > DEPTH:
            raise ValueError("a witness fills at most %d subtrees, not %d" % (DEPTH, count))
        w.filled = [_node(r.take(32)) for _ in range(count)]
        w.cursor = CommitmentTree._read_from(r) if r.flag() else None
        r.end()
        w.cursor_depth = w.next_depth()
        return w

    def __eq__(self, other):
        return isinstance(other, IncrementalWitness) and (self.tree, self.filled, self.cursor) == (other.tree, other.filled, other.cursor)

    def __repr__(self):
        return "IncrementalWitness(position=%d, %d filled%s)" % (self.position(), len(self.filled), ", cursor" if self.cursor else "")


def _append_nodes(start, frontier, row, ctx):
    if ctx is None:
        return host.merkle_tree_append(start, frontier, row)
    try:
        return ctx.merkle_tree_append(start, frontier, row)
    except Exception as e:
        if getattr(e, "bad_index", -1) != -1:       # as the host path reports it
            err = ValueError(str(e))
            err.bad_index = e.bad_index
            raise err from e
        raise


class _Pool:
    """Where a node (level, index) lies among the results of one append call over the leaves [E, S): the row first, then level by level
    the nodes (h, i) for E >> h <= i < S >> h.  Index arithmetic on int64 arrays, one entry per tree or witness."""

    def __init__(self, E, S, row, nodes):
        self.E, self.S = E, S
        self.off = [0] * (DEPTH + 2)
        self.off[1] = S - E
        for h in range(1, DEPTH + 1):
            self.off[h + 1] = self.off[h] + (S >> h) - (E >> h)
        assert row.shape[0] == S - E and nodes.shape[0] == self.off[DEPTH + 1] - self.off[1]
        self.bytes = row.tobytes() + nodes.tobytes()

    def index(self, level, i):
        """of node (level, i), or -1 where the node ends at or before E: such a node is in the old state"""
        at = self.off[level] + i - (self.E >> level)
        return np.where(i >= (self.E >> level), at, -1)

    def node(self, at):
        return self.bytes[32 * at:32 * at + 32]

    def lazy_trees(self, a, m):
        """The lazy CommitmentTree over the leaves [a, a + m) for every entry (a a multiple of 2^level of the subtree, m >= 1): pool indices
        (left[T], right[T] with -1 for none, parents[T, 32] with -2 for None and -1 for the old state's entry of that slot) and the number
        of slots that appends from empty would have used.  The pair is the leaves from P = a + ((m - 1) & ~1); slot k holds the node
        (k + 1, (P >> (k + 1)) - 1) where bit k + 1 of P - a is set."""
        F = (m - 1) & ~np.int64(1)
        P = a + F
        left = P - self.E
        right = np.where(m % 2 == 0, P + 1 - self.E, -1)
        parents = np.full((a.shape[0], DEPTH), -2, np.int64)
        used = np.zeros(a.shape[0], np.int64)
        for k in range(DEPTH - 1):
            level = k + 1
            parents[:, k] = np.where((F >> level) & 1 == 1, self.index(level, (P >> level) - 1), -2)
            used += (F >> level) != 0
        return left.tolist(), right.tolist(), parents.tolist(), used.tolist()

    def tree(self, left, right, parents, used, old_parents):
        t = CommitmentTree()
        t.left = self.node(left)
        t.right = self.node(right) if right >= 0 else None
        t.parents = [None if v == -2 else old_parents[k] if v == -1 else self.node(v) for k, v in enumerate(parents[:max(used, len(old_parents))])]
        return t


def advance(tree, witnesses, nodes, track=(), ctx=None):
    """Appends the block `nodes` to `tree` and to every witness of `witnesses`, all of them witnesses of that tree, with ONE native call
    (ctx: a masp_amd.Context for the GPU, None for host threads) and no hash in Python; the states are byte for byte those of appending
    one by one.  track: indices into `nodes`; for each, in that order, the returned list holds the witness that
    IncrementalWitness.from_tree(tree) right after nodes[k] would have become by the block's end.

    Every node that the new states hold is in the old state, is one of the leaves, or is a complete inner node whose last leaf lies in the
    block: the call hashes the last kind, everything else here is (level, index) arithmetic in numpy over all witnesses
    at once.  On any error nothing is modified: a node that is not canonical (ValueError with .bad_index, the index into `nodes`), a block
    beyond 2^32 leaves, a witness whose filled subtrees and cursor do not end where `tree` ends."""
    row = _rows(nodes)
    n = row.shape[0]
    witnesses = list(witnesses)
    track = [int(k) for k in track]
    for k in track:
        if not 0 <= k < n:
            raise ValueError("track: %d is not an index into a block of %d nodes" % (k, n))
    S0 = tree.size()
    if tree.left is None and S0:
        raise ValueError("a tree without a left leaf is empty")
    # every witness's position, what it has filled and its cursor have to end at the tree's size
    W = len(witnesses)
    p = np.array([w.position() for w in witnesses] + [S0 + k for k in track], np.int64)
    f = np.array([len(w.filled) for w in witnesses] + [0] * len(track), np.int64)
    cm = np.array([w.cursor.size() if w.cursor is not None else 0 for w in witnesses], np.int64)
    cd = np.array([w.cursor_depth if w.cursor is not None else -1 for w in witnesses], np.int64)
    if W:
        implied, seen, level = p[:W] + 1, np.zeros(W, np.int64), np.full(W, -1, np.int64)
        for h in range(DEPTH):
            clear = (p[:W] >> h) & 1 == 0
            implied = implied + np.where(clear & (seen < f[:W]), np.int64(1) << h, 0)
            level = np.where(clear & (seen == f[:W]), h, level)      # where the cursor is, if there is one
            seen = seen + clear
        ok = (p[:W] >= 0) & (f[:W] <= seen) & (implied + cm == S0) & ((cm == 0) | ((cd == level) & (level >= 1) & (cm < (np.int64(1) << np.maximum(level, 0)))))
        if not ok.all():
            k = int(np.argmin(ok))
            raise ValueError("witness %d (position %d) does not belong to a tree of %d leaves" % (k, int(p[k]), S0))
    if n == 0:
        return []
    S1 = S0 + n
    if S1 > 1 << DEPTH:
        raise ValueError("the tree is full: %d + %d leaves are more than 2^%d" % (S0, n, DEPTH))
    # the lazy pair goes in front of the row: the call starts at the even position E, and parents[k] is its frontier[k + 1]
    E = (S0 - 1) & ~1 if S0 else 0
    loose = [x for x in (tree.left, tree.right) if x is not None]
    if loose:
        row = np.concatenate([np.frombuffer(b"".join(loose), np.uint8).reshape(-1, 32), row])
    frontier = np.zeros((DEPTH, 32), np.uint8)
    for k, node in enumerate(tree.parents[:DEPTH - 1]):
        if node is not None:
            frontier[k + 1] = np.frombuffer(node, np.uint8)
    try:
        block = _append_nodes(E, frontier, row, ctx)
    except ValueError as e:
        if getattr(e, "bad_index", -1) >= 0:
            e.bad_index -= len(loose)
        raise
    pool = _Pool(E, S1, row, block)
    # the tree at the block's end, and as it was behind each tracked leaf
    zero = np.zeros(1 + len(track), np.int64)
    shapes = list(zip(*pool.lazy_trees(zero, np.array([S1] + [S0 + k + 1 for k in track], np.int64))))
    new_tree = pool.tree(*shapes[0], tree.parents)
    made = [IncrementalWitness(pool.tree(*s, tree.parents)) for s in shapes[1:]]
    # the witnesses: per level with a clear bit of the position, the right sibling's subtree [a, a + 2^h) is complete (filled), begun (the
    # cursor) or empty
    T = p.shape[0]
    fill = np.full((T, DEPTH), -1, np.int64)
    seen, done = np.zeros(T, np.int64), np.zeros(T, bool)
    cur_h, cur_a = np.full(T, -1, np.int64), np.zeros(T, np.int64)
    for h in range(DEPTH):
        clear = ((p >> h) & 1 == 0) & ~done
        a = ((p >> h) + 1) << h
        complete = clear & (a + (np.int64(1) << h) <= S1)
        fill[:, h] = np.where(complete & (seen >= f), pool.index(h, (p >> h) + 1), -1)
        begun = clear & ~complete & (a < S1)
        cur_h, cur_a = np.where(begun, h, cur_h), np.where(begun, a, cur_a)
        done |= clear & ~complete
        seen = seen + complete
    has = np.nonzero(cur_h >= 0)[0]
    cursors = dict(zip(has.tolist(), zip(*pool.lazy_trees(cur_a[has], S1 - cur_a[has])))) if has.shape[0] else {}
    fill, cur_h = fill.tolist(), cur_h.tolist()
    state = []
    for k, w in enumerate(witnesses + made):
        filled = w.filled + [pool.node(at) for at in fill[k] if at >= 0]
        cursor = None
        if k in cursors:        # (a cursor of the same level goes on from the old one's nodes, any other starts behind the old tree's end)
            cursor = pool.tree(*cursors[k], w.cursor.parents if w.cursor is not None and w.cursor_depth == cur_h[k] else [])
        state.append((filled, cursor, cur_h[k]))
    # nothing can fail from here on
    tree.left, tree.right, tree.parents = new_tree.left, new_tree.right, new_tree.parents
    for w, (filled, cursor, depth) in zip(witnesses + made, state):
        w.filled, w.cursor = filled, cursor
        w.cursor_depth = depth if cursor is not None else w.next_depth()
    return made
