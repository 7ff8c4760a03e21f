"""The tests' yardstick for the incremental commitment tree: a plain-Python transcription of CommitmentTree's and IncrementalWitness's
one-by-one `append_inner`, `root_inner`, `path_inner`, `next_depth`, `read` and `write` (masp_primitives/src/merkle_tree.rs:271-723)
over host.merkle_hash through merkle_ref.combine.  Nothing here calls the tree code under test.  Nodes are 32-byte strings."""
from merkle_ref import DEPTH, combine, empty_root


class Filler:
    """PathFiller (merkle_tree.rs:87-103)"""

    def __init__(self, queue=()):
        self.queue = list(queue)

    def next(self, depth):
        return self.queue.pop(0) if self.queue else empty_root(depth)


def _compact(n):
    if n < 253:
        return bytes([n])
    assert n <= 0xffff
    return b"\xfd" + n.to_bytes(2, "little")


def _opt(node):
    return b"\x00" if node is None else b"\x01" + node


class Reader:
    def __init__(self, data):
        self.data, self.at = bytes(data), 0

    def take(self, n):
        assert self.at + n <= len(self.data)
        self.at += n
        return self.data[self.at - n:self.at]

    def compact(self):
        b = self.take(1)[0]
        return b if b < 253 else int.from_bytes(self.take(2), "little")

    def opt(self):
        flag = self.take(1)[0]
        assert flag in (0, 1)
        return self.take(32) if flag else None


class Tree:
    def __init__(self):
        self.left, self.right, self.parents = None, None, []

    def copy(self):
        t = Tree()
        t.left, t.right, t.parents = self.left, self.right, list(self.parents)
        return t

    def size(self):
        return (self.left is not None) + (self.right is not None) + sum(1 << (i + 1) for i, p in enumerate(self.parents) if p is not None)

    def is_complete(self, depth):
        if depth == 0:
            return self.left is not None and self.right is None and not self.parents
        padded = (self.parents + [None] * depth)[:depth - 1]
        return self.left is not None and self.right is not None and all(p is not None for p in padded)

    def append(self, node, depth=DEPTH):
        """False where the reference returns Err(())"""
        if self.is_complete(depth):
            return False
        if self.left is None:
            self.left = node
        elif self.right is None:
            self.right = node
        else:
            combined = combine(0, self.left, self.right)
            self.left, self.right = node, None
            for i in range(depth):
                if i < len(self.parents):
                    if self.parents[i] is not None:
                        combined = combine(i + 1, self.parents[i], combined)
                        self.parents[i] = None
                    else:
                        self.parents[i] = combined
                        break
                else:
                    self.parents.append(combined)
                    break
        return True

    def root(self, depth=DEPTH, filler=None):
        filler = filler or Filler()
        assert depth > 0
        left = self.left if self.left is not None else filler.next(0)
        right = self.right if self.right is not None else filler.next(0)
        root = combine(0, left, right)
        for i, p in enumerate((self.parents + [None] * depth)[:depth - 1]):
            root = combine(i + 1, p, root) if p is not None else combine(i + 1, root, filler.next(i + 1))
        return root

    def write(self):
        return _opt(self.left) + _opt(self.right) + _compact(len(self.parents)) + b"".join(_opt(p) for p in self.parents)

    @classmethod
    def read_from(cls, r):
        t = cls()
        t.left, t.right = r.opt(), r.opt()
        t.parents = [r.opt() for _ in range(r.compact())]
        return t

    @classmethod
    def read(cls, data):
        return cls.read_from(Reader(data))


class Witness:
    def __init__(self, tree):
        self.tree, self.filled, self.cursor_depth, self.cursor = tree.copy(), [], 0, None

    def position(self):
        return self.tree.size() - 1

    def filler(self):
        queue = list(self.filled)
        if self.cursor is not None:
            queue.append(self.cursor.root(self.cursor_depth))
        return Filler(queue)

    def next_depth(self):
        skip = len(self.filled)
        if self.tree.left is None:
            if skip > 0:
                skip -= 1
            else:
                return 0
        if self.tree.right is None:
            if skip > 0:
                skip -= 1
            else:
                return 0
        d = 1
        for p in self.tree.parents:
            if p is None:
                if skip > 0:
                    skip -= 1
                else:
                    return d
            d += 1
        return d + skip

    def append(self, node, depth=DEPTH):
        if self.cursor is not None:
            cursor, self.cursor = self.cursor, None
            assert cursor.append(node, depth), "cursor should not be full"
            if cursor.is_complete(self.cursor_depth):
                self.filled.append(cursor.root(self.cursor_depth))
            else:
                self.cursor = cursor
        else:
            self.cursor_depth = self.next_depth()
            if self.cursor_depth >= depth:
                return False
            if self.cursor_depth == 0:
                self.filled.append(node)
            else:
                cursor = Tree()
                assert cursor.append(node, depth)
                self.cursor = cursor
        return True

    def root(self, depth=DEPTH):
        return self.tree.root(depth, self.filler())

    def path(self, depth=DEPTH):
        """([(sibling, is_right)], position), or None for the witness of the empty tree"""
        filler = self.filler()
        if self.tree.left is None:
            return None
        auth = [(self.tree.left, True) if self.tree.right is not None else (filler.next(0), False)]
        for i, p in enumerate((self.tree.parents + [None] * depth)[:depth - 1]):
            auth.append((p, True) if p is not None else (filler.next(i + 1), False))
        assert len(auth) == depth
        return auth, self.position()

    def write(self):
        out = self.tree.write() + _compact(len(self.filled)) + b"".join(self.filled)
        return out + (b"\x00" if self.cursor is None else b"\x01" + self.cursor.write())

    @classmethod
    def read(cls, data):
        r = Reader(data)
        w = cls(Tree.read_from(r))
        w.filled = [r.take(32) for _ in range(r.compact())]
        flag = r.take(1)[0]
        w.cursor = Tree.read_from(r) if flag else None
        w.cursor_depth = w.next_depth()
        return w


def path_ser(auth, position):
    """MerklePath's serialisation (merkle_tree.rs:845-863): the depth, the siblings from the top down each behind its length, the position"""
    out = bytes([len(auth)])
    for node, _ in reversed(auth):
        out += b"\x20" + node
    return out + position.to_bytes(8, "little")


def block_nodes(start, frontier, row):
    """What a block of leaves `row` at position `start` completes, by the definition alone: for h = 1..32 in turn the nodes (h, i) with
    start >> h <= i < (start + len(row)) >> h, each the hash of its two children, found top-down; a node that ends at or before `start`
    is the old frontier's (frontier[h] = node (h, (start >> h) - 1), 32 entries, read where bit h of start is set)."""
    end = start + len(row)
    memo = {}

    def node(h, i):
        if ((i + 1) << h) <= start:
            assert i == (start >> h) - 1 and (start >> h) & 1, "only the frontier's nodes lie before the block"
            return frontier[h]
        if h == 0:
            return row[i - start]
        if (h, i) not in memo:
            memo[h, i] = combine(h - 1, node(h - 1, 2 * i), node(h - 1, 2 * i + 1))
        return memo[h, i]

    return [node(h, i) for h in range(1, DEPTH + 1) for i in range(start >> h, end >> h)]
