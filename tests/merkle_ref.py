"""The tests' yardstick for the commitment tree: a plain-Python transcription of FrozenCommitmentTree's `complete`, `merge`, `root` and `path`
(masp_primitives/src/merkle_tree.rs:105-256) over host.merkle_hash, the one-hash primitive that the circuit tests and
tests/golden/pedersen_hash_vectors.json pin.  Nothing here calls the tree functions under test.  Nodes are 32-byte strings."""
import functools
import random

from masp_amd import host as H

DEPTH = 32
Q = H.FR_MODULUS


@functools.lru_cache(maxsize=None)
def combine(level, lhs, rhs):
    return H.merkle_hash(level, lhs, rhs)


@functools.lru_cache(maxsize=None)
def empty_root(level):
    return (1).to_bytes(32, "little") if level == 0 else combine(level - 1, empty_root(level - 1), empty_root(level - 1))


def complete(tree, prev_start, prev_width, heightp):
    """appends to `tree` (a list) every row above the one at prev_start, as merkle_tree.rs:177-205"""
    tree = list(tree)
    for height in range(heightp, DEPTH):
        if prev_width % 2 == 1:
            prev_width += 1
            tree.append(empty_root(height))
        for j in range(prev_width // 2):
            tree.append(combine(height, tree[prev_start + 2 * j], tree[prev_start + 2 * j + 1]))
        prev_start += prev_width
        prev_width //= 2
    return tree


def new(leaves):
    return complete(list(leaves), 0, len(leaves), 0)


def root(tree):
    return tree[-1] if tree else empty_root(DEPTH)


def path(tree, size, pos, height0=0):
    """[(sibling, is_right)] of position pos in a vector whose first row has `size` nodes of level height0 (merkle_tree.rs:214-251)"""
    out, start, width = [], 0, size
    for height in range(height0, DEPTH):
        if width % 2 == 1:
            width += 1
        if pos % 2 == 0:
            out.append((tree[start + pos + 1] if pos + 1 < width else empty_root(height), False))
        else:
            out.append((tree[start + pos - 1] if pos - 1 < width else empty_root(height), True))
        start += width
        width //= 2
        pos //= 2
    return out


def merge(subtrees):
    """subtrees: [(vector, size)] -> (vector, size), merkle_tree.rs:123-175 without its asserts"""
    if not subtrees:
        return [], 0
    if len(subtrees) == 1:
        return list(subtrees[0][0]), subtrees[0][1]
    height, first_start, first_width = 0, 0, subtrees[0][1]
    last_start, last_width = 0, subtrees[-1][1]
    prev_start, prev_width = 0, (len(subtrees) - 1) * first_width + last_width
    leafs, tree = prev_width, []
    while True:
        if last_width % 2 == 1 and first_width > 1:
            last_width += 1
            prev_width += 1
        for vec, _ in subtrees[:-1]:
            tree.extend(vec[first_start:first_start + first_width])
        tree.extend(subtrees[-1][0][last_start:last_start + last_width])
        if first_width == 1:
            break
        first_start += first_width
        first_width //= 2
        last_start += last_width
        last_width //= 2
        prev_start += prev_width
        prev_width //= 2
        height += 1
    return complete(tree, prev_start, prev_width, height), leafs


def random_nodes(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(Q).to_bytes(32, "little") for _ in range(n)]


def as_list(nodes):
    """an (N, 32) uint8 array as a list of 32-byte strings"""
    return [bytes(r) for r in nodes]
