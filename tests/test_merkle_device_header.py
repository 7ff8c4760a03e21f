"""device/merkle.hpp on the CPU (tests/merkle_shim.py compiles it for the host): the Merkle hash of the commitment tree's kernels against
host.merkle_hash, the pinned one-hash primitive, and the canonicity test against the BLS12-381 scalar modulus.  Every comparison is of bytes."""
import json
import os
import random

import merkle_shim as S
from masp_amd import host as H

Q = H.FR_MODULUS
LEVELS = (0, 1, 31, 32, 62)      # 62 = 0b111110: with level 1, every personalisation bit is set and cleared


def b(x):
    return x.to_bytes(32, "little")


def check(items):
    got = S.combine(items)
    for (level, lhs, rhs), g in zip(items, got):
        assert g == H.merkle_hash(level, lhs, rhs), (level, lhs.hex(), rhs.hex())
    return got


def test_random_nodes_at_the_levels():
    rng = random.Random(1201)
    check([(level, b(rng.randrange(Q)), b(rng.randrange(Q))) for level in LEVELS for _ in range(4)])


def test_edge_nodes():
    rng = random.Random(1202)
    high = [x for x in (Q - 1, (1 << 254), (1 << 254) + 1, (1 << 254) | rng.getrandbits(200)) if x < Q]
    assert all(x >> 254 == 1 for x in high)                                   # bit 254 set: the message's 255th bit of a node
    low = [(1 << 254) - 1, (1 << 253) - 1, (1 << 64) - 1]                     # bit 254 clear, the low bits all set
    values = [0, 1] + high + low
    items = [(level, b(x), b(y)) for level in (0, 31, 62) for x in values for y in (0, 1, Q - 1, (1 << 254) - 1)]
    items += [(level, b(y), b(x)) for level in (1, 32) for x in values for y in (Q - 1, 0)]
    check(items)


def test_swapping_the_children_changes_the_parent():
    rng = random.Random(1203)
    for level in LEVELS:
        x, y = b(rng.randrange(Q)), b(rng.randrange(Q))
        p, q = check([(level, x, y), (level, y, x)])
        assert p != q
    # ... and so does the level, and a node's bit 254 alone
    lo, y = rng.getrandbits(200), b(rng.randrange(Q))
    got = check([(3, b(lo), y), (4, b(lo), y), (3, b(lo | 1 << 254), y), (3, y, b(lo)), (3, y, b(lo | 1 << 254))])
    assert len(set(got)) == 5


def test_fr_is_canonical():
    nodes = [b(Q - 1), b(Q), b(Q + 1), b((1 << 256) - 1), b(0), b(1), b(1 << 255), b(Q - (1 << 32)), b(Q + (1 << 224))]
    assert S.is_canonical(nodes) == [True, False, False, False, True, True, False, True, False]
    rng = random.Random(1204)
    for _ in range(64):
        x = rng.getrandbits(256)
        assert S.is_canonical([b(x)]) == [x < Q]
        # H.merkle_hash refuses exactly these (Fr::from_bytes)
        try:
            H.merkle_hash(0, b(x), b(0))
            ok = True
        except ValueError:
            ok = False
        assert ok == (x < Q)


def test_golden_merkle_vectors_of_510_bits():
    """the reference's Pedersen vectors with the MerkleTree personalisation and exactly 6 + 510 bits are two 255-bit nodes"""
    vs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pedersen_hash_vectors.json")))
    items, want = [], []
    for v in vs:
        if v["personalization"] >= 0 and len(v["input_bits"]) == 516:
            bits = v["input_bits"][6:]
            lhs = sum(bit << i for i, bit in enumerate(bits[:255]))
            rhs = sum(bit << i for i, bit in enumerate(bits[255:]))
            # (255 bits may exceed the modulus: the device function hashes bits, as the reference's pedersen_hash does)
            items.append((v["personalization"], b(lhs), b(rhs)))
            want.append(int(v["u"], 16).to_bytes(32, "little"))
    print("%d golden MerkleTree vectors of 510 bits" % len(items))
    if items:
        assert S.combine(items) == want


def test_row_layout_matches_the_reference_walk():
    for n in (1, 2, 3, 5, 37, 4097, (1 << 22) - 1):
        start, width = 0, n
        for i in range(33):
            assert S.row(n, i) == (start, width)
            width += width & 1
            start += width
            width //= 2
