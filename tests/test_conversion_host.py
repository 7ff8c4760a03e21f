"""Allowed conversions in batches on the host (masp_host_allowed_conversions, masp_amd/convert.py with ctx=None) against
conversion_ref's composition of vector-pinned primitives, against host.AllowedConversion one by one, and with the Convert circuit as
judge of the leaf.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import conversion_ref as R
from masp_amd import FrozenCommitmentTree, convert
from masp_amd import host as H
from masp_amd.convert import AllowedConversion, batch


def _same(got, want):
    for x, y in zip(got, want):
        assert (x is None and y is None) or np.array_equal(x, y)


def test_the_random_batch_has_every_status():
    _, want = R.references("random130")
    status = [w[0] for w in want]
    assert status.count(0) >= 40 and status.count(1) >= 10 and status.count(2) >= 5 and len(status) == 130


def test_edges_against_the_reference():
    convs, want = R.references("edges")
    got = H.allowed_conversions(*R.arrays(convs), threads=1)
    R.check(got, want)
    status, gens, cmus = got
    assert status[R.edge("empty")] == 0 and gens[R.edge("empty")].tobytes() == H.JUBJUB_IDENTITY
    assert gens[R.edge("cancels")].tobytes() == H.JUBJUB_IDENTITY and gens[R.edge("zero")].tobytes() == H.JUBJUB_IDENTITY
    assert gens[R.edge("+2^64")].tobytes() == H.JUBJUB_IDENTITY                      # truncates to 0
    assert gens[R.edge("+2^64+5")].tobytes() == H.jubjub_mul(H.asset_generator(R.A), 5)
    assert cmus[R.edge("empty")].tobytes() == cmus[R.edge("cancels")].tobytes() != bytes(32)
    assert status[R.edge("min alone")] == 2 and status[R.edge("min next to a bad identifier")] == 1
    assert status[R.edge("a bad identifier next to min")] == 1
    assert gens[R.edge("order 1")].tobytes() == gens[R.edge("order 2")].tobytes() != bytes(32)
    assert cmus[R.edge("order 1")].tobytes() == cmus[R.edge("order 2")].tobytes()
    assert gens[R.edge("bit 255")][31] & 0x80
    assert [status[R.edge(n)] for n in ("bad first", "bad middle", "bad last")] == [1, 1, 1]
    assert not gens[status != 0].any() and not cmus[status != 0].any()


def test_random_batch_against_the_reference_and_threads():
    convs, want = R.references("random130")
    arrays = R.arrays(convs)
    one = H.allowed_conversions(*arrays, threads=1)
    R.check(one, want)
    _same(H.allowed_conversions(*arrays, threads=4), one)
    status, gens, cmus = H.allowed_conversions(*arrays, threads=4, want_generators=False)
    assert gens is None
    _same((status, cmus), (one[0], one[2]))


def test_against_allowed_conversion_one_by_one():
    convs, want = R.references("random130")
    status, gens, cmus = H.allowed_conversions(*R.arrays(convs), threads=4)
    seen = 0
    for terms, s, g, c in zip(convs, status, gens, cmus):
        if s == 0 and len(set(i for i, _ in terms)) == len(terms) and all(v for _, v in terms):   # (nothing for __init__ to merge or drop)
            conv = H.AllowedConversion(sorted(terms))
            assert conv.generator == g.tobytes() and conv.cmu() == c.tobytes()
            seen += 1
    assert seen >= 30
    with pytest.raises(ValueError):
        H.AllowedConversion([(R.A, R.I128_MIN)])


def test_argument_errors():
    L = H.load_library()
    off, ids, vals = R.arrays([[(R.A, 1)], [(R.B, 2), (R.A, 3)]])
    out = [np.zeros(2, np.uint8), np.full((2, 32), 0xee, np.uint8), np.full((2, 32), 0xee, np.uint8)]
    p = [a.ctypes.data_as(C.c_void_p) for a in (off, ids, vals, *out)]
    call = lambda n, o, t, i, v, s, g, c: L.masp_host_allowed_conversions(n, o, t, i, v, s, g, c, 2)
    assert call(0, None, 0, None, None, None, None, None) == 0                      # no conversions: nothing is read
    assert call(2, p[0], 3, p[1], p[2], p[3], None, p[5]) == 0                      # generators_out may be NULL
    assert (out[1] == 0xee).all() and not (out[2] == 0xee).all()
    out[2][:] = 0xee
    for k in (0, 1, 2, 3, 5):
        q = [None if i == k else x for i, x in enumerate(p)]
        assert call(2, q[0], 3, *q[1:]) == 1, k
    for bad in ([1, 1, 3], [0, 2, 1], [0, 1, 2], [0, 4, 3]):                       # not from 0, decreasing, not to n_terms
        o = np.array(bad, np.uint64)
        assert call(2, o.ctypes.data_as(C.c_void_p), 3, *p[1:]) == 1, bad
    assert call((1 << 22) + 1, *p[:1], 3, *p[1:]) == 1
    assert (out[1] == 0xee).all() and (out[2] == 0xee).all()                        # nothing was written by the refused calls
    empty = np.zeros(4, np.uint64)                                                   # three conversions without terms: the arrays may be NULL
    st, g, c = np.zeros(3, np.uint8), np.zeros((3, 32), np.uint8), np.zeros((3, 32), np.uint8)
    assert call(3, empty.ctypes.data_as(C.c_void_p), 0, None, None, *[a.ctypes.data_as(C.c_void_p) for a in (st, g, c)]) == 0
    assert [x.tobytes() for x in g] == [H.JUBJUB_IDENTITY] * 3
    with pytest.raises(ValueError):
        H.allowed_conversions([0, 1], bytes(32), [1, 2])


def test_write_read_round_trip():
    conv = AllowedConversion([(R.B, -(1 << 100)), (R.A, 5), (R.C3, 1 << 64)])
    blob = conv.write()
    assert blob[0] == 3 and len(blob) == 1 + 3 * 48 + 32 and blob[-32:] == conv.generator
    assert blob[1:33] == min(R.A, R.B, R.C3)                                        # identifier order
    for back in (AllowedConversion.read(blob), AllowedConversion.read_unchecked(blob)):
        assert back.assets == conv.assets and back.generator == conv.generator and back.cmu() == conv.cmu() and back.write() == blob
    empty = AllowedConversion([])
    assert empty.write() == b"\x00" + H.JUBJUB_IDENTITY and AllowedConversion.read(empty.write()).assets == {}
    # the pairs are summed as I128Sum::read sums them: a repeated identifier merges
    twice = b"\x02" + R.A + (3).to_bytes(16, "little") + R.A + (4).to_bytes(16, "little") + AllowedConversion([(R.A, 7)]).generator
    assert AllowedConversion.read(twice).assets == {R.A: 7}


def test_read_refuses_what_the_reference_refuses():
    conv = AllowedConversion([(R.A, 5), (R.B, -6)])
    blob = conv.write()
    other = AllowedConversion([(R.A, 5), (R.B, -7)]).generator                      # another valid point
    with pytest.raises(ValueError):
        AllowedConversion.read(blob[:-32] + other)
    assert AllowedConversion.read_unchecked(blob[:-32] + other).generator == other   # (believed)
    off_curve = next(k.to_bytes(32, "little") for k in range(2, 100) if H.load_library().masp_host_point_uv(k.to_bytes(32, "little"), bytes(64)))
    for read in (AllowedConversion.read, AllowedConversion.read_unchecked):
        with pytest.raises(ValueError):
            read(blob[:-32] + off_curve)
        with pytest.raises(ValueError):
            read(b"\x01" + R.BAD_ASSET + (1).to_bytes(16, "little") + H.JUBJUB_IDENTITY)
        with pytest.raises(ValueError):
            read(blob[:-1])
        with pytest.raises(ValueError):
            read(b"\xfd\x02\x00" + blob[1:])                                        # a CompactSize that is not canonical


def test_batch_on_the_host_and_its_merge():
    sums = [[(R.A, 5), (R.B, -6)], {R.A: 1 << 64}, [(R.A, 3), (R.A, (1 << 64) - 3)], [(R.A, 5), (R.A, -5)], [],
            [(R.BAD_ASSET, 1)], [(R.A, R.I128_MIN)], [(R.A, R.I128_MIN + 1), (R.A, -1), (R.BAD_ASSET, 2)]]
    got = batch.allowed_conversions(sums, ctx=None, threads=2)
    assert len(got) == len(sums)
    for s, g in zip(sums[:5], got[:5]):
        one = H.AllowedConversion(s)
        assert isinstance(g, AllowedConversion) and g.assets == one.assets and g.generator == one.generator and g.cmu() == one.cmu()
        assert g.commitment() == one.commitment()
    # merged BEFORE the 64-bit truncation, as AllowedConversion.__init__ does: 3 + (2^64 - 3) = 2^64 truncates to 0 ...
    assert got[2].generator == H.JUBJUB_IDENTITY and got[2].assets == {R.A: 1 << 64}
    # ... where the call itself, which sums the terms as given, adds [3] G and [2^64 - 3] G
    _, gens, _ = H.allowed_conversions([0, 2], R.A + R.A, [3, (1 << 64) - 3])
    assert gens[0].tobytes() == H.jubjub_mul(H.asset_generator(R.A), 1 << 64) != H.JUBJUB_IDENTITY
    assert [isinstance(g, ValueError) and g.status for g in got[5:]] == [1, 2, 1]
    assert batch.allowed_conversions([], ctx=None) == []
    assert convert.AllowedConversion is H.AllowedConversion


def test_batch_read_on_the_host():
    convs = [AllowedConversion([(R.A, 5), (R.B, -6)]), AllowedConversion([]), AllowedConversion([(R.C3, 1 << 90)])]
    blobs = [c.write() for c in convs]
    tampered = blobs[0][:-32] + convs[2].generator
    bad_id = b"\x01" + R.BAD_ASSET + (1).to_bytes(16, "little") + H.JUBJUB_IDENTITY
    got = batch.read_allowed_conversions(blobs + [tampered, bad_id, blobs[2][:-3]], ctx=None)
    for c, g in zip(convs, got[:3]):
        assert g.assets == c.assets and g.generator == c.generator and g.cmu() == c.cmu()
    assert all(isinstance(g, ValueError) for g in got[3:]) and len(got) == 6
    assert batch.read_allowed_conversions([], ctx=None) == []


@pytest.fixture(scope="module")
def small_tree():
    sums = [[(R.ASSETS[k], 1 + k), (R.ASSETS[k + 1], -(2 + k))] for k in range(5)]
    convs = batch.allowed_conversions(sums, ctx=None)
    return sums, convs, batch.conversion_tree(convs, ctx=None)


def test_conversion_tree_against_the_leaves_one_by_one(small_tree):
    sums, convs, tree = small_tree
    assert tree.size() == 5
    assert tree.root() == FrozenCommitmentTree([H.AllowedConversion(s).commitment() for s in sums]).root()


def test_the_convert_circuit_judges_the_leaf(small_tree):
    """The circuit hashes the generator into the leaf itself and walks the path: it is satisfied, with the tree's root as its anchor
    input, only if the batch call's cmu is the leaf the circuit computes."""
    _, convs, tree = small_tree
    for pos in (0, 3, 4):
        path = tree.path(pos)
        inputs, _, _ = H.convert_assignment(convs[pos].generator, 1000 + pos, tree.root(), path.siblings, pos, 77 + pos, check=True)
        assert inputs[3].tobytes() == tree.root()
        assert path.root(convs[pos].cmu()) == tree.root()
    with pytest.raises(H.HostError):                     # ... and not with another conversion's generator
        H.convert_assignment(convs[1].generator, 5, tree.root(), tree.path(0).siblings, 0, 9, check=True)
