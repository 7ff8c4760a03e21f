"""Nullifiers and note commitments on the GPU (masp_hip_sapling_note_nullifiers, k_nullifier.hip) through the C ABI, against the host
twin (masp_host_sapling_note_nullifiers) and nullifier_ref's composition of vector-pinned primitives; the product's kernels for both lane
widths through the test-side shim.  Every comparison is of bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import compact_notes as CN
import masp_amd
import nullifier_ref as NR
import nullifier_shim as S
from masp_amd import host as H
from masp_amd import note_encryption as NE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def _same(got, want):
    for x, y in zip(got, want):
        assert (x is None and y is None) or np.array_equal(x, y)


def test_sizes_against_the_host_twin(ctx):
    notes, want = NR.references("random130", lambda: NR.random_batch(130, 9))
    assert 0 < sum(1 for w in want if w[0]) < 130
    for n in (0, 1, 7, 9, 63, 64, 65, 130):
        arrays = NR.arrays(notes[:n])
        host = H.note_nullifiers(*arrays, threads=4)
        got = ctx.note_nullifiers(*arrays)
        _same(got, host)
        NR.check(got, want[:n])
        status, cmus, nfs = ctx.note_nullifiers(*arrays, want_cmus=False)      # cmus_out = NULL
        assert cmus is None
        _same((status, nfs), (host[0], host[2]))


def test_arguments(ctx):
    L, h = ctx._L, ctx._h
    null = [None] * 11
    assert L.masp_hip_sapling_note_nullifiers(h, 0, *null) == 0                 # no notes: nothing is read
    assert L.masp_hip_sapling_note_nullifiers(h, 1, *null) == 1                 # MASP_HIP_E_INVALID_ARG
    arrays = NR.arrays([NR.good_note(1)])
    out = [np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8)]
    p = [a.ctypes.data_as(C.c_void_p) for a in list(arrays) + out]
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):                                   # every array but cmus_out
        assert L.masp_hip_sapling_note_nullifiers(h, 1, *[None if i == k else x for i, x in enumerate(p)]) == 1, k
    assert L.masp_hip_sapling_note_nullifiers(h, (1 << 22) + 1, *p) == 1
    with pytest.raises(masp_amd.MaspHipError):
        ctx.note_nullifiers_configure(4)
    assert NE.batch.note_nullifiers([], ctx) == []


def test_edge_list(ctx):
    notes, want = NR.references("edges", NR.edge_notes)
    NR.check(ctx.note_nullifiers(*NR.arrays(notes)), want)


def test_uniqueness(ctx):
    base = NR.good_note(41)
    notes = [base, dict(base, position=base["position"] ^ 1), dict(base, nk=NR.random_point(random.Random(5))), dict(base, value=base["value"] ^ 1)]
    status, cmus, nfs = ctx.note_nullifiers(*NR.arrays(notes))
    NR.check((status, cmus, nfs), [NR.reference(n) for n in notes])
    cmus, nfs = [c.tobytes() for c in cmus], [f.tobytes() for f in nfs]
    assert nfs[1] != nfs[0] and cmus[1] == cmus[0]        # another position: another nullifier of the same commitment
    assert nfs[2] != nfs[0] and cmus[2] == cmus[0]        # another nk
    assert cmus[3] != cmus[0] and nfs[3] != nfs[0]        # another value


def test_every_status_next_to_its_control(ctx):
    notes = [n for control, spoiled, _ in NR.status_notes() for n in (control, spoiled)] + [n for n, _ in NR.double_notes()]
    want = [NR.reference(n) for n in notes]
    assert sorted(set(w[0] for w in want)) == [0, 1, 2, 3, 4, 5]
    NR.check(ctx.note_nullifiers(*NR.arrays(notes)), want)


def test_a_bad_note_between_two_good_ones(ctx):
    a, b = NR.good_note(51), NR.good_note(52)
    alone = ctx.note_nullifiers(*NR.arrays([a, b]))
    NR.check(alone, [NR.reference(a), NR.reference(b)])
    for s in (1, 2, 3, 4, 5):
        status, cmus, nfs = ctx.note_nullifiers(*NR.arrays([a, NR.spoil(NR.good_note(53), s), b]))
        assert status.tolist() == [0, s, 0]
        assert not cmus[1].any() and not nfs[1].any()
        assert np.array_equal(cmus[[0, 2]], alone[1]) and np.array_equal(nfs[[0, 2]], alone[2])


def test_a_thousand_notes_one_in_ten_invalid(ctx):
    notes = NR.random_batch(1000, 77)
    arrays = NR.arrays(notes)
    host = H.note_nullifiers(*arrays)
    bad = sorted(set(host[0].tolist()))
    assert bad == [0, 1, 2, 3, 4, 5] and 50 < int((host[0] != 0).sum()) < 200
    first = ctx.note_nullifiers(*arrays)
    _same(first, host)
    _same(ctx.note_nullifiers(*arrays), first)            # the same call twice: the same bytes
    for lanes in (1, 8):                                   # ... and whichever lane width the call is told to use
        ctx.note_nullifiers_configure(lanes)
        try:
            _same(ctx.note_nullifiers(*arrays), first)
        finally:
            ctx.note_nullifiers_configure(0)


@pytest.mark.parametrize("n", [1, 7, 9, 65])
def test_both_lane_widths_give_the_same_bytes(n):
    notes, want = NR.references("random130", lambda: NR.random_batch(130, 9))
    arrays = NR.arrays(notes[3:3 + n])
    one, eight = S.run_gpu(arrays, 1), S.run_gpu(arrays, 8)
    _same(one, eight)
    NR.check(one, want[3:3 + n])


def test_from_compact_outputs_to_nullifiers(ctx):
    """64 compact outputs, 8 of them notes of two ivks -> the compact scan -> positions behind a tree of 5 leaves -> the nullifiers"""
    rng = random.Random(31)
    ivks_int = [rng.randrange(1, CN.RJ) for _ in range(2)]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    nks = [NR.random_point(rng) for _ in range(2)]
    epks, cmus, encs = CN.noise(64, 31)
    places = [2, 9, 17, 30, 31, 40, 55, 63]
    for j, o in enumerate(places):
        out, _, _ = CN.planted(ivks_int[j % 2], 3100 + j)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
    outs = [NE.CompactShieldedOutput(e.tobytes(), c.tobytes(), x[:84].tobytes()) for e, c, x in zip(epks, cmus, encs)]
    found = NE.batch.try_compact_note_decryption(ivks, outs, ctx)
    assert [o for o, f in enumerate(found) if f is not None] == places
    tree_size = 5
    items = [(f[0][0], f[0][1], nks[f[1]], tree_size + o) for o, f in enumerate(found) if f is not None]
    got = NE.batch.note_nullifiers(items, ctx)
    assert len(got) == 8 and len(set(nf for _, nf in got)) == 8
    for o, item, (cmu, nf) in zip(places, items, got):
        assert cmu == outs[o].cmu
        assert nf == NE.note_nf(*item)
    assert got == NE.batch.note_nullifiers(items, None)
