"""Note::cmu and Note::nf on the host (masp_host_sapling_note_nullifiers, note_encryption.note_nf and batch.note_nullifiers with
ctx=None) against nullifier_ref's composition of vector-pinned primitives, and against the nullifier the Spend circuit's witness
synthesis computes and the oracle's R1CS evaluation pins.  CPU only; every comparison is of bytes."""
import numpy as np
import pytest

import nullifier_ref as NR
from masp_amd import host as H
from masp_amd import note_encryption as NE
from test_circuits import spend_instance


def test_reference_and_host_twin_against_the_spend_circuit():
    import masp_amd
    assert masp_amd.note_nf is NE.note_nf
    for seed in (1, 2, 3):
        inst, cmu, pk_d = spend_instance(seed, value=seed * 1000 + 7)
        _, _, _, _, nf = H.spend_assignment(check=True, **inst)
        nk = H.jubjub_mul(H.point_bytes(*H.generator_uv(0)), inst["nsk"])     # nk = [nsk] G_proof_generation_key
        note = dict(asset=inst["asset_identifier"], value=inst["value"], d=inst["diversifier"], pk_d=pk_d, lead=1, rseed=NR._le(inst["rcm"]),
                    nk=nk, position=inst["position"])
        assert NR.reference(note) == (0, cmu, nf)
        status, cmus, nfs = H.note_nullifiers(*NR.arrays([note]), threads=1)
        assert (int(status[0]), cmus[0].tobytes(), nfs[0].tobytes()) == (0, cmu, nf)
        assert NE.note_nf(*NR.as_items([note])[0]) == nf


def test_edge_list():
    notes, want = NR.references("edges", NR.edge_notes)
    assert [w[0] for w in want] == [0] * len(notes)
    NR.check(H.note_nullifiers(*NR.arrays(notes), threads=2), want)
    for item, w in zip(NR.as_items(notes), want):
        assert NE.note_nf(*item) == w[2]
        assert NE.note_cmu(item[0], item[1]) == w[1]


def test_uniqueness():
    base = NR.good_note(41)
    notes = [base, dict(base, position=base["position"] ^ 1), dict(base, nk=NR.random_point(__import__("random").Random(5))),
             dict(base, value=base["value"] ^ 1)]
    status, cmus, nfs = H.note_nullifiers(*NR.arrays(notes))
    NR.check((status, cmus, nfs), [NR.reference(n) for n in notes])
    cmus, nfs = [c.tobytes() for c in cmus], [f.tobytes() for f in nfs]
    assert nfs[1] != nfs[0] and cmus[1] == cmus[0]        # another position: another nullifier of the same commitment
    assert nfs[2] != nfs[0] and cmus[2] == cmus[0]        # another nk
    assert cmus[3] != cmus[0] and nfs[3] != nfs[0]        # another value


def test_every_status_next_to_its_control():
    cases = NR.status_notes()
    for control, spoiled, s in cases:
        assert sum(1 for f in NR.FIELDS if control[f] != spoiled[f]) == 1
        assert NR.status_of(control) == 0 and NR.status_of(spoiled) == s
    notes = [n for control, spoiled, _ in cases for n in (control, spoiled)] + [n for n, _ in NR.double_notes()]
    want = [NR.reference(n) for n in notes]
    assert [w[0] for w in want[-3:]] == [s for _, s in NR.double_notes()]
    assert sorted(set(w[0] for w in want)) == [0, 1, 2, 3, 4, 5]
    NR.check(H.note_nullifiers(*NR.arrays(notes), threads=1), want)
    for (control, spoiled, s), item in zip(cases, NR.as_items([c[1] for c in cases])):
        with pytest.raises(ValueError, match=NE.NULLIFIER_STATUS[s][:12]):
            NE.note_nf(*item)


def test_a_bad_note_between_two_good_ones():
    a, b = NR.good_note(51), NR.good_note(52)
    alone = H.note_nullifiers(*NR.arrays([a, b]))
    for s in (1, 2, 3, 4, 5):
        status, cmus, nfs = H.note_nullifiers(*NR.arrays([a, NR.spoil(NR.good_note(53), s), b]))
        assert status.tolist() == [0, s, 0]
        assert not cmus[1].any() and not nfs[1].any()
        assert np.array_equal(cmus[[0, 2]], alone[1]) and np.array_equal(nfs[[0, 2]], alone[2])
    got = NE.batch.note_nullifiers(NR.as_items([a, NR.spoil(a, 3), b]), None)
    assert got[1] is None and got[0] == (alone[1][0].tobytes(), alone[2][0].tobytes()) and got[2] == (alone[1][1].tobytes(), alone[2][1].tobytes())


def test_threads_and_sizes():
    notes, want = NR.references("random130", lambda: NR.random_batch(130, 9))
    assert 0 < sum(1 for w in want if w[0]) < 130
    one = H.note_nullifiers(*NR.arrays(notes), threads=1)
    four = H.note_nullifiers(*NR.arrays(notes), threads=4)
    NR.check(one, want)
    for x, y in zip(one, four):
        assert np.array_equal(x, y)
    status, cmus, nfs = H.note_nullifiers(*NR.arrays(notes), threads=4, want_cmus=False)
    assert cmus is None and np.array_equal(nfs, one[2]) and np.array_equal(status, one[0])


def test_no_notes():
    status, cmus, nfs = H.note_nullifiers(*NR.arrays([]))
    assert status.shape == (0,) and cmus.shape == (0, 32) and nfs.shape == (0, 32)
    null = [None] * 11
    assert H.load_library().masp_host_sapling_note_nullifiers(0, *null, 4) == 0
    assert H.load_library().masp_host_sapling_note_nullifiers(1, *null, 4) == 1     # MASP_HOST_E_INVALID: a NULL array with n > 0
    assert NE.batch.note_nullifiers([], None) == []
