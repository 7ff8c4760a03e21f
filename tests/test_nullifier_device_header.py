"""masp_amd/csrc/device/nullifier.hpp compiled for the host (tests/native/nullifier_dev.hip): the fixed-base tables of G_ncr and G_nf
against the host's scalar multiplication, and the per-note steps and the whole note against nullifier_ref.  CPU only; bytes."""
import random

import numpy as np

import nullifier_ref as NR
import nullifier_shim as S
from masp_amd import host as H

RJ = H.JUBJUB_ORDER


def _scalars(windows, top):
    """0 and 1, 15 and 16, one digit in the first and in the last window, every digit 15, the largest scalar in use, sixteen random ones"""
    rng = random.Random(windows)
    return [0, 1, 15, 16, 7, 9 << (4 * (windows - 1)), (1 << (4 * windows)) - 1, top] + [rng.randrange(top + 1) for _ in range(16)]


def test_g_ncr_table_products():
    # (every digit 15 is 2^252 - 1, past r_J - 1: the table serves it all the same)
    for k in _scalars(63, RJ - 1):
        assert S.table_mul(0, k) == H.jubjub_mul(NR.G_NCR, NR._le(k)), k


def test_g_nf_table_products():
    for k in _scalars(16, (1 << 64) - 1):
        assert S.table_mul(1, k) == H.jubjub_mul(NR.G_NF, NR._le(k)), k


def _check_trace(notes, want, tr):
    for note, w, t in zip(notes, want, tr):
        t = t.tobytes()
        msg, rcm, cm, rho, bad = t[:104], t[104:136], t[136:168], t[168:200], t[200:205]
        L = H.load_library()
        # each step wrote its own flag, whatever the others found
        assert bad[0] == (L.masp_host_asset_generator(note["asset"], bytes(32)) != 0)
        assert bad[1] == (L.masp_host_diversifier_base(note["d"], bytes(32)) != 0)
        assert bad[2] == (L.masp_host_point_uv(note["pk_d"], bytes(64)) != 0)
        assert bad[3] == (note["lead"] not in (1, 2) or (note["lead"] == 1 and int.from_bytes(note["rseed"], "little") >= RJ))
        assert bad[4] == (L.masp_host_point_uv(note["nk"], bytes(64)) != 0)
        if not bad[0]:
            assert msg[:32] == H.asset_generator(note["asset"])
        assert msg[32:40] == NR._le(note["value"], 8)
        if not bad[1]:
            assert msg[40:72] == H.diversifier_base(note["d"])
        assert msg[72:104] == note["pk_d"]
        if not bad[3]:
            assert rcm == (note["rseed"] if note["lead"] == 1 else H.sapling_rseed_scalar(note["rseed"], 4))
        if w[0] == 0:
            want_cm = H.jubjub_add(H.point_bytes(*H.pedersen_hash(-1, [(msg[i // 8] >> (i % 8)) & 1 for i in range(832)])), H.jubjub_mul(NR.G_NCR, rcm))
            assert cm == want_cm and NR._le(H.point_uv(cm)[0]) == w[1]
            assert rho == H.jubjub_add(cm, H.jubjub_mul(NR.G_NF, NR._le(note["position"])))


def test_steps_and_whole_note_on_the_edge_list():
    notes, want = NR.references("edges", NR.edge_notes)
    status, cmus, nfs, tr = S.steps_host(NR.arrays(notes), lanes=1, trace=True)
    NR.check((status, cmus, nfs), want)
    _check_trace(notes, want, tr)


def test_steps_on_every_status():
    notes = [n for control, spoiled, _ in NR.status_notes() for n in (control, spoiled)] + [n for n, _ in NR.double_notes()]
    want = [NR.reference(n) for n in notes]
    status, cmus, nfs, tr = S.steps_host(NR.arrays(notes), lanes=1, trace=True)
    NR.check((status, cmus, nfs), want)
    _check_trace(notes, want, tr)


def test_lane_shares_sum_to_the_same_bytes():
    notes, want = NR.references("edges", NR.edge_notes)
    for lanes in (8, 3, 64):
        NR.check(S.steps_host(NR.arrays(notes), lanes=lanes), want)


def test_host_twin_agrees_on_a_mixed_batch():
    notes, want = NR.references("random130", lambda: NR.random_batch(130, 9))
    got = S.steps_host(NR.arrays(notes), lanes=8)
    NR.check(got, want)
    for x, y in zip(got, H.note_nullifiers(*NR.arrays(notes), threads=2)):
        assert np.array_equal(x, y)
