"""Compact (ZIP 307) trial decryption of Sapling notes on the host (libmasp_host.so: masp_host_sapling_try_compact_note_decryption and its
batch form) against the reference's ten vectors, the full path, and one near miss per refusal.  Every comparison is of bytes."""
import random

import numpy as np
import pytest

import compact_notes as CN
from masp_amd import host as H
from masp_amd import note_encryption as NE

VECTORS, ASSET, RJ = CN.VECTORS, CN.ASSET, CN.RJ


@pytest.mark.parametrize("i", range(10))
def test_vector(i):
    tv = VECTORS[i]
    out = NE.CompactShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"][:84])
    assert NE.compact_output(NE.ShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"])) == out
    note = NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"]))
    assert NE.try_sapling_compact_note_decryption(tv["ivk"], out, lead_byte=1) == (note, NE.PaymentAddress(tv["default_d"], tv["default_pk_d"]))
    assert H.sapling_try_compact_note_decryption(tv["ivk"], tv["epk"], tv["cmu"], tv["c_enc"][:84], 1) == (tv["p_enc"][:84], tv["default_pk_d"])
    assert NE.try_sapling_compact_note_decryption(tv["ivk"], out, lead_byte=2) is None
    assert NE.try_sapling_compact_note_decryption(VECTORS[(i + 1) % 10]["ivk"], out, lead_byte=1) is None
    with pytest.raises(H.HostError):
        NE.try_sapling_compact_note_decryption(RJ, out, lead_byte=1)                  # not a SaplingIvk


def test_agreement_with_the_full_path():
    rng = random.Random(61)
    for k in range(6):
        ivk, lead = (rng.randrange(1, RJ) if k else RJ - 1), 1 + k % 2
        out, note, to = CN.planted(ivk, 6100 + k, lead)
        full = NE.try_sapling_note_decryption(ivk, out, lead_byte=lead)
        assert full is not None and full[:2] == (note, to)
        assert NE.try_sapling_compact_note_decryption(ivk, NE.compact_output(out), lead_byte=lead) == full[:2]
        assert NE.try_sapling_compact_note_decryption(ivk, NE.compact_output(out), lead_byte=3 - lead) is None
        assert NE.try_sapling_compact_note_decryption(ivk % (RJ - 1) + 1, NE.compact_output(out), lead_byte=lead) is None


def test_one_near_miss_per_refusal():
    ivk = random.Random(62).randrange(1, RJ)
    seen = set()
    for name, out, lead, k in CN.near_misses(ivk, 62):
        got = NE.try_sapling_compact_note_decryption(k, NE.compact_output(out), lead_byte=lead)
        assert (got is not None) == (name == "honest"), (name, lead)
        if name == "honest":       # ... and a lead byte other than the argument
            assert NE.try_sapling_compact_note_decryption(k, NE.compact_output(out), lead_byte=3 - lead) is None
        seen.add(name)
    assert seen == {"honest", "cmu bit", "asset identifier", "diversifier", "esk", "rcm", "ivk zero", "epk"}
    # the esk near miss passes everything but the last check: the same note is accepted once the check is not made (lead byte 1 has none),
    # and its full form is refused too
    name, out, lead, k = next(m for m in CN.near_misses(ivk, 62) if m[0] == "esk")
    assert NE.try_sapling_note_decryption(k, out, lead_byte=2) is None


def _single(ivks, epks, cmus, encs, lead):
    """the single form over every pair: (per output the first ivk that succeeds with its result, the candidate count by the definition)"""
    res, cand = [], 0
    for e, c, x in zip(epks, cmus, encs):
        first = None
        for k, ivk in enumerate(ivks):
            r = H.sapling_try_compact_note_decryption(ivk, e.tobytes(), c.tobytes(), x.tobytes(), lead)
            if r is not None and first is None:
                first = (k, r)
            if H.load_library().masp_host_point_uv(e.tobytes(), bytes(64)) == 0:
                key = H.kdf_sapling(H.sapling_ka_agree(ivk, e.tobytes()), e.tobytes())
                cand += (x[0] ^ CN.pynote.chacha20_block(key, 1, CN.NONCE)[0]) == lead
        res.append(first)
    return res, cand


def test_batch_against_single():
    rng = random.Random(63)
    ivks_int = [0, rng.randrange(1, RJ), RJ - 1, rng.randrange(1, RJ)]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    rows = [m[1] for m in CN.near_misses(ivks_int[1], 63)] + CN.small_order_rows(ivks_int[3], 6300)
    rows += [CN.planted(ivks_int[2], 6310)[0], CN.planted(ivks_int[3], 6311, 1)[0]]
    epks, cmus, encs = CN.rows_to_arrays(rows)
    ne, nc, nx = CN.noise(150, 63)
    epks, cmus, encs = np.concatenate([epks, ne]), np.concatenate([cmus, nc]), np.concatenate([encs, nx])[:, :84].copy()
    for lead in (1, 2):
        want, want_cand = _single(ivks, epks, cmus, encs, lead)
        for threads in (1, 3):
            hit, pts, pks, cand = H.sapling_try_compact_note_decryption_batch(ivks, epks, cmus, encs, lead_byte=lead, threads=threads)
            got = [None if k < 0 else (int(k), (pts[o].tobytes(), pks[o].tobytes())) for o, k in enumerate(hit.tolist())]
            assert got == want and cand == want_cand
        assert sum(w is not None for w in want) >= 2 and want_cand > sum(w is not None for w in want)
    with pytest.raises(H.HostError):
        H.sapling_try_compact_note_decryption_batch([RJ.to_bytes(32, "little")], epks, cmus, encs)
