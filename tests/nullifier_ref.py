"""The nullifier tests' other side and their shared inputs.  `reference` composes Note::cmu and Note::nf from one-call primitives that
the reference's vectors pin (tests/test_circuits.py) and hashlib: it goes through none of the code under test.  The cases (the edge
list, one bad note per status, random batches) are computed once and shared by the host, the device-header and the GPU file."""
import hashlib
import random

import numpy as np

import pynote
from masp_amd import host as H

RJ = H.JUBJUB_ORDER
G_NCR = H.point_bytes(*H.generator_uv(1))     # note_commitment_randomness
G_NF = H.point_bytes(*H.generator_uv(2))      # nullifier_position
ASSET = H.asset_identifier(b"benchmark")
FIELDS = ("asset", "value", "d", "pk_d", "lead", "rseed", "nk", "position")


def _le(k, n=32):
    return int(k).to_bytes(n, "little")


def status_of(note):
    """the status the semantics give a note, from the one-call primitives"""
    L = H.load_library()
    if L.masp_host_asset_generator(note["asset"], bytes(32)) != 0:
        return 1
    if L.masp_host_diversifier_base(note["d"], bytes(32)) != 0:
        return 2
    if L.masp_host_point_uv(note["pk_d"], bytes(64)) != 0:
        return 3
    if note["lead"] not in (1, 2) or (note["lead"] == 1 and int.from_bytes(note["rseed"], "little") >= RJ):
        return 4
    if L.masp_host_point_uv(note["nk"], bytes(64)) != 0:
        return 5
    return 0


def reference(note):
    """-> (status, cmu, nf); the outputs are zeros where the status is not 0"""
    s = status_of(note)
    if s:
        return s, bytes(32), bytes(32)
    g, gd = H.asset_generator(note["asset"]), H.diversifier_base(note["d"])
    rcm = note["rseed"] if note["lead"] == 1 else pynote.rseed_scalar(note["rseed"], 4)
    msg = g + _le(note["value"], 8) + gd + note["pk_d"]
    bits = [(msg[i // 8] >> (i % 8)) & 1 for i in range(8 * len(msg))]
    cm = H.jubjub_add(H.point_bytes(*H.pedersen_hash(-1, bits)), H.jubjub_mul(G_NCR, rcm))
    rho = H.jubjub_add(cm, H.jubjub_mul(G_NF, _le(note["position"])))
    return 0, _le(H.point_uv(cm)[0]), hashlib.blake2s(note["nk"] + rho, person=b"MASP__nf").digest()


def random_point(rng):
    """a point of the prime-order subgroup, as a pk_d or an nk is"""
    return H.jubjub_mul(G_NCR, _le(rng.randrange(1, RJ)))


def good_note(seed, lead=None):
    rng = random.Random(seed)
    while True:
        d = rng.randbytes(11)
        if H.load_library().masp_host_diversifier_base(d, bytes(32)) == 0:
            break
    lead = lead if lead is not None else rng.choice((1, 2))
    return dict(asset=ASSET, value=rng.randrange(1 << 64), d=d, pk_d=random_point(rng), lead=lead,
                rseed=_le(rng.randrange(RJ)) if lead == 1 else rng.randbytes(32), nk=random_point(rng), position=rng.randrange(1 << 64))


def _first(cands, bad):
    return next(c for c in cands if bad(c))


def _no_point(b):
    return H.load_library().masp_host_point_uv(b, bytes(64)) != 0


BAD_ASSET = _first((bytes([i]) * 32 for i in range(256)), lambda a: H.load_library().masp_host_asset_generator(a, bytes(32)) != 0)
BAD_D = _first((bytes([i]) * 11 for i in range(256)), lambda d: H.load_library().masp_host_diversifier_base(d, bytes(32)) != 0)
OFF_CURVE = _first((_le(v) for v in range(2, 100)), _no_point)
NOT_CANONICAL = _le(H.FR_MODULUS + 5)     # (its low 255 bits are not below the field modulus)
NEGATIVE_ZERO = _le(1 | (1 << 255))       # u = 0 with the sign bit set


def spoil(note, status, variant=0):
    """the note with the one field changed that gives it `status`"""
    if status == 1:
        return dict(note, asset=BAD_ASSET)
    if status == 2:
        return dict(note, d=BAD_D)
    if status == 3:
        return dict(note, pk_d=(OFF_CURVE, NOT_CANONICAL, NEGATIVE_ZERO)[variant % 3])
    if status == 4:
        return (dict(note, lead=1, rseed=_le(RJ)), dict(note, lead=1, rseed=_le((1 << 256) - 1)), dict(note, lead=0), dict(note, lead=3),
                dict(note, lead=255))[variant % 5]
    return dict(note, nk=(OFF_CURVE, NOT_CANONICAL, NEGATIVE_ZERO)[variant % 3])


def edge_notes():
    """the issue's edge list: every position and value on one note of either lead byte, the three rcm and three rseeds"""
    out = []
    for lead in (1, 2):
        base = good_note(700 + lead, lead)
        for pos in (0, 1, 15, 16, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 0xf0f0f0f0f0f0f0f0):
            out.append(dict(base, position=pos))
        for value in (0, 1, (1 << 64) - 1):
            out.append(dict(base, value=value))
    base = good_note(703, 1)
    for rcm in (0, 1, RJ - 1):
        out.append(dict(base, rseed=_le(rcm)))
    for k in range(3):
        out.append(good_note(710 + k, 2))
    return out


def status_notes():
    """[(control, spoiled, status)]: every status, every way to it, next to the note that differs in that one field"""
    out = []
    for s, variants in ((1, 1), (2, 1), (3, 3), (4, 5), (5, 3)):
        for v in range(variants):
            base = good_note(800 + 10 * s + v, 1 if s == 4 and v < 2 else None)   # (rcm is a lead-byte-1 note's field)
            out.append((base, spoil(base, s, v), s))
    return out


def double_notes():
    """[(spoiled, status)]: two checks fail, the first in the order counts"""
    base = good_note(899)
    return [(spoil(spoil(base, 5), 2), 2), (spoil(spoil(base, 4, 2), 3), 3), (spoil(spoil(base, 1), 5), 1)]


def random_batch(n, seed, bad_share=0.1):
    """n notes, about bad_share of them spoiled in a random field"""
    rng = random.Random(seed)
    notes = []
    for i in range(n):
        note = good_note(seed * 100000 + i)
        if rng.random() < bad_share:
            note = spoil(note, rng.randrange(1, 6), rng.randrange(15))
        notes.append(note)
    return notes


def arrays(notes):
    """the eight arrays of either note_nullifiers call"""
    cat = lambda f, w: np.frombuffer(b"".join(n[f] for n in notes), np.uint8).reshape(len(notes), w).copy()
    return (cat("asset", 32), np.array([n["value"] for n in notes], np.uint64), cat("d", 11), cat("pk_d", 32),
            np.array([n["lead"] for n in notes], np.uint8), cat("rseed", 32), cat("nk", 32), np.array([n["position"] for n in notes], np.uint64))


def as_items(notes):
    """the notes as note_encryption's (Note, PaymentAddress, nk, position)"""
    from masp_amd import note_encryption as NE
    return [(NE.Note(n["asset"], n["value"], n["pk_d"], NE.Rseed(n["lead"], n["rseed"])), NE.PaymentAddress(n["d"], n["pk_d"]), n["nk"], n["position"])
            for n in notes]


_cache = {}


def references(name, make):
    """(notes, [reference(note)]) of a named list, computed once"""
    if name not in _cache:
        notes = make()
        _cache[name] = (notes, [reference(n) for n in notes])
    return _cache[name]


def check(got, want):
    """got: (status, cmus or None, nfs) arrays; want: [reference(note)]"""
    status, cmus, nfs = got
    assert status.tolist() == [w[0] for w in want]
    if cmus is not None:
        assert [c.tobytes() for c in cmus] == [w[1] for w in want]
    assert [f.tobytes() for f in nfs] == [w[2] for w in want]
