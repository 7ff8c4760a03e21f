"""Inputs of the compact (ZIP 307) note decryption tests, shared by the host and the GPU file: planted notes, noise, and one near miss
per refusal of the reference's check.  Everything is built as a FULL output (epk, cmu, enc_ciphertext[612]); the compact form takes
enc_ciphertext[:84]."""
import json
import os
import random

import numpy as np

import pynote
from masp_amd import host as H
from masp_amd import note_encryption as NE

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "note_encryption_vectors.json")))
VECTORS = [{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in tv.items()} for tv in DOC["vectors"]]
ASSET = bytes.fromhex(DOC["asset_identifier"])
RJ = H.JUBJUB_ORDER
NONCE = bytes(12)
IDENTITY = (1).to_bytes(32, "little")
ORDER2 = (H.FR_MODULUS - 1).to_bytes(32, "little")


def _le(k):
    return k.to_bytes(32, "little")


def no_gd(d):
    try:
        H.diversifier_base(d)
        return False
    except H.HostError:
        return True


def recipient(ivk, seed):
    """a diversifier with a g_d and pk_d = [ivk] g_d"""
    rng = random.Random(seed)
    while True:
        d = rng.randbytes(11)
        if not no_gd(d):
            return NE.PaymentAddress(d, H.jubjub_mul(H.diversifier_base(d), _le(ivk)))


def planted(ivk, seed, lead_byte=2):
    """-> (ShieldedOutput, Note, PaymentAddress) of a note of ivk"""
    rng = random.Random(seed)
    to = recipient(ivk, seed)
    if lead_byte == 2:
        note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(2, rng.randbytes(32)))
        return NE.sapling_note_encrypt(note, to, rng.randbytes(512)), note, to
    note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(1, _le(rng.randrange(RJ))))
    return NE.sapling_note_encrypt(note, to, rng.randbytes(512), esk=_le(rng.randrange(1, RJ))), note, to


def noise(n, seed):
    """n outputs of random bytes: about half of the epks decode"""
    rng = np.random.default_rng(seed)
    epks = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    epks[:, 31] &= 0x7f | (rng.integers(0, 2, n, dtype=np.uint8) << 7)
    epks[:, 31] &= 0xbf        # v below 2^254: mostly canonical
    return epks, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 612), dtype=np.uint8)


def rows_to_arrays(rows):
    return tuple(np.frombuffer(b"".join(bytes(r[f]) for r in rows), np.uint8).reshape(len(rows), -1).copy() for f in range(3))


def _reencrypt(ivk, out, plaintext):
    """the output with another plaintext under the key ivk derives for its epk"""
    key = H.kdf_sapling(H.sapling_ka_agree(_le(ivk), out.epk), out.epk)
    ct, tag = pynote.aead_encrypt(key, NONCE, plaintext)
    return NE.ShieldedOutput(out.epk, out.cmu, ct + tag)


def near_misses(ivk, seed):
    """[(name, ShieldedOutput, the lead byte it is a near miss for, the ivk it is one for)]: each differs from an honest note of ivk
    in the one thing its name says"""
    rng = random.Random(seed)
    res = []
    bad_asset = next(a for a in (bytes([i]) * 32 for i in range(256)) if H.load_library().masp_host_asset_generator(a, bytes(32)) != 0)
    bad_d = next(d for d in (bytes([i]) * 11 for i in range(256)) if no_gd(d))
    for lead in (1, 2):
        out, note, to = planted(ivk, seed * 10 + lead, lead)
        pt = NE.note_plaintext_bytes(note, to)
        honest = _reencrypt(ivk, out, pt)          # (the planted note with an empty memo: the base of the edits below)
        res.append(("honest", honest, lead, ivk))
        cmu = bytearray(out.cmu)
        cmu[rng.randrange(31)] ^= 1 << rng.randrange(8)
        res.append(("cmu bit", honest._replace(cmu=bytes(cmu)), lead, ivk))
        res.append(("asset identifier", _reencrypt(ivk, out, pt[:20] + bad_asset + pt[52:]), lead, ivk))
        res.append(("diversifier", _reencrypt(ivk, out, pt[:1] + bad_d + pt[12:]), lead, ivk))
    # lead byte 2 under an esk other than the derived one: the commitment is right, the epk check fails
    out, note, to = planted(ivk, seed * 10 + 3, 2)
    res.append(("esk", NE.sapling_note_encrypt(note, to, esk=_le(rng.randrange(1, RJ))), 2, ivk))
    # lead byte 1 with rcm >= r_J
    out, note, to = planted(ivk, seed * 10 + 4, 1)
    pt = NE.note_plaintext_bytes(note, to)
    for rcm in (RJ, (1 << 256) - 1):
        res.append(("rcm", _reencrypt(ivk, out, pt[:52] + _le(rcm) + pt[84:]), 1, ivk))
    # ivk = 0: the shared secret is the identity whatever the epk, and pk_d = [0] g_d is the identity
    for lead in (1, 2):
        out, note, to = planted(ivk, seed * 10 + 5 + lead, lead)
        res.append(("ivk zero", _reencrypt(0, out, NE.note_plaintext_bytes(note, to)), lead, 0))
    # an epk that does not decode
    out, note, to = planted(ivk, seed * 10 + 8, 2)
    off_curve = next(v for v in range(2, 100) if H.load_library().masp_host_point_uv(_le(v), bytes(64)) != 0)
    for epk in (_le(H.FR_MODULUS + 5), _le(off_curve), _le(1 | (1 << 255))):
        res.append(("epk", out._replace(epk=epk), 2, ivk))
    return res


def small_order_rows(ivk, seed):
    """outputs whose epk has small order (the identity, the point of order 2): [8 k] epk is the identity for EVERY k, so one key serves
    every ivk and a plaintext with the right lead byte is a candidate for all of them"""
    rows = []
    for epk in (IDENTITY, ORDER2):
        for lead in (1, 2):
            _, note, to = planted(ivk, seed + lead, lead)
            ct, tag = pynote.aead_encrypt(pynote.kdf_sapling(IDENTITY, epk), NONCE, NE.note_plaintext_bytes(note, to))
            rows.append(NE.ShieldedOutput(epk, NE.note_cmu(note, to), ct + tag))
    return rows
