"""Sapling note encryption and trial decryption for MASP: the mirror of `masp_note_encryption` over
`masp_primitives::sapling::note_encryption::SaplingDomain`.

`sapling_note_encrypt` and `try_sapling_note_decryption` run on the host (libmasp_host.so); `batch.try_note_decryption` scans
outputs x ivks on the GPU (masp_hip_sapling_trial_decrypt: key agreement, KDF and the AEAD's tag for every pair) and finishes the pairs
whose tag verifies on the host (masp_host_sapling_finish_note_decryption: decryption, parsing, the commitment, the esk check).

The compact (ZIP 307) form, what a light wallet runs: a `CompactShieldedOutput` carries the first 84 bytes of enc_ciphertext (the note
without its memo) and no tag.  `try_sapling_compact_note_decryption` runs on the host; `batch.try_compact_note_decryption` runs the WHOLE
check on the GPU (masp_hip_sapling_compact_trial_decrypt: the lead byte for every pair, then parsing, group hashes, pk_d, the Pedersen
note commitment and the esk check for the pairs that pass it), so its hits are final and the host finishes nothing.

The sender's side: `encrypt_outgoing_plaintext` makes an output's out_ciphertext (pk_d | esk under the ock = PRF^ock(ovk, cv, cmu, epk)),
`try_sapling_output_recovery` and `try_sapling_output_recovery_with_ock` read an `OutputDescription` back on the host, and
`batch.try_output_recovery` scans outputs x ovks on the GPU (masp_hip_sapling_output_recovery_scan: PRF^ock and out_ciphertext's tag for
every pair) and finishes the pairs whose tag verifies on the host (masp_host_sapling_try_output_recovery_with_ock: everything else).

Once a note is the wallet's: `note_nf` is Note::nf(&nk, position) on the host, and `batch.note_nullifiers` computes the commitments and
nullifiers of a list of notes on the GPU (masp_hip_sapling_note_nullifiers) or on host threads.

Making outputs: `batch.build_outputs` turns output plans into `OutputDescription`s without their proofs, cv, cmu, epk and the two
ciphertexts, on the GPU (masp_hip_sapling_build_outputs) or on host threads.  Making spends: `batch.build_spends` turns spend plans into
what the builder puts around a Spend proof, cv, rk and nf with cmu and nk, on the GPU (masp_hip_sapling_build_spends) or on host threads."""
import os
from collections import namedtuple

import numpy as np

from . import host as H

NOTE_PLAINTEXT_SIZE = H.NOTE_PLAINTEXT_SIZE
ENC_CIPHERTEXT_SIZE = H.ENC_CIPHERTEXT_SIZE
MEMO_SIZE = 512

PaymentAddress = namedtuple("PaymentAddress", "diversifier pk_d")             # 11 bytes, 32 bytes
Rseed = namedtuple("Rseed", "lead_byte bytes")                                # 1: BeforeZip212(rcm), 2: AfterZip212(rseed)
Note = namedtuple("Note", "asset_identifier value pk_d rseed")                # 32 bytes, int, 32 bytes, Rseed
ShieldedOutput = namedtuple("ShieldedOutput", "epk cmu enc_ciphertext")       # ephemeral_key, cmstar_bytes, enc_ciphertext
CompactShieldedOutput = namedtuple("CompactShieldedOutput", "epk cmu enc_ciphertext")   # CompactOutputDescription: enc_ciphertext[84]
COMPACT_NOTE_SIZE = H.COMPACT_NOTE_SIZE
OutputDescription = namedtuple("OutputDescription", "cv cmu epk enc_ciphertext out_ciphertext")   # (without the proof)
OUT_PLAINTEXT_SIZE, OUT_CIPHERTEXT_SIZE = H.OUT_PLAINTEXT_SIZE, H.OUT_CIPHERTEXT_SIZE
EMPTY_MEMO = b"\xf6" + bytes(MEMO_SIZE - 1)


def compact_output(output):
    """CompactOutputDescription::from(OutputDescription): the first 84 bytes of enc_ciphertext"""
    return CompactShieldedOutput(bytes(output.epk), bytes(output.cmu), bytes(output.enc_ciphertext)[:COMPACT_NOTE_SIZE])


def note_rcm(note):
    """Note::rcm as 32 bytes"""
    return bytes(note.rseed.bytes) if note.rseed.lead_byte == 1 else H.sapling_rseed_scalar(note.rseed.bytes, 4)


def note_derive_esk(note):
    """Note::derive_esk: None before ZIP 212"""
    return None if note.rseed.lead_byte == 1 else H.sapling_rseed_scalar(note.rseed.bytes, 5)


def note_cmu(note, to):
    return H.note_cmu(note.asset_identifier, note.value, to.diversifier, note.pk_d, note_rcm(note))


def _nullifier_arrays(items):
    """items: (Note, PaymentAddress, nk, position) each -> the eight arrays of either note_nullifiers"""
    items = list(items)
    cat = lambda f: np.frombuffer(b"".join(f(it) for it in items), dtype=np.uint8)
    return (cat(lambda it: H._b(it[0].asset_identifier)), np.array([int(it[0].value) for it in items], dtype=np.uint64),
            cat(lambda it: H._b(it[1].diversifier, 11)), cat(lambda it: H._b(it[0].pk_d)),
            np.array([int(it[0].rseed.lead_byte) & 0xff for it in items], dtype=np.uint8), cat(lambda it: H._b(it[0].rseed.bytes)),
            cat(lambda it: H._b(it[2])), np.array([int(it[3]) for it in items], dtype=np.uint64))


NULLIFIER_STATUS = {1: "the asset identifier has no generator", 2: "the diversifier has no g_d", 3: "pk_d does not decode",
                    4: "the lead byte is neither 1 nor 2, or rcm is not below r_J", 5: "nk does not decode"}


BUILD_OUTPUT_STATUS = {1: "the asset identifier has no generator", 2: "the diversifier has no g_d", 3: "pk_d does not decode",
                       4: "the lead byte is neither 1 nor 2, or rcm is not below r_J", 5: "esk is not below r_J", 6: "rcv is not below r_J"}


def _build_output_arrays(plans):
    """plans: (ovk or None, Note, PaymentAddress, memo, rcv, esk=None, out_random=None) each -> the twelve arrays of either build_outputs.
    An absent ovk without out_random gets os.urandom(96), as encrypt_outgoing_plaintext draws it."""
    plans = [tuple(p) + (None,) * (7 - len(p)) for p in plans]
    cat = lambda f: np.frombuffer(b"".join(f(p) for p in plans), dtype=np.uint8)
    scalar = lambda x: bytes(32) if x is None else H._b(x)
    flags = np.array([p[0] is not None for p in plans], dtype=np.uint8)
    randoms = None if flags.all() else cat(lambda p: bytes(96) if p[0] is not None else os.urandom(96) if p[6] is None else H._b(p[6], 96))
    esks = cat(lambda p: scalar(p[5])) if any(p[1].rseed.lead_byte == 1 for p in plans) else None
    return (cat(lambda p: H._b(p[1].asset_identifier)), np.array([int(p[1].value) for p in plans], dtype=np.uint64),
            cat(lambda p: H._b(p[2].diversifier, 11)), cat(lambda p: H._b(p[2].pk_d)),
            np.array([int(p[1].rseed.lead_byte) & 0xff for p in plans], dtype=np.uint8), cat(lambda p: H._b(p[1].rseed.bytes)), esks,
            cat(lambda p: scalar(p[4])), cat(lambda p: H._b(EMPTY_MEMO if p[3] is None else p[3], MEMO_SIZE)), cat(lambda p: scalar(p[0])),
            flags, randoms)


BUILD_SPEND_STATUS = {1: "the asset identifier has no generator", 2: "the diversifier has no g_d", 3: "pk_d does not decode",
                      4: "the lead byte is neither 1 nor 2, or rcm is not below r_J", 5: "ak does not decode", 6: "ak is of small order",
                      7: "nsk is not below r_J", 8: "ar is not below r_J", 9: "rcv is not below r_J"}


def _build_spend_arrays(plans):
    """plans: ((ak, nsk), Note, PaymentAddress, position, ar, rcv) each -> the eleven arrays of either build_spends"""
    cat = lambda f: np.frombuffer(b"".join(f(p) for p in plans), dtype=np.uint8)
    return (cat(lambda p: H._b(p[1].asset_identifier)), np.array([int(p[1].value) for p in plans], dtype=np.uint64),
            cat(lambda p: H._b(p[2].diversifier, 11)), cat(lambda p: H._b(p[1].pk_d)),
            np.array([int(p[1].rseed.lead_byte) & 0xff for p in plans], dtype=np.uint8), cat(lambda p: H._b(p[1].rseed.bytes)),
            cat(lambda p: H._b(p[0][0])), cat(lambda p: H._b(p[0][1])), cat(lambda p: H._b(p[4])), cat(lambda p: H._b(p[5])),
            np.array([int(p[3]) for p in plans], dtype=np.uint64))


def note_nf(note, to, nk, position):
    """Note::nf(&nk, position) -> the 32-byte nullifier, on the host.  nk: the 32 bytes of the NullifierDerivingKey; position: the note's
    position in the commitment tree, below 2^64.  ValueError where the note has none (NULLIFIER_STATUS)."""
    status, _, nfs = H.note_nullifiers(*_nullifier_arrays([(note, to, nk, position)]), threads=1, want_cmus=False)
    if status[0]:
        raise ValueError("note_nf: %s" % NULLIFIER_STATUS.get(int(status[0]), int(status[0])))
    return nfs[0].tobytes()


def note_plaintext_bytes(note, to, memo=EMPTY_MEMO):
    """SaplingDomain::note_plaintext_bytes"""
    memo = bytes(memo)
    assert len(memo) == MEMO_SIZE and note.rseed.lead_byte in (1, 2)
    pt = bytes([note.rseed.lead_byte]) + bytes(to.diversifier) + int(note.value).to_bytes(8, "little") + bytes(note.asset_identifier) + \
        bytes(note.rseed.bytes) + memo
    assert len(pt) == NOTE_PLAINTEXT_SIZE
    return pt


def _parse(plaintext, pk_d):
    lead, d, value = plaintext[0], plaintext[1:12], int.from_bytes(plaintext[12:20], "little")
    note = Note(plaintext[20:52], value, pk_d, Rseed(lead, plaintext[52:84]))
    return note, PaymentAddress(d, pk_d), plaintext[84:]


def sapling_note_encrypt(note, to, memo=EMPTY_MEMO, esk=None):
    """-> ShieldedOutput.  esk: 32 bytes; default the note's derived one (ZIP 212), which a lead-byte-1 note does not have."""
    esk = esk if esk is not None else note_derive_esk(note)
    assert esk is not None, "a note before ZIP 212 needs an esk"
    epk, enc = H.sapling_note_encrypt(esk, to.diversifier, to.pk_d, note_plaintext_bytes(note, to, memo))
    return ShieldedOutput(epk, note_cmu(note, to), enc)


def try_sapling_note_decryption(ivk, output, lead_byte=2):
    """-> (Note, PaymentAddress, memo) or None.  ivk: 32 bytes or an int below r_J; lead_byte: the one valid at the output's height."""
    r = H.sapling_try_note_decryption(ivk, output.epk, output.cmu, output.enc_ciphertext, lead_byte)
    return None if r is None else _parse(*r)


def _parse_compact(plaintext, pk_d):
    note, to, _ = _parse(plaintext, pk_d)
    return note, to


def try_sapling_compact_note_decryption(ivk, output, lead_byte=2):
    """-> (Note, PaymentAddress) or None, on the host.  output: a CompactShieldedOutput."""
    r = H.sapling_try_compact_note_decryption(ivk, output.epk, output.cmu, output.enc_ciphertext, lead_byte)
    return None if r is None else _parse_compact(*r)


def prf_ock(ovk, cv, cmu, epk):
    """PRF^ock -> the 32-byte outgoing cipher key"""
    return H.prf_ock(ovk, cv, cmu, epk)


def encrypt_outgoing_plaintext(ovk, cv, cmu, epk, pk_d, esk, rng_bytes=None):
    """NoteEncryption::encrypt_outgoing_plaintext -> out_ciphertext[80].  ovk None is the ovk = ⊥ case: a random ock and a random op, which
    nobody recovers; rng_bytes: the 96 bytes (ock | op) to use for it instead of os.urandom."""
    if ovk is not None:
        return H.sapling_encrypt_outgoing(H.prf_ock(ovk, cv, cmu, epk), pk_d, esk)
    r = os.urandom(32 + OUT_PLAINTEXT_SIZE) if rng_bytes is None else bytes(rng_bytes)
    assert len(r) == 32 + OUT_PLAINTEXT_SIZE
    return H.sapling_encrypt_outgoing(r[:32], r[32:64], r[64:])


def try_sapling_output_recovery(ovk, output, lead_byte=2):
    """-> (Note, PaymentAddress, memo) or None, on the host.  ovk: 32 bytes; output: an OutputDescription."""
    r = H.sapling_try_output_recovery(ovk, output.cv, output.epk, output.cmu, output.enc_ciphertext, output.out_ciphertext, lead_byte)
    return None if r is None else _parse(*r)


def try_sapling_output_recovery_with_ock(ock, output, lead_byte=2):
    """-> (Note, PaymentAddress, memo) or None, on the host.  ock: the 32-byte outgoing cipher key."""
    r = H.sapling_try_output_recovery_with_ock(ock, output.epk, output.cmu, output.enc_ciphertext, output.out_ciphertext, lead_byte)
    return None if r is None else _parse(*r)


class batch:
    """masp_note_encryption::batch"""

    @staticmethod
    def try_note_decryption(ivks, outputs, ctx, lead_byte=2):
        """One entry per output, in order: None or ((Note, PaymentAddress, memo), index of the first ivk of the list for which the whole
        check succeeds).  ctx: a masp_amd.Context; the scan runs on its GPU."""
        outputs = list(outputs)
        ivks = [H._b(k) for k in ivks]
        result = [None] * len(outputs)
        if not ivks or not outputs:
            return result
        epks = np.frombuffer(b"".join(bytes(o.epk) for o in outputs), dtype=np.uint8)
        encs = np.frombuffer(b"".join(bytes(o.enc_ciphertext) for o in outputs), dtype=np.uint8)
        _, hit_output, hit_ivk, hit_keys = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
        for o, k, key in zip(hit_output.tolist(), hit_ivk.tolist(), hit_keys):   # sorted by (output, ivk): the first success wins
            if result[o] is not None:
                continue
            out = outputs[o]
            r = H.sapling_finish_note_decryption(key.tobytes(), ivks[k], out.epk, out.cmu, out.enc_ciphertext, lead_byte)
            if r is not None:
                result[o] = (_parse(*r), k)
        return result

    @staticmethod
    def try_compact_note_decryption(ivks, outputs, ctx, lead_byte=2):
        """One entry per CompactShieldedOutput, in order: None or ((Note, PaymentAddress), index of the first ivk of the list for which the
        whole check succeeds).  The whole check runs on ctx's GPU: nothing is finished on the host."""
        outputs = list(outputs)
        ivks = [H._b(k) for k in ivks]
        result = [None] * len(outputs)
        if not ivks or not outputs:
            return result
        epks, cmus, encs = (np.frombuffer(b"".join(bytes(getattr(o, f)) for o in outputs), dtype=np.uint8) for f in ("epk", "cmu", "enc_ciphertext"))
        _, hit_output, hit_ivk, hit_pt, hit_pk, _ = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs, lead_byte)
        for o, k, pt, pk in zip(hit_output.tolist(), hit_ivk.tolist(), hit_pt, hit_pk):   # sorted by (output, ivk): the first success wins
            if result[o] is None:
                result[o] = (_parse_compact(pt.tobytes(), pk.tobytes()), k)
        return result

    @staticmethod
    def note_nullifiers(items, ctx, threads=None):
        """items: (Note, PaymentAddress, nk, position) each -> one entry per item, in order: (cmu, nf), 32 bytes each, or None where the
        note has none (note_nf raises there).  ctx: a masp_amd.Context, the notes run on its GPU (masp_hip_sapling_note_nullifiers); None:
        on `threads` host threads."""
        items = list(items)
        if not items:
            return []
        arrays = _nullifier_arrays(items)
        status, cmus, nfs = H.note_nullifiers(*arrays, threads=threads) if ctx is None else ctx.note_nullifiers(*arrays)
        return [None if s else (c.tobytes(), f.tobytes()) for s, c, f in zip(status.tolist(), cmus, nfs)]

    @staticmethod
    def build_outputs(plans, ctx, threads=None):
        """plans: (ovk or None, Note, PaymentAddress, memo, rcv, esk=None, out_random=None) each -> one entry per plan, in order: an
        OutputDescription (without the proof), or None where the plan is refused (BUILD_OUTPUT_STATUS).  esk: for a lead-byte-1 note (a
        ZIP 212 note derives its own); rcv, esk: 32 bytes or an int; out_random: the 96 bytes (ock | op) of an output without ovk, default
        os.urandom(96) as encrypt_outgoing_plaintext draws them.  Everything below this is a function of its inputs.  ctx: a
        masp_amd.Context, the outputs are built on its GPU (masp_hip_sapling_build_outputs); None: on `threads` host threads."""
        plans = list(plans)
        if not plans:
            return []
        arrays = _build_output_arrays(plans)
        status, cvs, cmus, epks, encs, couts = H.build_outputs(*arrays, threads=threads) if ctx is None else ctx.build_outputs(*arrays)
        return [None if s else OutputDescription(cv.tobytes(), cmu.tobytes(), epk.tobytes(), enc.tobytes(), cout.tobytes())
                for s, cv, cmu, epk, enc, cout in zip(status.tolist(), cvs, cmus, epks, encs, couts)]

    @staticmethod
    def build_spends(plans, ctx, threads=None):
        """plans: ((ak, nsk), Note, PaymentAddress, position, ar, rcv) each -> one entry per plan, in order: (cv, rk, nf, cmu, nk), 32 bytes
        each, what the builder puts around a Spend proof and the nk it derived on the way, or None where the plan is refused
        (BUILD_SPEND_STATUS).  (ak, nsk): the proof generation key; nsk, ar, rcv: 32 bytes or an int.  The anchor is the caller's, from the
        tree.  A function of its inputs.  ctx: a masp_amd.Context, the spends are built on its GPU (masp_hip_sapling_build_spends); None: on
        `threads` host threads."""
        plans = list(plans)
        if not plans:
            return []
        arrays = _build_spend_arrays(plans)
        status, cvs, rks, nfs, cmus, nks = H.build_spends(*arrays, threads=threads) if ctx is None else ctx.build_spends(*arrays)
        return [None if s else tuple(a.tobytes() for a in row) for s, *row in zip(status.tolist(), cvs, rks, nfs, cmus, nks)]

    @staticmethod
    def try_output_recovery(ovks, outputs, ctx, lead_byte=2):
        """One entry per OutputDescription, in order: None or ((Note, PaymentAddress, memo), index of the first ovk of the list for which the
        whole check succeeds).  ctx: a masp_amd.Context; the scan runs on its GPU."""
        outputs = list(outputs)
        ovks = [H._b(k) for k in ovks]
        result = [None] * len(outputs)
        if not ovks or not outputs:
            return result
        cvs, epks, cmus, couts = (np.frombuffer(b"".join(bytes(getattr(o, f)) for o in outputs), dtype=np.uint8)
                                  for f in ("cv", "epk", "cmu", "out_ciphertext"))
        hit_output, hit_ovk, hit_ocks = ctx.sapling_output_recovery_scan(b"".join(ovks), cvs, epks, cmus, couts)
        for o, k, ock in zip(hit_output.tolist(), hit_ovk.tolist(), hit_ocks):   # sorted by (output, ovk): the first success wins
            if result[o] is not None:
                continue
            out = outputs[o]
            r = H.sapling_try_output_recovery_with_ock(ock.tobytes(), out.epk, out.cmu, out.enc_ciphertext, out.out_ciphertext, lead_byte)
            if r is not None:
                result[o] = (_parse(*r), k)
        return result
