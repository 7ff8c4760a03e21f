"""Outputs for the output recovery tests (test_output_recovery_host.py, test_gpu_output_recovery.py): honest sent notes, and rows crafted
from them by re-encrypting a chosen op or note plaintext under the right key with pynote's AEAD, so that out_ciphertext's tag verifies
and exactly one later check of try_output_recovery_with_ock is left to refuse.  Each crafted row has a positive control made the same way."""
import random

import pynote
from masp_amd import host as H
from masp_amd import note_encryption as NE

RJ = H.JUBJUB_ORDER
NONCE = bytes(12)
IDENTITY = (1).to_bytes(32, "little")                       # (0, 1)
ORDER2 = (H.FR_MODULUS - 1).to_bytes(32, "little")          # (0, -1)


def recipient(seed):
    """a payment address of a random ivk"""
    rng = random.Random(seed)
    ivk = rng.randrange(1, RJ)
    while True:
        d = rng.randbytes(11)
        try:
            gd = H.diversifier_base(d)
        except H.HostError:
            continue
        return NE.PaymentAddress(d, H.jubjub_mul(gd, ivk.to_bytes(32, "little")))


class Sent:
    """an honest output sent under ovk (None: ovk = ⊥), with what made it"""

    def __init__(self, ovk, asset, seed, lead_byte=2):
        rng = random.Random(seed)
        self.ovk, self.to = ovk, recipient(seed)
        if lead_byte == 2:
            self.note = NE.Note(asset, rng.randrange(1 << 64), self.to.pk_d, NE.Rseed(2, rng.randbytes(32)))
            self.esk = NE.note_derive_esk(self.note)
        else:
            self.note = NE.Note(asset, rng.randrange(1 << 64), self.to.pk_d, NE.Rseed(1, rng.randrange(RJ).to_bytes(32, "little")))
            self.esk = rng.randrange(1, RJ).to_bytes(32, "little")
        self.memo = rng.randbytes(512)
        self.cv = H.value_commitment(asset, self.note.value, rng.randrange(RJ).to_bytes(32, "little"))[0]
        out = NE.sapling_note_encrypt(self.note, self.to, self.memo, esk=self.esk)
        c_out = NE.encrypt_outgoing_plaintext(ovk, self.cv, out.cmu, out.epk, self.to.pk_d, self.esk, rng_bytes=rng.randbytes(96))
        self.output = NE.OutputDescription(self.cv, out.cmu, out.epk, out.enc_ciphertext, c_out)
        self.plaintext = NE.note_plaintext_bytes(self.note, self.to, self.memo)
        self.result = (self.note, self.to, self.memo)


def seal(key, plaintext):
    ct, tag = pynote.aead_encrypt(key, NONCE, plaintext)
    return ct + tag


def remake(s, pk_d=None, esk=None, cmu=None, secret_of=None, plaintext=None):
    """s.output with op = pk_d | esk and the given cmu; out_ciphertext under the right ock for (ovk, cv, cmu, epk); enc_ciphertext again
    under kdf(secret, epk) for secret = [8 secret_of[1]] secret_of[0] where asked (else as it is)"""
    o = s.output
    pk_d, esk, cmu = pk_d or s.to.pk_d, esk or s.esk, cmu or o.cmu
    enc = o.enc_ciphertext
    if secret_of is not None:
        enc = seal(pynote.kdf_sapling(H.sapling_ka_agree(secret_of[1], secret_of[0]), o.epk), plaintext or s.plaintext)
    return o._replace(cmu=cmu, enc_ciphertext=enc, out_ciphertext=seal(H.prf_ock(s.ovk, o.cv, cmu, o.epk), pk_d + esk))


def off_curve():
    return next(v.to_bytes(32, "little") for v in range(2, 100) if H.load_library().masp_host_point_uv(v.to_bytes(32, "little"), bytes(64)) != 0)


def crafted(s, seed):
    """s: a Sent of lead byte 2 -> (controls, refused): lists of (name, OutputDescription).  Every row's out_ciphertext verifies under
    s.ovk; the controls are recovered as s.result, the refused rows by nothing."""
    rng = random.Random(seed)
    o, pk, esk = s.output, s.to.pk_d, s.esk
    one = (1).to_bytes(32, "little")
    controls = [("op as it was, sealed by the mirror", remake(s)),
                ("enc sealed again under the honest secret", remake(s, secret_of=(pk, esk)))]
    assert controls[0][1] == o
    mixed = H.jubjub_add(pk, ORDER2)                        # decodes, [8 esk] of it is the honest secret, not in the subgroup
    assert H.sapling_ka_agree(esk, mixed) == H.sapling_ka_agree(esk, pk)
    cmu_mixed = H.note_cmu(s.note.asset_identifier, s.note.value, s.to.diversifier, mixed, NE.note_rcm(s.note))
    esk2 = rng.randrange(1, RJ).to_bytes(32, "little")
    other = NE.sapling_note_encrypt(s.note, s.to, s.memo, esk=esk2)      # epk, enc and op consistent under esk2, which the rseed does not give
    zip212 = NE.OutputDescription(o.cv, other.cmu, other.epk, other.enc_ciphertext,
                                  NE.encrypt_outgoing_plaintext(s.ovk, o.cv, other.cmu, other.epk, pk, esk2))
    bad_cmu = bytearray(o.cmu)
    bad_cmu[rng.randrange(31)] ^= 1 << rng.randrange(8)
    refused = [
        ("pk_d the identity", remake(s, pk_d=IDENTITY, secret_of=(IDENTITY, one))),
        ("pk_d of order 2", remake(s, pk_d=ORDER2, secret_of=(IDENTITY, one))),
        ("pk_d outside the subgroup", remake(s, pk_d=mixed, cmu=cmu_mixed)),
        ("pk_d does not decode", remake(s, pk_d=off_curve())),
        ("esk not canonical", remake(s, esk=(int.from_bytes(esk, "little") + RJ).to_bytes(32, "little"))),
        ("esk does not give epk", remake(s, esk=esk2, secret_of=(pk, esk2))),
        ("ZIP 212", zip212),
        ("wrong cmu", remake(s, cmu=bytes(bad_cmu))),
    ]
    return controls, refused
