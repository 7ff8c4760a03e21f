"""Output recovery with outgoing viewing keys on the host (libmasp_host.so: csrc/host/note_encryption.h) against the reference's ten
vectors (tests/golden/note_encryption_vectors.json: ovk, cv, ock, op, c_out) and the pure-Python mirror (pynote.py); every refusal of
try_output_recovery_with_ock, each beside a positive control; the host batch function; and the device header of the GPU scan
(device/out_recovery.hpp) compiled for the CPU.  Every comparison is of bytes."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import out_recovery_cases as K
import out_recovery_shim as S
import pynote
from masp_amd import host as H
from masp_amd import note_encryption as NE

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "note_encryption_vectors.json")))
VECTORS = [{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in tv.items()} for tv in DOC["vectors"]]
ASSET = bytes.fromhex(DOC["asset_identifier"])
NONCE = bytes(12)


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def description(tv):
    return NE.OutputDescription(tv["cv"], tv["cmu"], tv["epk"], tv["c_enc"], tv["c_out"])


@pytest.mark.parametrize("i", range(10))
def test_vector(i):
    tv = VECTORS[i]
    assert NE.prf_ock(tv["ovk"], tv["cv"], tv["cmu"], tv["epk"]) == tv["ock"]
    assert hashlib.blake2b(tv["ovk"] + tv["cv"] + tv["cmu"] + tv["epk"], digest_size=32, person=b"MASP__Derive_ock").digest() == tv["ock"]
    assert tv["default_pk_d"] + tv["esk"] == tv["op"]
    assert H.sapling_encrypt_outgoing(tv["ock"], tv["default_pk_d"], tv["esk"]) == tv["c_out"] == K.seal(tv["ock"], tv["op"])
    assert NE.encrypt_outgoing_plaintext(tv["ovk"], tv["cv"], tv["cmu"], tv["epk"], tv["default_pk_d"], tv["esk"]) == tv["c_out"]
    out = description(tv)
    want = (NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"])), NE.PaymentAddress(tv["default_d"], tv["default_pk_d"]), tv["memo"])
    assert NE.try_sapling_output_recovery(tv["ovk"], out, lead_byte=1) == want
    assert NE.try_sapling_output_recovery_with_ock(tv["ock"], out, lead_byte=1) == want
    assert NE.try_sapling_output_recovery(tv["ovk"], out, lead_byte=2) is None
    assert NE.try_sapling_output_recovery_with_ock(tv["ock"], out, lead_byte=2) is None


def test_the_subgroup_test_of_the_host_curve():
    """what extract_pk_d needs and the other paths never did: the identity and an honest pk_d pass, the point of order 2 and pk_d + it do not"""
    pk = K.recipient(1).pk_d
    # (the verdicts themselves are read through try_output_recovery_with_ock's refusals below; here the arithmetic they rest on)
    assert H.jubjub_mul(pk, K.RJ.to_bytes(32, "little")) == K.IDENTITY
    assert H.jubjub_mul(K.ORDER2, K.RJ.to_bytes(32, "little")) == K.ORDER2            # r_J is odd
    assert H.jubjub_mul(H.jubjub_add(pk, K.ORDER2), K.RJ.to_bytes(32, "little")) == K.ORDER2


@pytest.fixture(scope="module")
def sent():
    return K.Sent(random.Random(70).randbytes(32), ASSET, 71)


def test_honest_outputs_round_trip(sent):
    for lead in (1, 2):
        s = K.Sent(sent.ovk, ASSET, 72 + lead, lead)
        ock = NE.prf_ock(s.ovk, s.output.cv, s.output.cmu, s.output.epk)
        assert NE.try_sapling_output_recovery(s.ovk, s.output, lead) == s.result
        assert NE.try_sapling_output_recovery_with_ock(ock, s.output, lead) == s.result
        assert NE.try_sapling_output_recovery(s.ovk, s.output, 3 - lead) is None
        # the recipient's and the sender's view of the same output agree
        assert pynote.aead_decrypt(ock, NONCE, s.output.out_ciphertext[:64], s.output.out_ciphertext[64:]) == s.to.pk_d + s.esk


def test_wrong_key_and_broken_ciphertexts(sent):
    rng = random.Random(73)
    o = sent.output
    assert NE.try_sapling_output_recovery(sent.ovk, o) == sent.result
    assert NE.try_sapling_output_recovery(rng.randbytes(32), o) is None                                           # a wrong ovk
    assert NE.try_sapling_output_recovery(flip(sent.ovk, rng.randrange(256)), o) is None
    for bit in [0, 64 * 8 - 1, rng.randrange(64 * 8)]:                                                             # the body of c_out
        assert NE.try_sapling_output_recovery(sent.ovk, o._replace(out_ciphertext=flip(o.out_ciphertext, bit))) is None
    for bit in [64 * 8, 80 * 8 - 1, 64 * 8 + rng.randrange(128)]:                                                  # its tag
        assert NE.try_sapling_output_recovery(sent.ovk, o._replace(out_ciphertext=flip(o.out_ciphertext, bit))) is None
    for bit in [596 * 8, 612 * 8 - 1, rng.randrange(596 * 8)]:                                                     # enc: its tag, its body
        assert NE.try_sapling_output_recovery(sent.ovk, o._replace(enc_ciphertext=flip(o.enc_ciphertext, bit))) is None
    for f in ("cv", "cmu", "epk"):                                                                                # the ock is over all three
        assert NE.try_sapling_output_recovery(sent.ovk, o._replace(**{f: flip(getattr(o, f), rng.randrange(255))})) is None


def test_every_refusal_behind_a_valid_out_ciphertext(sent):
    controls, refused = K.crafted(sent, 74)
    assert [n for n, _ in refused] == ["pk_d the identity", "pk_d of order 2", "pk_d outside the subgroup", "pk_d does not decode",
                                       "esk not canonical", "esk does not give epk", "ZIP 212", "wrong cmu"]
    for name, o in controls:
        assert NE.try_sapling_output_recovery(sent.ovk, o) == sent.result, name
    for name, o in refused:
        ock = NE.prf_ock(sent.ovk, o.cv, o.cmu, o.epk)
        assert pynote.aead_decrypt(ock, NONCE, o.out_ciphertext[:64], o.out_ciphertext[64:]) is not None, name    # the tag is not the reason
        assert NE.try_sapling_output_recovery(sent.ovk, o) is None, name
        assert NE.try_sapling_output_recovery_with_ock(ock, o) is None, name
    by = dict(refused)
    # the rows whose enc_ciphertext also opens under the key op gives: refused by the one check the row is named for
    for name in ("pk_d the identity", "pk_d of order 2", "pk_d outside the subgroup", "esk not canonical", "esk does not give epk", "ZIP 212", "wrong cmu"):
        o = by[name]
        op = pynote.aead_decrypt(NE.prf_ock(sent.ovk, o.cv, o.cmu, o.epk), NONCE, o.out_ciphertext[:64], o.out_ciphertext[64:])
        key = pynote.kdf_sapling(H.sapling_ka_agree((int.from_bytes(op[32:], "little") % K.RJ).to_bytes(32, "little"), op[:32]), o.epk)
        assert pynote.aead_decrypt(key, NONCE, o.enc_ciphertext[:596], o.enc_ciphertext[596:]) == sent.plaintext, name
    # outside the subgroup: the same row with the honest pk_d and cmu is the honest output; nothing but pk_d's coset differs
    o = by["pk_d outside the subgroup"]
    assert o.enc_ciphertext == sent.output.enc_ciphertext and o.epk == sent.output.epk
    # ZIP 212: the recipient's side refuses the same output by its esk check
    assert by["ZIP 212"].epk != sent.output.epk and by["ZIP 212"].cmu == sent.output.cmu


def test_zip212_control_is_the_same_construction(sent):
    out = NE.sapling_note_encrypt(sent.note, sent.to, sent.memo, esk=sent.esk)
    o = NE.OutputDescription(sent.cv, out.cmu, out.epk, out.enc_ciphertext,
                             NE.encrypt_outgoing_plaintext(sent.ovk, sent.cv, out.cmu, out.epk, sent.to.pk_d, sent.esk))
    assert o == sent.output and NE.try_sapling_output_recovery(sent.ovk, o) == sent.result
    # before ZIP 212 there is no derived esk: any esk that gives epk is accepted
    s1 = K.Sent(sent.ovk, ASSET, 75, 1)
    assert NE.try_sapling_output_recovery(s1.ovk, s1.output, 1) == s1.result


def test_an_output_without_ovk_is_recovered_by_nobody(sent):
    rng = random.Random(76)
    r = rng.randbytes(96)
    s = K.Sent(None, ASSET, 77)
    assert NE.try_sapling_output_recovery(sent.ovk, s.output) is None
    o = s.output
    c_out = NE.encrypt_outgoing_plaintext(None, o.cv, o.cmu, o.epk, s.to.pk_d, s.esk, rng_bytes=r)
    assert c_out == K.seal(r[:32], r[32:]) and len(c_out) == 80
    assert NE.try_sapling_output_recovery_with_ock(r[:32], o._replace(out_ciphertext=c_out)) is None              # the tag verifies, op is noise
    assert NE.encrypt_outgoing_plaintext(None, o.cv, o.cmu, o.epk, s.to.pk_d, s.esk) != NE.encrypt_outgoing_plaintext(None, o.cv, o.cmu, o.epk, s.to.pk_d, s.esk)
    # the recipient still reads it
    assert s.output.enc_ciphertext == NE.sapling_note_encrypt(s.note, s.to, s.memo).enc_ciphertext


def columns(outs):
    return [np.frombuffer(b"".join(getattr(o, f) for o in outs), np.uint8).reshape(len(outs), -1)
            for f in ("cv", "epk", "cmu", "enc_ciphertext", "out_ciphertext")]


def test_host_batch_equals_the_per_pair_loop(sent):
    rng = random.Random(78)
    stranger, mine = rng.randbytes(32), sent.ovk
    controls, refused = K.crafted(sent, 79)
    outs = [description(tv) for tv in VECTORS] + [sent.output, K.Sent(stranger, ASSET, 80).output, K.Sent(None, ASSET, 81).output] + \
        [o for _, o in controls + refused] + [K.Sent(mine, ASSET, 82, 1).output]
    ovks = [VECTORS[3]["ovk"], stranger, mine, mine, VECTORS[7]["ovk"]]
    cvs, epks, cmus, encs, couts = columns(outs)
    for lead in (1, 2):
        hit, pts, pks = H.sapling_try_output_recovery_batch(ovks, cvs, epks, cmus, encs, couts, lead_byte=lead, threads=3)
        want = []
        for o in outs:
            rs = [H.sapling_try_output_recovery(k, o.cv, o.epk, o.cmu, o.enc_ciphertext, o.out_ciphertext, lead) for k in ovks]
            first = next((i for i, r in enumerate(rs) if r is not None), -1)
            want.append((first, rs[first] if first >= 0 else None))
        assert hit.tolist() == [w[0] for w in want]
        assert [(pts[i].tobytes(), pks[i].tobytes()) for i, w in enumerate(want) if w[1]] == [w[1] for w in want if w[1]]
        assert sum(1 for w in want if w[1]) == (3 if lead == 1 else 4)
    # an ovk listed twice behind a stranger: the first index
    hit, _, _ = H.sapling_try_output_recovery_batch([stranger, mine, mine], cvs, epks, cmus, encs, couts, lead_byte=2)
    assert hit.tolist()[10] == 1 and hit.tolist()[11] == 0 and sorted(set(hit.tolist())) == [-1, 0, 1]
    hit, _, _ = H.sapling_try_output_recovery_batch([], cvs, epks, cmus, encs, couts, lead_byte=2)
    assert hit.tolist() == [-1] * len(outs)


def pair_cases(sent):
    """the ten vectors, 64 random rows (of every eight, one with a c_out sealed under the row's own ock and one with such a c_out and a
    flipped bit) and the crafted rows"""
    rng = random.Random(83)
    pairs = [(tv["ovk"], tv["cv"], tv["cmu"], tv["epk"], tv["c_out"]) for tv in VECTORS]
    for i in range(64):
        ovk, cv, cmu, epk = (rng.randbytes(32) for _ in range(4))
        c_out = K.seal(H.prf_ock(ovk, cv, cmu, epk), rng.randbytes(64)) if i % 4 == 0 else rng.randbytes(80)
        if i % 8 == 4:
            c_out = flip(K.seal(H.prf_ock(ovk, cv, cmu, epk), rng.randbytes(64)), rng.randrange(640))
        pairs.append((ovk, cv, cmu, epk, c_out))
    controls, refused = K.crafted(sent, 74)
    pairs += [(sent.ovk, o.cv, o.cmu, o.epk, o.out_ciphertext) for _, o in controls + refused]
    return pairs


def check_pair_function(sent, gpu):
    pairs = pair_cases(sent)
    got = S.run(pairs, gpu)
    want = []
    for ovk, cv, cmu, epk, c_out in pairs:
        ock = H.prf_ock(ovk, cv, cmu, epk)
        want.append((ock, H.chacha20poly1305_decrypt(ock, NONCE, c_out[:64], c_out[64:]) is not None))
    assert got == want
    assert sum(1 for w in want if w[1]) == 10 + 8 + 10 and sum(1 for w in want if not w[1]) == 56


def test_the_device_header_on_the_host(sent):
    check_pair_function(sent, False)
