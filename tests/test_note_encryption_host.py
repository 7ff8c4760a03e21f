"""Sapling note encryption on the host (libmasp_host.so: csrc/host/chacha20poly1305.h, note_encryption.h) against the reference's ten
vectors (tests/golden/note_encryption_vectors.json, lead byte 1) and an independent pure-Python mirror (pynote.py); every refusal of
try_sapling_note_decryption; lead byte 2 round trips.  Every comparison is of bytes."""
import json
import os
import random

import pytest

import pynote
from masp_amd import host as H
from masp_amd import note_encryption as NE

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "note_encryption_vectors.json")))
VECTORS = [{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in tv.items()} for tv in DOC["vectors"]]
ASSET = bytes.fromhex(DOC["asset_identifier"])
NONCE = bytes(12)
RJ = H.JUBJUB_ORDER


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def test_there_are_ten_vectors_with_lead_byte_one():
    assert len(VECTORS) == 10 and DOC["lead_byte"] == 1
    assert all(tv["p_enc"][0] == 1 and tv["p_enc"][20:52] == ASSET for tv in VECTORS)


def test_rfc8439_aead_vector_pins_the_mirror_and_the_host():
    key, nonce = bytes(range(0x80, 0xa0)), bytes.fromhex("070000004041424344454647")
    pt = b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be it."
    ct, tag = pynote.aead_encrypt(key, nonce, pt, bytes.fromhex("50515253c0c1c2c3c4c5c6c7"))
    assert tag.hex() == "1ae10b594f09e26a7e902ecbd0600691" and ct[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    # RFC 8439 2.5.2: Poly1305 alone
    k = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert pynote.poly1305(k, b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"
    rng = random.Random(5)
    for n in list(range(0, 35)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 595, 596, 597, 1000]:
        key, nonce, m = rng.randbytes(32), rng.randbytes(12), rng.randbytes(n)
        ct, tag = H.chacha20poly1305_encrypt(key, nonce, m)
        assert (ct, tag) == pynote.aead_encrypt(key, nonce, m), n
        assert H.chacha20poly1305_decrypt(key, nonce, ct, tag) == m
        assert H.chacha20poly1305_decrypt(key, nonce, ct, flip(tag, rng.randrange(128))) is None
    # Poly1305 accumulators at the edges of the field: r and the blocks all ones
    for key in (b"\xff" * 32, b"\xff" * 16 + bytes(16), bytes(16) + b"\xff" * 16):
        for m in (b"\xff" * 16, b"\xff" * 64, b"\xff" * 17, b"\xfb" + b"\xff" * 15):
            otk = pynote.chacha20_block(key, 0, NONCE)[:32]
            assert H.chacha20poly1305_encrypt(key, NONCE, m)[1] == pynote.poly1305(otk, pynote._pad16(pynote.chacha20_xor(key, 1, NONCE, m)) +
                                                                                    (0).to_bytes(8, "little") + len(m).to_bytes(8, "little"))


@pytest.mark.parametrize("i", range(10))
def test_vector(i):
    tv = VECTORS[i]
    # key agreement from both sides, the KDF, against the vector and the mirror
    assert H.sapling_ka_agree(tv["esk"], tv["default_pk_d"]) == tv["shared_secret"]
    assert H.sapling_ka_agree(tv["ivk"], tv["epk"]) == tv["shared_secret"]
    assert H.kdf_sapling(tv["shared_secret"], tv["epk"]) == tv["k_enc"] == pynote.kdf_sapling(tv["shared_secret"], tv["epk"])
    # the AEAD
    ct, tag = pynote.aead_encrypt(tv["k_enc"], NONCE, tv["p_enc"])
    assert ct + tag == tv["c_enc"]
    assert H.chacha20poly1305_encrypt(tv["k_enc"], NONCE, tv["p_enc"]) == (ct, tag)
    # encryption with the vector's esk
    to = NE.PaymentAddress(tv["default_d"], tv["default_pk_d"])
    note = NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"]))
    assert NE.note_plaintext_bytes(note, to, tv["memo"]) == tv["p_enc"]
    out = NE.sapling_note_encrypt(note, to, tv["memo"], esk=tv["esk"])
    assert out.epk == tv["epk"] and out.enc_ciphertext == tv["c_enc"] and out.cmu == tv["cmu"]
    # decryption with the vector's ivk
    got = NE.try_sapling_note_decryption(tv["ivk"], out, lead_byte=1)
    assert got == (note, to, tv["memo"])
    assert H.sapling_finish_note_decryption(tv["k_enc"], tv["ivk"], tv["epk"], tv["cmu"], tv["c_enc"], 1) == (tv["p_enc"], tv["default_pk_d"])
    assert pynote.aead_decrypt(tv["k_enc"], NONCE, tv["c_enc"][:596], tv["c_enc"][596:]) == tv["p_enc"]


def test_every_refusal_on_the_vectors():
    rng = random.Random(6)
    for tv in VECTORS[:4]:
        out = NE.ShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"])
        assert NE.try_sapling_note_decryption(tv["ivk"], out, lead_byte=1) is not None
        assert NE.try_sapling_note_decryption(tv["ivk"], out, lead_byte=2) is None                              # the wrong lead byte
        for bit in [596 * 8, 612 * 8 - 1, 596 * 8 + rng.randrange(128)]:                                          # the tag
            assert NE.try_sapling_note_decryption(tv["ivk"], out._replace(enc_ciphertext=flip(tv["c_enc"], bit)), 1) is None
        for bit in [0, 596 * 8 - 1, rng.randrange(596 * 8)]:                                                      # the ciphertext
            assert NE.try_sapling_note_decryption(tv["ivk"], out._replace(enc_ciphertext=flip(tv["c_enc"], bit)), 1) is None
        for bit in [0, 255, rng.randrange(256)]:                                                                  # epk (decoding or not)
            assert NE.try_sapling_note_decryption(tv["ivk"], out._replace(epk=flip(tv["epk"], bit)), 1) is None
        for bit in [0, rng.randrange(255)]:                                                                       # cmu
            assert NE.try_sapling_note_decryption(tv["ivk"], out._replace(cmu=flip(tv["cmu"], bit)), 1) is None
        other = VECTORS[5]["ivk"]
        assert NE.try_sapling_note_decryption(other, out, 1) is None                                               # another ivk
        assert NE.try_sapling_note_decryption(0, out, 1) is None
        assert NE.try_sapling_note_decryption(RJ - 1, out, 1) is None
        with pytest.raises(H.HostError):
            NE.try_sapling_note_decryption(RJ, out, 1)                                                             # not a SaplingIvk
    # epk not canonical (v >= r), not on the curve, negative zero
    tv = VECTORS[0]
    off_curve = next(v for v in range(2, 100) if H.load_library().masp_host_point_uv(v.to_bytes(32, "little"), bytes(64)) != 0)
    for epk in ((H.FR_MODULUS + 1).to_bytes(32, "little"), b"\xff" * 32, off_curve.to_bytes(32, "little"), (1 | (1 << 255)).to_bytes(32, "little")):
        assert NE.try_sapling_note_decryption(tv["ivk"], NE.ShieldedOutput(epk, tv["cmu"], tv["c_enc"]), 1) is None


def _recipient(ivk, d_seed):
    """a diversifier with a g_d and pk_d = [ivk] g_d"""
    rng = random.Random(d_seed)
    while True:
        d = rng.randbytes(11)
        try:
            gd = H.diversifier_base(d)
        except H.HostError:
            continue
        return NE.PaymentAddress(d, H.jubjub_mul(gd, ivk.to_bytes(32, "little")))


def test_parse_refusals_inside_a_valid_ciphertext():
    """Ciphertexts whose tag verifies (made with the right key) and whose plaintext is refused: asset identifier, rcm >= r_J, a
    diversifier without g_d — and the commitment: the refusals of sapling_parse_note_plaintext_without_memo."""
    tv = VECTORS[1]
    def enc(pt):
        ct, tag = pynote.aead_encrypt(tv["k_enc"], NONCE, pt)
        return NE.ShieldedOutput(tv["epk"], tv["cmu"], ct + tag)
    p = tv["p_enc"]
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p), 1) is not None
    bad_asset = next(a for a in (bytes([i]) * 32 for i in range(256)) if H.load_library().masp_host_asset_generator(a, bytes(32)) != 0)
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:20] + bad_asset + p[52:]), 1) is None
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:52] + RJ.to_bytes(32, "little") + p[84:]), 1) is None
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:52] + b"\xff" * 32 + p[84:]), 1) is None
    bad_d = next(d for d in (bytes([i]) * 11 for i in range(256)) if _no_gd(d))
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:1] + bad_d + p[12:]), 1) is None
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:12] + (tv["v"] + 1).to_bytes(8, "little") + p[20:]), 1) is None   # the commitment
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(b"\x02" + p[1:]), 1) is None
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(b"\x00" + p[1:]), 0) is None
    # the memo is not committed to: another memo is another valid note
    assert NE.try_sapling_note_decryption(tv["ivk"], enc(p[:84] + b"\x01" * 512), 1)[2] == b"\x01" * 512


def _no_gd(d):
    try:
        H.diversifier_base(d)
        return False
    except H.HostError:
        return True


def test_lead_byte_two_round_trips_and_the_esk_check():
    rng = random.Random(7)
    for k in range(4):
        ivk = rng.randrange(1, RJ) if k else RJ - 1
        to = _recipient(ivk, 100 + k)
        rseed = rng.randbytes(32)
        note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(2, rseed))
        # rcm and esk derived from the rseed, against the mirror
        assert NE.note_rcm(note) == pynote.rseed_scalar(rseed, 4) and NE.note_derive_esk(note) == pynote.rseed_scalar(rseed, 5)
        assert H.prf_expand(rseed, b"\x04") == pynote.prf_expand(rseed, b"\x04")
        memo = rng.randbytes(512)
        out = NE.sapling_note_encrypt(note, to, memo)
        # the mirror agrees on every byte of the output
        esk = pynote.rseed_scalar(rseed, 5)
        assert out.epk == H.jubjub_mul(H.diversifier_base(to.diversifier), esk)
        key = pynote.kdf_sapling(H.sapling_ka_agree(esk, to.pk_d), out.epk)
        ct, tag = pynote.aead_encrypt(key, NONCE, NE.note_plaintext_bytes(note, to, memo))
        assert out.enc_ciphertext == ct + tag
        assert NE.try_sapling_note_decryption(ivk, out) == (note, to, memo)
        assert NE.try_sapling_note_decryption(ivk, out, lead_byte=1) is None
        assert NE.try_sapling_note_decryption(ivk % (RJ - 1) + 1, out) is None
        # the same note under an esk other than the derived one: tag and commitment pass, the esk check refuses
        other = NE.sapling_note_encrypt(note, to, memo, esk=rng.randrange(1, RJ).to_bytes(32, "little"))
        assert other.cmu == out.cmu and other.epk != out.epk
        assert NE.try_sapling_note_decryption(ivk, other) is None
        key2 = H.kdf_sapling(H.sapling_ka_agree(ivk.to_bytes(32, "little"), other.epk), other.epk)
        assert pynote.aead_decrypt(key2, NONCE, other.enc_ciphertext[:596], other.enc_ciphertext[596:]) == NE.note_plaintext_bytes(note, to, memo)


def test_host_batch_reports_the_first_ivk():
    ivks = [tv["ivk"] for tv in VECTORS]
    hit, pts, pks = H.sapling_try_note_decryption_batch(ivks + ivks, [tv["epk"] for tv in VECTORS], [tv["cmu"] for tv in VECTORS],
                                                        [tv["c_enc"] for tv in VECTORS], lead_byte=1, threads=3)
    assert hit.tolist() == list(range(10))
    assert [p.tobytes() for p in pts] == [tv["p_enc"] for tv in VECTORS] and [p.tobytes() for p in pks] == [tv["default_pk_d"] for tv in VECTORS]
    hit, _, _ = H.sapling_try_note_decryption_batch(ivks[3:5], [tv["epk"] for tv in VECTORS], [tv["cmu"] for tv in VECTORS],
                                                    [tv["c_enc"] for tv in VECTORS], lead_byte=1)
    assert hit.tolist() == [-1, -1, -1, 0, 1, -1, -1, -1, -1, -1]
