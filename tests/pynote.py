"""Pure-Python ChaCha20, Poly1305, the RFC 8439 AEAD and the Sapling KDF / PRF^expand, written from the specifications (RFC 8439,
RFC 7693 through hashlib, the Zcash protocol specification 5.4.4.3-4): the independent side of the note-encryption tests."""
import hashlib
import struct

JUBJUB_ORDER = 6554484396890773809930967563523245729705921265872317281365359162392183254199


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xffffffff


def chacha20_block(key, counter, nonce):
    s = list(struct.unpack("<4I", b"expand 32-byte k")) + list(struct.unpack("<8I", key)) + [counter & 0xffffffff] + list(struct.unpack("<3I", nonce))
    x = s[:]

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & 0xffffffff for a, b in zip(x, s)))


def chacha20_xor(key, counter, nonce, data):
    out = bytearray()
    for off in range(0, len(data), 64):
        ks = chacha20_block(key, counter + off // 64, nonce)
        out += bytes(a ^ b for a, b in zip(data[off:off + 64], ks))
    return bytes(out)


def poly1305(key, msg):
    r = int.from_bytes(key[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    s = int.from_bytes(key[16:32], "little")
    p = (1 << 130) - 5
    acc = 0
    for off in range(0, len(msg), 16):
        blk = msg[off:off + 16]
        acc = (acc + int.from_bytes(blk + b"\x01", "little")) * r % p
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(b):
    return b + bytes(-len(b) % 16)


def aead_encrypt(key, nonce, plaintext, aad=b""):
    otk = chacha20_block(key, 0, nonce)[:32]
    ct = chacha20_xor(key, 1, nonce, plaintext)
    tag = poly1305(otk, _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct)))
    return ct, tag


def aead_decrypt(key, nonce, ct, tag, aad=b""):
    otk = chacha20_block(key, 0, nonce)[:32]
    if poly1305(otk, _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))) != tag:
        return None
    return chacha20_xor(key, 1, nonce, ct)


def kdf_sapling(secret, epk):
    return hashlib.blake2b(secret + epk, digest_size=32, person=b"MASP__SaplingKDF").digest()


def prf_expand(sk, t):
    return hashlib.blake2b(sk + t, digest_size=64, person=b"MASP__ExpandSeed").digest()


def rseed_scalar(rseed, domain):
    return (int.from_bytes(prf_expand(rseed, bytes([domain])), "little") % JUBJUB_ORDER).to_bytes(32, "little")
