"""The note scan's device headers on their own (masp_amd/csrc/device/blake2b.hpp, chacha20.hpp, poly1305.hpp) against hashlib and
the pure-Python mirror, at message lengths around the 16-, 64- and 128-byte boundaries: compiled for the host, and in a kernel."""
import hashlib
import random

import pytest

import note_crypto_shim as S
import pynote


def _cases():
    rng = random.Random(21)
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 111, 112, 113, 127, 128]
    b2b, cc, poly = [], [], []
    for n in lens:
        msg = rng.randbytes(n)
        for outlen in (32, 64):
            person = rng.randbytes(16) if n % 2 else b"MASP__SaplingKDF"
            b2b.append((person + bytes([outlen]), msg, n, hashlib.blake2b(msg, digest_size=outlen, person=person).digest()))
        key = rng.randbytes(32)
        poly.append((key, msg, n, pynote.poly1305(key, msg)))
    for key in (b"\xff" * 32, b"\xff" * 16 + bytes(16)):           # r at its clamped maximum, blocks of all ones: the widest limbs
        for msg in (b"\xff" * 16, b"\xff" * 128, b"\xff" * 17, b"\xfb" + b"\xff" * 15 + b"\xff" * 16):
            poly.append((key, msg, len(msg), pynote.poly1305(key, msg)))
    for counter in (0, 1, 2, 0xffffffff):
        key, nonce = rng.randbytes(32), (bytes(12) if counter < 2 else rng.randbytes(12))
        cc.append((key, counter.to_bytes(4, "little") + nonce, 0, pynote.chacha20_block(key, counter, nonce)))
    # RFC 8439 2.3.2
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    cc.append((key, (1).to_bytes(4, "little") + nonce, 0, bytes.fromhex(
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")))
    return b2b, cc, poly


def _check(gpu):
    b2b, cc, poly = _cases()
    got = S.run(0, [c[:3] for c in b2b], gpu)
    assert [g[:len(c[3])] for g, c in zip(got, b2b)] == [c[3] for c in b2b]
    got = S.run(1, [c[:3] for c in cc], gpu)
    assert got == [c[3] for c in cc]
    got = S.run(2, [c[:3] for c in poly], gpu)
    assert [g[:16] for g in got] == [c[3] for c in poly]


def test_device_headers_on_the_host():
    _check(False)


@pytest.mark.gpu
def test_device_headers_on_the_device():
    _check(True)
