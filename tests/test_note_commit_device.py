"""The compact note scan's device headers on their own (masp_amd/csrc/device/blake2s.hpp, group_hash.hpp, pedersen.hpp, and the four steps
of stage 2 in compact_note.hpp) against hashlib, Python integers and the host library: compiled for the host, and in a kernel.  Every comparison is of bytes."""
import functools
import hashlib
import random

import pytest

import compact_notes as CN
import note_commit_shim as S
from masp_amd import host as H

RJ = H.JUBJUB_ORDER


@functools.lru_cache(maxsize=None)
def _cases():
    """per op: [(head, message, length, the 64 result bytes to expect or their prefix)]; computed once for both halves"""
    rng = random.Random(51)
    b2s = []
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 75, 127, 128):
        for person in (b"MASP__gd", b"MASP__v_", rng.randbytes(8)):
            msg = rng.randbytes(n)
            b2s.append((person, msg, n, hashlib.blake2s(msg, person=person).digest()))
    gd = []
    for _ in range(24):
        d = rng.randbytes(11)
        try:
            gd.append((b"", d, 11, H.diversifier_base(d) + b"\x01"))
        except H.HostError:
            gd.append((b"", d, 11, bytes(33)))
    assert 4 <= sum(c[3][32] for c in gd) <= 20          # some exist, some must fail
    ag = []
    for i in range(24):
        ident = rng.randbytes(32) if i else H.asset_identifier(b"benchmark")
        try:
            ag.append((b"", ident, 32, H.asset_generator(ident) + b"\x01\x01"))
        except ValueError:
            ag.append((b"", ident, 32, bytes(34)))
    assert 4 <= sum(c[3][32] for c in ag) <= 20
    cm = []
    idents = [c[1] for c in ag if c[3][32]]
    divs = [c[1] for c in gd if c[3][32]]
    for value in (0, (1 << 64) - 1, rng.randrange(1 << 64)):
        for rcm in (0, RJ - 1, rng.randrange(RJ)):
            ident, d = rng.choice(idents), rng.choice(divs)
            pk_d = H.jubjub_mul(H.diversifier_base(d), rng.randrange(1, RJ).to_bytes(32, "little"))
            rcm = rcm.to_bytes(32, "little")
            msg = ident + value.to_bytes(8, "little") + d + b"\x00" + pk_d + rcm
            cm.append((b"", msg, len(msg), H.note_cmu(ident, value, d, pk_d, rcm) + b"\x01"))
    # an identifier / a diversifier without a point: no commitment
    bad_id, bad_d = next(c[1] for c in ag if not c[3][32]), next(c[1] for c in gd if not c[3][32])
    for ident, d in ((bad_id, divs[0]), (idents[0], bad_d)):
        msg = ident + bytes(8) + d + b"\x00" + bytes(32) + bytes(32)
        cm.append((b"", msg, len(msg), bytes(33)))
    wide = []
    for x in (0, 1, RJ - 1, RJ, RJ + 1, (1 << 512) - 1, (1 << 511), rng.randrange(1 << 512), rng.randrange(1 << 512), rng.randrange(1 << 253)):
        wide.append((b"", x.to_bytes(64, "little"), 64, (x % RJ).to_bytes(32, "little")))
    prf = []
    for domain in (4, 5):
        for rseed in (bytes(32), b"\xff" * 32, rng.randbytes(32), rng.randbytes(32)):
            prf.append((bytes([domain]), rseed, 32, H.sapling_rseed_scalar(rseed, domain)))
    return b2s, gd, ag, cm, wide, prf


@functools.lru_cache(maxsize=None)
def _stage2_cases():
    """candidates for the four steps of stage 2 (device/compact_note.hpp): the near misses of the host file, outputs with an epk of small
    order and honest notes, each under the key its ivk derives -> (items, the 84-byte rows, per item (steps passed, pk_d or None))"""
    rng = random.Random(52)
    ivk = rng.randrange(1, RJ)
    # how far each kind gets: parse, pk_d, the commitment, the esk check
    steps = {"honest": 4, "cmu bit": 2, "asset identifier": 0, "diversifier": 0, "esk": 3, "rcm": 0, "ivk zero": 1}
    items, rows, want = [], [], []
    for name, out, lead, k in CN.near_misses(ivk, 52):
        if name == "epk":
            continue                       # (no key: stage 1 never sees it)
        kb = k.to_bytes(32, "little")
        key = H.kdf_sapling(H.sapling_ka_agree(kb, out.epk), out.epk)
        items.append((bytes([lead]), key + kb + out.epk + out.cmu, 128))
        rows.append(out.enc_ciphertext[:84])
        r = H.sapling_try_compact_note_decryption(kb, out.epk, out.cmu, out.enc_ciphertext[:84], lead)
        assert (r is not None) == (steps[name] == 4)
        want.append((steps[name], r[1] if r else None))
        if name == "honest":               # the other lead byte: refused at the first step
            items.append((bytes([3 - lead]), key + kb + out.epk + out.cmu, 128))
            rows.append(out.enc_ciphertext[:84])
            want.append((0, None))
    others = [0, 1, RJ - 1, ivk]
    for out in CN.small_order_rows(ivk, 5200) + [CN.planted(RJ - 1, 5210)[0], CN.planted(1, 5211, 1)[0]]:
        for k in others:
            for lead in (1, 2):
                kb = k.to_bytes(32, "little")
                key = H.kdf_sapling(H.sapling_ka_agree(kb, out.epk), out.epk)
                items.append((bytes([lead]), key + kb + out.epk + out.cmu, 128))
                rows.append(out.enc_ciphertext[:84])
                r = H.sapling_try_compact_note_decryption(kb, out.epk, out.cmu, out.enc_ciphertext[:84], lead)
                want.append((4 if r else None, r[1] if r else None))
    assert sum(w[0] == 4 for w in want) >= 6
    return items, rows, want


def _check_stage2(gpu):
    items, rows, want = _stage2_cases()
    got = S.run(6, items, gpu, extra=rows)
    for g, (steps, pk_d), item in zip(got, want, items):
        if steps is None:
            assert g[0] < 4, item
        else:
            assert g[0] == steps, (g[0], steps, item)
        if pk_d is not None:
            assert g[1:33] == pk_d


def _check(gpu):
    for op, cases in enumerate(_cases()):
        got = S.run(op, [c[:3] for c in cases], gpu)
        assert [g[:len(c[3])] for g, c in zip(got, cases)] == [c[3] for c in cases], op


def test_device_headers_on_the_host():
    _check(False)


def test_stage_two_steps_on_the_host():
    _check_stage2(False)


@pytest.mark.gpu
def test_stage_two_steps_on_the_device():
    _check_stage2(True)


@pytest.mark.gpu
def test_device_headers_on_the_device():
    _check(True)
