"""Batch trial decryption of Sapling notes on the GPU (masp_hip_sapling_trial_decrypt, k_note_scan.hip) through the C ABI, against the
host path (libmasp_host.so) run over the same pairs and the reference's ten vectors.  Every comparison is of bytes."""
import json
import os
import random

import numpy as np
import pytest

import masp_amd
import pynote
from masp_amd import host as H
from masp_amd import note_encryption as NE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "note_encryption_vectors.json")))
VECTORS = [{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in tv.items()} for tv in DOC["vectors"]]
ASSET = bytes.fromhex(DOC["asset_identifier"])
RJ = H.JUBJUB_ORDER
NONCE = bytes(12)


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def recipient(ivk, seed):
    rng = random.Random(seed)
    while True:
        d = rng.randbytes(11)
        try:
            gd = H.diversifier_base(d)
        except H.HostError:
            continue
        return NE.PaymentAddress(d, H.jubjub_mul(gd, ivk.to_bytes(32, "little")))


def planted(ivk, seed, lead_byte=2):
    rng = random.Random(seed)
    to = recipient(ivk, seed)
    if lead_byte == 2:
        note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(2, rng.randbytes(32)))
        return NE.sapling_note_encrypt(note, to, rng.randbytes(512)), note, to
    note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(1, rng.randrange(RJ).to_bytes(32, "little")))
    return NE.sapling_note_encrypt(note, to, rng.randbytes(512), esk=rng.randrange(1, RJ).to_bytes(32, "little")), note, to


def noise(n, seed):
    """n outputs of random bytes: about half of the epks decode (the others are reported by status)"""
    rng = np.random.default_rng(seed)
    epks = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    epks[:, 31] &= 0x7f | (rng.integers(0, 2, n, dtype=np.uint8) << 7)
    epks[:, 31] &= 0xbf        # v below 2^254: mostly canonical
    return epks, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 612), dtype=np.uint8)


def host_status(epks):
    """0 if the host decodes the epk (JPoint::from_bytes), else 1"""
    L = H.load_library()
    buf = bytes(64)
    return [0 if L.masp_host_point_uv(e.tobytes(), buf) == 0 else 1 for e in epks]


def host_result(ivks, epks, cmus, encs, lead_byte):
    hit, pts, pks = H.sapling_try_note_decryption_batch(np.frombuffer(b"".join(ivks), np.uint8), epks, cmus, encs, lead_byte=lead_byte)
    return [None if k < 0 else (NE._parse(pts[o].tobytes(), pks[o].tobytes()), int(k)) for o, k in enumerate(hit.tolist())]


def gpu_result(ctx, ivks, epks, cmus, encs, lead_byte):
    outs = [NE.ShieldedOutput(e.tobytes(), c.tobytes(), x.tobytes()) for e, c, x in zip(epks, cmus, encs)]
    return NE.batch.try_note_decryption(ivks, outs, ctx, lead_byte=lead_byte)


def test_the_vectors_as_one_call(ctx):
    ivks = [tv["ivk"] for tv in VECTORS]
    epks = np.frombuffer(b"".join(tv["epk"] for tv in VECTORS), np.uint8).reshape(-1, 32)
    encs = np.frombuffer(b"".join(tv["c_enc"] for tv in VECTORS), np.uint8).reshape(-1, 612)
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
    assert status.tolist() == [0] * 10
    assert ho.tolist() == list(range(10)) and hi.tolist() == list(range(10))
    assert [k.tobytes() for k in hk] == [tv["k_enc"] for tv in VECTORS]
    outs = [NE.ShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"]) for tv in VECTORS]
    got = NE.batch.try_note_decryption(ivks, outs, ctx, lead_byte=1)
    for i, tv in enumerate(VECTORS):
        note = NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"]))
        assert got[i] == ((note, NE.PaymentAddress(tv["default_d"], tv["default_pk_d"]), tv["memo"]), i)
    assert NE.batch.try_note_decryption(ivks, outs, ctx, lead_byte=2) == [None] * 10
    # both settings of the measurement knobs give the same bytes
    try:
        for sd in (0, 1):
            for inv in (0, 1):
                ctx.note_scan_configure(sd, inv)
                s2, o2, i2, k2 = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
                assert (s2.tolist(), o2.tolist(), i2.tolist(), k2.tobytes()) == (status.tolist(), ho.tolist(), hi.tolist(), hk.tobytes()), (sd, inv)
    finally:
        ctx.note_scan_configure(1, 0)      # the defaults


def _scan(ctx, n, n_ivk, places, seed, against_host=True):
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    epks, cmus, encs = noise(n, seed)
    want_pairs = []
    for j, o in enumerate(places):
        k = j % n_ivk
        out, _, _ = planted(ivks_int[k], seed * 1000 + j)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
        want_pairs.append((o, k, H.kdf_sapling(H.sapling_ka_agree(ivks[k], out.epk), out.epk)))
    want_pairs.sort()
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
    assert [1 if s else 0 for s in status.tolist()] == host_status(epks)
    assert 0 < sum(1 for s in status.tolist() if s) < n            # both kinds are in the batch
    # the raw hits: the planted pairs, no other pair, sorted, each with the host's key
    assert list(zip(ho.tolist(), hi.tolist(), (k.tobytes() for k in hk))) == want_pairs
    if not against_host:
        return ivks, epks, cmus, encs
    # the whole result list against the host path over every pair
    want = host_result(ivks, epks, cmus, encs, 2)
    assert [i for i, w in enumerate(want) if w is not None] == sorted(places)
    assert gpu_result(ctx, ivks, epks, cmus, encs, 2) == want
    return ivks, epks, cmus, encs


def test_scan_with_planted_notes(ctx):
    n = 3 * 1024 + 37          # not a multiple of the block
    places = [0, 1, 63, 64, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 3071, 3072, n - 2, n - 1] + random.Random(31).sample(range(1100, 3000), 32)
    assert len(set(places)) == len(places)
    _scan(ctx, n, 8, places, 41)


def test_scan_over_several_chunks(ctx):
    """32 ivks: 8 192 outputs per launch, so 16 484 outputs are three chunks (both buffer sets, the first one twice); notes at the chunks' edges"""
    n = 2 * 8192 + 100
    places = [0, 8191, 8192, 8193, 16383, 16384, n - 1] + random.Random(32).sample(range(100, 16000), 33)
    assert len(set(places)) == len(places)
    _scan(ctx, n, 32, places, 42)


@pytest.mark.parametrize("n", [2 * 8192, 3 * 8192 + 1])
def test_scan_ends_on_a_chunk_boundary_or_one_output_behind_it(ctx, n):
    """32 ivks, 8 192 outputs per chunk.  16 384 outputs: the call ends exactly where the second chunk does, no empty third one.  24 577: four
    chunks, both buffer sets used twice, the last chunk a single output.  Notes at every chunk's first and last output; the statuses of every
    output and the raw hits (the planted pairs with the host's keys, and no other pair; the host path over all 786 464 pairs is left to the
    smaller tests)"""
    places = sorted({0, 8191, 8192, n - 1} | ({16383, 16384, 24575, 24576} if n > 3 * 8192 else set()))
    _scan(ctx, n, 32, places, 46, against_host=False)


def test_every_pair_a_hit(ctx):
    rng = random.Random(43)
    ivk = rng.randrange(1, RJ)
    other = rng.randrange(1, RJ)
    n = 300
    outs = [planted(ivk, 4300 + i)[0] for i in range(n)]
    epks, cmus, encs = (np.frombuffer(b"".join(getattr(o, f) for o in outs), np.uint8).reshape(n, -1) for f in ("epk", "cmu", "enc_ciphertext"))
    b = ivk.to_bytes(32, "little")
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b, epks, encs)
    assert ho.tolist() == list(range(n)) and hi.tolist() == [0] * n
    # the same ivk listed twice (and a stranger in front): every pair of the two hits, the first index is reported
    ivks = [other.to_bytes(32, "little"), b, b]
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
    assert list(zip(ho.tolist(), hi.tolist())) == [(o, k) for o in range(n) for k in (1, 2)]
    assert hk[0::2].tobytes() == hk[1::2].tobytes()
    got = gpu_result(ctx, ivks, epks, cmus, encs, 2)
    assert got == host_result(ivks, epks, cmus, encs, 2) and [g[1] for g in got] == [1] * n
    # too little room: an error and the needed count, nothing dropped silently
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs, hit_capacity=2 * n - 1)
    assert e.value.code == 10 and e.value.needed == 2 * n
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs, hit_capacity=2 * n)
    assert len(ho) == 2 * n


def test_small_order_epk_and_edge_ivks(ctx):
    """epk of small order: [8 ivk] epk is the identity for every ivk, so a ciphertext under kdf(identity, epk) verifies for all of
    them (ivk = 0 and r_J - 1 included), and the final answer is whatever the host path gives.  Non-decoding epks next to them."""
    rng = random.Random(44)
    ivks_int = [0, RJ - 1, rng.randrange(1, RJ), 1]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    ident = (1).to_bytes(32, "little")
    order2 = (H.FR_MODULUS - 1).to_bytes(32, "little")
    rows = []
    for epk in (ident, order2):
        for lead in (1, 2):
            _, note, to = planted(ivks_int[2], 4400 + lead, lead)
            key = pynote.kdf_sapling(ident, epk)
            ct, tag = pynote.aead_encrypt(key, NONCE, NE.note_plaintext_bytes(note, to))
            rows.append((epk, NE.note_cmu(note, to), ct + tag))
    out, _, _ = planted(ivks_int[1], 4410)          # a note of r_J - 1
    rows.append(tuple(out))
    out, _, _ = planted(ivks_int[3], 4411)          # a note of ivk = 1 (pk_d = g_d)
    rows.append(tuple(out))
    bad = [(H.FR_MODULUS + 5).to_bytes(32, "little"), b"\xff" * 32, (1 | (1 << 255)).to_bytes(32, "little")]
    bad.append(next(v.to_bytes(32, "little") for v in range(2, 100) if H.load_library().masp_host_point_uv(v.to_bytes(32, "little"), bytes(64)) != 0))
    for e in bad:
        rows.insert(rng.randrange(len(rows) + 1), (e, rows[0][1], rows[0][2]))
    epks, cmus, encs = (np.frombuffer(b"".join(r[f] for r in rows), np.uint8).reshape(len(rows), -1) for f in range(3))
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"".join(ivks), epks, encs)
    want_status = {bad[0]: 1, bad[1]: 1, bad[2]: 3, bad[3]: 2}
    assert status.tolist() == [want_status.get(r[0], 0) for r in rows]
    hits = list(zip(ho.tolist(), hi.tolist()))
    for o, r in enumerate(rows):
        if r[0] in (ident, order2):
            assert [h for h in hits if h[0] == o] == [(o, k) for k in range(4)]
        elif r[0] in bad:
            assert not [h for h in hits if h[0] == o]
    for lead in (1, 2):
        want = host_result(ivks, epks, cmus, encs, lead)
        assert gpu_result(ctx, ivks, epks, cmus, encs, lead) == want
    assert sum(w is not None for w in host_result(ivks, epks, cmus, encs, 2)) == 2       # the two honest notes; the esk check refuses the rest


def test_an_ivk_at_or_above_the_group_order_is_refused(ctx):
    """1 ivk x 1 output.  r_J, r_J + 1, r_J with its top word one higher (every lower word equal) and 2^256 - 1 are no SaplingIvk: the
    host library refuses each, and so does the call, with MASP_HIP_E_INVALID_ARG.  (r_J - 1 is one: test_small_order_epk_and_edge_ivks.)"""
    tv = VECTORS[0]
    epk, enc = np.frombuffer(tv["epk"], np.uint8), np.frombuffer(tv["c_enc"], np.uint8)
    for k in (RJ, RJ + 1, RJ + (1 << 224), (1 << 256) - 1):
        ivk = k.to_bytes(32, "little")
        with pytest.raises(H.HostError):
            H.sapling_try_note_decryption_batch([ivk], [tv["epk"]], [tv["cmu"]], [tv["c_enc"]], threads=1)
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.sapling_trial_decrypt(ivk, epk, enc)
        assert e.value.code == 1, k


def test_arguments(ctx):
    tv = VECTORS[0]
    epk, enc = np.frombuffer(tv["epk"], np.uint8), np.frombuffer(tv["c_enc"], np.uint8)
    for k in (RJ, RJ + 1, (1 << 256) - 1):
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.sapling_trial_decrypt(tv["ivk"] + k.to_bytes(32, "little"), epk, enc)
        assert e.value.code == 1
    status, ho, hi, hk = ctx.sapling_trial_decrypt(b"", epk, enc)
    assert len(ho) == 0 and status.tolist() == [0]
    status, ho, hi, hk = ctx.sapling_trial_decrypt(tv["ivk"], b"", b"")
    assert len(ho) == 0 and len(status) == 0
    assert NE.batch.try_note_decryption([], [NE.ShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"])], ctx) == [None]
    assert NE.batch.try_note_decryption([tv["ivk"]], [], ctx) == []
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.sapling_trial_decrypt(tv["ivk"], epk, enc, hit_capacity=0)
    assert e.value.code == 10 and e.value.needed == 1
