"""Compact (ZIP 307) batch trial decryption of Sapling notes on the GPU (masp_hip_sapling_compact_trial_decrypt, k_note_scan_compact.hip)
through the C ABI, against the host path (libmasp_host.so) run over the same pairs and the reference's ten vectors.  Every test is built
from a full-scan input of which the compact form takes enc[:, :84].  Every comparison is of bytes."""
import random

import numpy as np
import pytest

import compact_notes as CN
import masp_amd
from masp_amd import host as H
from masp_amd import note_encryption as NE

pytestmark = pytest.mark.gpu

VECTORS, ASSET, RJ = CN.VECTORS, CN.ASSET, CN.RJ


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def host_result(ivks, epks, cmus, encs, lead_byte):
    """(the batch answer per output, the candidate count) of the host path over every pair"""
    hit, pts, pks, cand = H.sapling_try_compact_note_decryption_batch(np.frombuffer(b"".join(ivks), np.uint8), epks, cmus, encs[:, :84],
                                                                      lead_byte=lead_byte)
    return [None if k < 0 else (NE._parse_compact(pts[o].tobytes(), pks[o].tobytes()), int(k)) for o, k in enumerate(hit.tolist())], cand


def gpu_result(ctx, ivks, epks, cmus, encs, lead_byte):
    outs = [NE.CompactShieldedOutput(e.tobytes(), c.tobytes(), x[:84].tobytes()) for e, c, x in zip(epks, cmus, encs)]
    return NE.batch.try_compact_note_decryption(ivks, outs, ctx, lead_byte=lead_byte)


def host_status(epks):
    L = H.load_library()
    buf = bytes(64)
    return [0 if L.masp_host_point_uv(e.tobytes(), buf) == 0 else 1 for e in epks]


def test_the_vectors_as_one_call(ctx):
    ivks = [tv["ivk"] for tv in VECTORS]
    epks, cmus, encs = CN.rows_to_arrays([(tv["epk"], tv["cmu"], tv["c_enc"]) for tv in VECTORS])
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 1)
    assert status.tolist() == [0] * 10
    assert ho.tolist() == list(range(10)) and hi.tolist() == list(range(10))
    assert [p.tobytes() for p in hp] == [tv["p_enc"][:84] for tv in VECTORS]
    assert [p.tobytes() for p in hk] == [tv["default_pk_d"] for tv in VECTORS]
    assert cand >= 10
    got = gpu_result(ctx, ivks, epks, cmus, encs, 1)
    for i, tv in enumerate(VECTORS):
        note = NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"]))
        assert got[i] == ((note, NE.PaymentAddress(tv["default_d"], tv["default_pk_d"])), i)
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 2)
    assert status.tolist() == [0] * 10 and len(ho) == 0
    assert gpu_result(ctx, ivks, epks, cmus, encs, 2) == [None] * 10


def _scan(ctx, n, n_ivk, places, seed, against_host=True):
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    epks, cmus, encs = CN.noise(n, seed)
    want_pairs, want_notes = [], {}
    for j, o in enumerate(places):
        k = j % n_ivk
        out, note, to = CN.planted(ivks_int[k], seed * 1000 + j)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
        want_pairs.append((o, k, NE.note_plaintext_bytes(note, to)[:84], to.pk_d))
        want_notes[o] = ((note, to), k)
    want_pairs.sort()
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 2)
    assert [1 if s else 0 for s in status.tolist()] == host_status(epks)
    assert 0 < sum(1 for s in status.tolist() if s) < n            # both kinds are in the batch
    # the hits: the planted pairs, no other pair, sorted, each with its plaintext and pk_d
    assert list(zip(ho.tolist(), hi.tolist(), (p.tobytes() for p in hp), (p.tobytes() for p in hk))) == want_pairs
    got = gpu_result(ctx, ivks, epks, cmus, encs, 2)
    assert got == [want_notes.get(o) for o in range(n)]
    if not against_host:
        return cand
    # the whole result list and the candidate count against the host path over every pair
    want, want_cand = host_result(ivks, epks, cmus, encs, 2)
    assert [i for i, w in enumerate(want) if w is not None] == sorted(places)
    assert got == want
    print("candidates: device %d, host %d, planted %d" % (cand, want_cand, len(places)))
    assert cand == want_cand
    return cand


def test_noise_with_planted_notes(ctx):
    """3 109 outputs x 8 ivks: about half of the 24 872 pairs decode and one in 256 of those passes the byte test, so about 48 pairs of noise
    are candidates that stage 2 has to refuse (seed 41, counted by the host batch function: 83 candidates, of which 48 are planted)"""
    n = 3 * 1024 + 37          # not a multiple of the block
    places = [0, 1, 63, 64, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 3071, 3072, n - 2, n - 1] + random.Random(31).sample(range(1100, 3000), 32)
    assert len(set(places)) == len(places)
    cand = _scan(ctx, n, 8, places, 41)
    assert cand > len(places)


def test_scan_over_several_chunks(ctx):
    """32 ivks: 8 192 outputs per launch, so 16 484 outputs are three chunks (both buffer sets, the first one twice); notes at the chunks' edges"""
    n = 2 * 8192 + 100
    places = [0, 8191, 8192, 8193, 16383, 16384, n - 1] + random.Random(32).sample(range(100, 16000), 33)
    assert len(set(places)) == len(places)
    # (the planted pairs with their bytes, and no other pair; the host path over these 527 488 pairs would take ten seconds and is what
    # test_noise_with_planted_notes compares with)
    cand = _scan(ctx, n, 32, places, 42, against_host=False)
    assert cand > len(places)


@pytest.mark.parametrize("n", [2 * 8192, 3 * 8192 + 1])
def test_scan_ends_on_a_chunk_boundary_or_one_output_behind_it(ctx, n):
    """32 ivks, 8 192 outputs per chunk.  16 384 outputs: the call ends exactly where the second chunk does, no empty third one.  24 577: four
    chunks, both buffer sets used twice, the last chunk a single output.  Notes at every chunk's first and last output; the statuses of every
    output and the hits (the planted pairs with their plaintexts and pk_d, and no other pair)"""
    places = sorted({0, 8191, 8192, n - 1} | ({16383, 16384, 24575, 24576} if n > 3 * 8192 else set()))
    cand = _scan(ctx, n, 32, places, 46, against_host=False)
    assert cand > len(places)


def test_every_pair_a_candidate_and_a_hit(ctx):
    rng = random.Random(43)
    ivk, other = rng.randrange(1, RJ), rng.randrange(1, RJ)
    n = 300
    made = [CN.planted(ivk, 4300 + i) for i in range(n)]
    epks, cmus, encs = CN.rows_to_arrays([m[0] for m in made])
    b = ivk.to_bytes(32, "little")
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b, epks, cmus, encs[:, :84], 2)
    assert ho.tolist() == list(range(n)) and hi.tolist() == [0] * n and cand == n      # every pair of the launch a candidate
    ivks = [other.to_bytes(32, "little"), b, b]
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 2)
    assert list(zip(ho.tolist(), hi.tolist())) == [(o, k) for o in range(n) for k in (1, 2)]
    assert hp[0::2].tobytes() == hp[1::2].tobytes() == b"".join(NE.note_plaintext_bytes(m[1], m[2])[:84] for m in made)
    assert hk[0::2].tobytes() == hk[1::2].tobytes() == b"".join(m[2].pk_d for m in made)
    got = gpu_result(ctx, ivks, epks, cmus, encs, 2)
    want, want_cand = host_result(ivks, epks, cmus, encs, 2)
    assert got == want and [g[1] for g in got] == [1] * n and cand == want_cand
    # too little room: an error and the needed count, nothing written
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 2, hit_capacity=2 * n - 1)
    assert e.value.code == 10 and e.value.needed == 2 * n == 600
    L = masp_amd.load_library()
    import ctypes as C
    ho2, hi2, hp2, hk2 = np.full(599, 7, np.uint32), np.full(599, 7, np.uint32), np.full((599, 84), 7, np.uint8), np.full((599, 32), 7, np.uint8)
    nh = C.c_size_t(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    iv = np.frombuffer(b"".join(ivks), np.uint8)
    x84 = np.ascontiguousarray(encs[:, :84])
    rc = L.masp_hip_sapling_compact_trial_decrypt(ctx._h, 3, p(iv), n, p(epks), p(cmus), p(x84), 2, None, 599, p(ho2), p(hi2), p(hp2), p(hk2),
                                                  C.byref(nh), None)
    assert rc == 10 and nh.value == 600
    assert (ho2 == 7).all() and (hi2 == 7).all() and (hp2 == 7).all() and (hk2 == 7).all()
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], 2, hit_capacity=2 * n)
    assert len(ho) == 2 * n


def test_near_misses_in_one_batch(ctx):
    """every near miss of the host file next to honest notes of both lead bytes and outputs with an epk of small order, whose one key serves
    every ivk: candidates of several ivks from one output, in one wave"""
    rng = random.Random(44)
    ivks_int = [0, 1, RJ - 1, rng.randrange(1, RJ)]
    ivks = [k.to_bytes(32, "little") for k in ivks_int]
    rows = [m[1] for m in CN.near_misses(ivks_int[3], 44)] + CN.small_order_rows(ivks_int[3], 4400)
    rows += [CN.planted(ivks_int[2], 4410)[0], CN.planted(ivks_int[1], 4411)[0], CN.planted(ivks_int[3], 4412, 1)[0], CN.planted(ivks_int[2], 4413, 1)[0]]
    rng.shuffle(rows)
    epks, cmus, encs = CN.rows_to_arrays(rows)
    for lead in (1, 2):
        want, want_cand = host_result(ivks, epks, cmus, encs, lead)
        status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"".join(ivks), epks, cmus, encs[:, :84], lead)
        assert [1 if s else 0 for s in status.tolist()] == host_status(epks)
        assert cand == want_cand
        # the small-order outputs with this lead byte: a candidate for each of the four ivks
        assert want_cand >= 4 * 2 + 2
        assert gpu_result(ctx, ivks, epks, cmus, encs, lead) == want
        assert sum(w is not None for w in want) >= 3          # the honest notes
        # every hit is a pair the single host form accepts, with its bytes
        for o, k, pt, pk in zip(ho.tolist(), hi.tolist(), hp, hk):
            assert H.sapling_try_compact_note_decryption(ivks[k], epks[o].tobytes(), cmus[o].tobytes(), encs[o, :84].tobytes(), lead) == \
                (pt.tobytes(), pk.tobytes())


def test_an_ivk_at_or_above_the_group_order_is_refused(ctx):
    """1 ivk x 1 output.  r_J, r_J + 1, r_J with its top word one higher (every lower word equal) and 2^256 - 1 are no SaplingIvk: the
    host library refuses each, and so does the call, with MASP_HIP_E_INVALID_ARG.  (r_J - 1 is one: test_near_misses_in_one_batch.)"""
    tv = VECTORS[0]
    epk, cmu, enc = (np.frombuffer(tv[f], np.uint8) for f in ("epk", "cmu", "c_enc"))
    enc = enc[:84].copy()
    for k in (RJ, RJ + 1, RJ + (1 << 224), (1 << 256) - 1):
        ivk = k.to_bytes(32, "little")
        with pytest.raises(H.HostError):
            H.sapling_try_compact_note_decryption_batch([ivk], [tv["epk"]], [tv["cmu"]], [tv["c_enc"][:84]], lead_byte=1, threads=1)
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.sapling_compact_trial_decrypt(ivk, epk, cmu, enc, 1)
        assert e.value.code == 1, k


def test_arguments(ctx):
    tv = VECTORS[0]
    epk, cmu, enc = (np.frombuffer(tv[f], np.uint8) for f in ("epk", "cmu", "c_enc"))
    enc = enc[:84].copy()
    for k in (RJ, RJ + 1, (1 << 256) - 1):
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.sapling_compact_trial_decrypt(tv["ivk"] + k.to_bytes(32, "little"), epk, cmu, enc, 1)
        assert e.value.code == 1
    for lead in (0, 3, -1, 256 + 1):
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.sapling_compact_trial_decrypt(tv["ivk"], epk, cmu, enc, lead)
        assert e.value.code == 1
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(b"", epk, cmu, enc, 1)
    assert len(ho) == 0 and status.tolist() == [0] and cand == 0
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(tv["ivk"], b"", b"", b"", 1)
    assert len(ho) == 0 and len(status) == 0 and cand == 0
    out = NE.CompactShieldedOutput(tv["epk"], tv["cmu"], tv["c_enc"][:84])
    assert NE.batch.try_compact_note_decryption([], [out], ctx, lead_byte=1) == [None]
    assert NE.batch.try_compact_note_decryption([tv["ivk"]], [], ctx, lead_byte=1) == []
    status, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(tv["ivk"], epk, cmu, enc, 1, count_candidates=False)      # n_candidates = NULL
    assert ho.tolist() == [0] and hp[0].tobytes() == tv["p_enc"][:84] and cand is None
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.sapling_compact_trial_decrypt(tv["ivk"], epk, cmu, enc, 1, hit_capacity=0)
    assert e.value.code == 10 and e.value.needed == 1


def test_the_full_scan_is_unchanged(ctx):
    """the two scans share the streams, WalletState::mu and the decode buffers: a full scan gives the same bytes before and after a compact one"""
    rng = random.Random(45)
    ivks_int = [rng.randrange(1, RJ) for _ in range(3)]
    ivks = b"".join(k.to_bytes(32, "little") for k in ivks_int)
    epks, cmus, encs = CN.noise(700, 45)
    for j, o in enumerate((0, 255, 256, 699)):
        out, _, _ = CN.planted(ivks_int[j % 3], 4500 + j)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
    before = ctx.sapling_trial_decrypt(ivks, epks, encs)
    assert list(zip(before[1].tolist(), before[2].tolist())) == [(0, 0), (255, 1), (256, 2), (699, 0)]
    compact = ctx.sapling_compact_trial_decrypt(ivks, epks, cmus, encs[:, :84], 2)
    assert list(zip(compact[1].tolist(), compact[2].tolist())) == [(0, 0), (255, 1), (256, 2), (699, 0)]
    after = ctx.sapling_trial_decrypt(ivks, epks, encs)
    assert [a.tobytes() for a in after] == [b.tobytes() for b in before]
    assert [k.tobytes() for k in after[3]] == [H.kdf_sapling(H.sapling_ka_agree(ivks[32 * k:32 * k + 32], epks[o].tobytes()), epks[o].tobytes())
                                              for o, k in zip(after[1].tolist(), after[2].tolist())]
