"""Batch output recovery with outgoing viewing keys on the GPU (masp_hip_sapling_output_recovery_scan, k_out_recovery.hip) through the
C ABI, against the host path (libmasp_host.so) run over the same pairs and the reference's ten vectors.  Every comparison is of bytes."""
import json
import os
import random

import numpy as np
import pytest

import masp_amd
import out_recovery_cases as K
from masp_amd import host as H
from masp_amd import note_encryption as NE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DOC = json.load(open(os.path.join(HERE, "golden", "note_encryption_vectors.json")))
VECTORS = [{k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in tv.items()} for tv in DOC["vectors"]]
ASSET = bytes.fromhex(DOC["asset_identifier"])
FIELDS = ("cv", "cmu", "epk", "enc_ciphertext", "out_ciphertext")


@pytest.fixture(scope="module")
def ctx():
    c = masp_amd.Context(0)
    yield c
    c.close()


def noise(n, seed):
    """n outputs of random bytes, as a dict of arrays"""
    rng = np.random.default_rng(seed)
    return {f: rng.integers(0, 256, (n, w), dtype=np.uint8) for f, w in zip(FIELDS, (32, 32, 32, 612, 80))}


def put(rows, o, output):
    for f in FIELDS:
        rows[f][o] = np.frombuffer(getattr(output, f), np.uint8)


def rows_of(outputs):
    return {f: np.frombuffer(b"".join(getattr(o, f) for o in outputs), np.uint8).reshape(len(outputs), -1).copy() for f in FIELDS}


def outputs_of(rows):
    return [NE.OutputDescription(*(rows[f][o].tobytes() for f in FIELDS)) for o in range(len(rows["cv"]))]


def scan(ctx, ovks, rows, **kw):
    ho, hk, ocks = ctx.sapling_output_recovery_scan(b"".join(ovks), rows["cv"], rows["epk"], rows["cmu"], rows["out_ciphertext"], **kw)
    return list(zip(ho.tolist(), hk.tolist(), (k.tobytes() for k in ocks)))


def host_result(ovks, rows, lead_byte):
    hit, pts, pks = H.sapling_try_output_recovery_batch(list(ovks), rows["cv"], rows["epk"], rows["cmu"], rows["enc_ciphertext"],
                                                        rows["out_ciphertext"], lead_byte=lead_byte)
    return [None if k < 0 else (NE._parse(pts[o].tobytes(), pks[o].tobytes()), int(k)) for o, k in enumerate(hit.tolist())]


def gpu_result(ctx, ovks, rows, lead_byte):
    return NE.batch.try_output_recovery(ovks, outputs_of(rows), ctx, lead_byte=lead_byte)


def test_the_vectors_as_one_call(ctx):
    ovks = [tv["ovk"] for tv in VECTORS]
    outs = [NE.OutputDescription(tv["cv"], tv["cmu"], tv["epk"], tv["c_enc"], tv["c_out"]) for tv in VECTORS]
    assert scan(ctx, ovks, rows_of(outs)) == [(i, i, tv["ock"]) for i, tv in enumerate(VECTORS)]
    got = NE.batch.try_output_recovery(ovks, outs, ctx, lead_byte=1)
    for i, tv in enumerate(VECTORS):
        note = NE.Note(ASSET, tv["v"], tv["default_pk_d"], NE.Rseed(1, tv["rcm"]))
        assert got[i] == ((note, NE.PaymentAddress(tv["default_d"], tv["default_pk_d"]), tv["memo"]), i)
    assert NE.batch.try_output_recovery(ovks, outs, ctx, lead_byte=2) == [None] * 10


def _scan(ctx, n, n_ovk, places, seed, against_host=True):
    rng = random.Random(seed)
    ovks = [rng.randbytes(32) for _ in range(n_ovk)]
    rows = noise(n, seed)
    want_pairs = []
    for j, o in enumerate(places):
        k = j % n_ovk
        s = K.Sent(ovks[k], ASSET, seed * 1000 + j)
        put(rows, o, s.output)
        want_pairs.append((o, k, H.prf_ock(ovks[k], s.output.cv, s.output.cmu, s.output.epk)))
    want_pairs.sort()
    # the raw hits: the planted pairs, no other pair, sorted, each with the host's ock
    assert scan(ctx, ovks, rows) == want_pairs
    if not against_host:
        return
    # the whole result list against the host path over every pair
    want = host_result(ovks, rows, 2)
    assert [i for i, w in enumerate(want) if w is not None] == sorted(places)
    assert gpu_result(ctx, ovks, rows, 2) == want


def test_scan_with_planted_notes(ctx):
    n = 3 * 1024 + 37          # not a multiple of the block
    places = [0, 1, 63, 64, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 3071, 3072, n - 2, n - 1] + random.Random(51).sample(range(1100, 3000), 32)
    assert len(set(places)) == len(places) == 48
    _scan(ctx, n, 8, places, 61)
    up, kern = ctx.out_recovery_last_timing()
    assert up > 0 and kern > 0


def test_scan_over_several_chunks(ctx):
    """32 ovks: 8 192 outputs per launch, so 16 484 outputs are three chunks (both buffer sets, the first one twice); notes at the chunks' edges"""
    n = 2 * 8192 + 100
    places = [0, 8191, 8192, 8193, 16383, 16384, n - 1] + random.Random(52).sample(range(100, 16000), 9)
    assert len(set(places)) == len(places)
    _scan(ctx, n, 32, places, 62)


@pytest.mark.parametrize("n", [2 * 8192, 3 * 8192 + 1])
def test_scan_ends_on_a_chunk_boundary_or_one_output_behind_it(ctx, n):
    """32 ovks, 8 192 outputs per chunk.  16 384 outputs: the call ends exactly where the second chunk does, no empty third one.  24 577: four
    chunks, both buffer sets used twice, the last chunk a single output.  Notes at every chunk's first and last output; the raw hits (the
    planted pairs with the host's ocks, and no other pair; the host path over all 786 464 pairs is left to the smaller tests)"""
    places = sorted({0, 8191, 8192, n - 1} | ({16383, 16384, 24575, 24576} if n > 3 * 8192 else set()))
    _scan(ctx, n, 32, places, 66, against_host=False)


def test_every_pair_a_hit(ctx):
    rng = random.Random(63)
    ovk, other = rng.randbytes(32), rng.randbytes(32)
    n = 300
    rows = rows_of([K.Sent(ovk, ASSET, 6300 + i).output for i in range(n)])
    assert [h[:2] for h in scan(ctx, [ovk], rows)] == [(o, 0) for o in range(n)]
    # the same ovk listed twice (and a stranger in front): every pair of the two hits, the first index is reported
    ovks = [other, ovk, ovk]
    hits = scan(ctx, ovks, rows)
    assert [h[:2] for h in hits] == [(o, k) for o in range(n) for k in (1, 2)]
    assert [h[2] for h in hits[0::2]] == [h[2] for h in hits[1::2]]
    got = gpu_result(ctx, ovks, rows, 2)
    assert got == host_result(ovks, rows, 2) and [g[1] for g in got] == [1] * n
    # too little room: an error and the needed count, nothing dropped silently
    with pytest.raises(masp_amd.MaspHipError) as e:
        scan(ctx, ovks, rows, hit_capacity=2 * n - 1)
    assert e.value.code == 10 and e.value.needed == 2 * n
    assert len(scan(ctx, ovks, rows, hit_capacity=2 * n)) == 2 * n


def test_tag_verifies_and_the_reference_refuses(ctx):
    """the crafted rows of the host tests (subgroup, esk, ZIP 212, cmu, ...) beside honest notes of both lead bytes: every one of them is a
    hit on the device, and what becomes of it is the host's answer"""
    rng = random.Random(64)
    mine, stranger = rng.randbytes(32), rng.randbytes(32)
    s = K.Sent(mine, ASSET, 65)
    controls, refused = K.crafted(s, 66)
    outs = [o for _, o in refused] + [o for _, o in controls] + [K.Sent(mine, ASSET, 67, 1).output, K.Sent(stranger, ASSET, 68).output,
                                                                 K.Sent(None, ASSET, 69).output, K.Sent(mine, ASSET, 70).output]
    rows = rows_of(outs)
    ovks = [stranger, mine]
    hits = scan(ctx, ovks, rows)
    n_mine = len(refused) + len(controls)
    assert [h[:2] for h in hits] == [(o, 1) for o in range(n_mine + 1)] + [(n_mine + 1, 0), (n_mine + 3, 1)]
    assert [h[2] for h in hits] == [H.prf_ock(ovks[k], outs[o].cv, outs[o].cmu, outs[o].epk) for o, k, _ in hits]
    for lead in (1, 2):
        want = host_result(ovks, rows, lead)
        assert gpu_result(ctx, ovks, rows, lead) == want
        assert [i for i, w in enumerate(want) if w] == ([n_mine] if lead == 1 else [len(refused), len(refused) + 1, n_mine + 1, n_mine + 3])


def test_arguments(ctx):
    tv = VECTORS[0]
    rows = rows_of([NE.OutputDescription(tv["cv"], tv["cmu"], tv["epk"], tv["c_enc"], tv["c_out"])])
    empty = {f: np.zeros((0, r.shape[1]), np.uint8) for f, r in rows.items()}
    assert scan(ctx, [], rows) == []
    assert scan(ctx, [tv["ovk"]], empty) == []
    assert NE.batch.try_output_recovery([], outputs_of(rows), ctx) == [None]
    assert NE.batch.try_output_recovery([tv["ovk"]], [], ctx) == []
    with pytest.raises(masp_amd.MaspHipError) as e:
        scan(ctx, [tv["ovk"]], rows, hit_capacity=0)
    assert e.value.code == 10 and e.value.needed == 1
    # a null context: refused, not dereferenced
    import ctypes as C
    L = ctx._L
    nh = C.c_size_t(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ovk = np.frombuffer(tv["ovk"], np.uint8).copy()
    assert L.masp_hip_sapling_output_recovery_scan(None, 1, p(ovk), 1, p(rows["cv"]), p(rows["epk"]), p(rows["cmu"]), p(rows["out_ciphertext"]), 0,
                                                   None, None, None, C.byref(nh)) == 1
    assert L.masp_hip_out_recovery_last_timing(None, (C.c_double * 2)()) == 1


def test_the_device_header_on_the_device():
    """device/out_recovery.hpp's pair function in a kernel of its own against its host leg and the host library"""
    import test_output_recovery_host as T
    T.check_pair_function(K.Sent(random.Random(70).randbytes(32), ASSET, 71), True)
