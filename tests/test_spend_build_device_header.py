"""device/spend_build.hpp on the CPU (the header is __host__ __device__; tests/native/spend_build_dev.hip through spend_build_shim): every
stage of the signatures and of the spend descriptions against spend_build_ref, the fixed-base multiplication on each of the three tables,
the wide reduction and S = r + c rsk at their edges against Python integers, and the secrets gone from the state after the last stage.
CPU only; every comparison is of bytes or of integers."""
import random

import numpy as np

import spend_build_ref as R
import spend_build_shim as S
from masp_amd import host as H

RJ = R.RJ


def test_fixed_base_mul_on_each_table_at_the_edge_scalars():
    for table, g in (("spend", R.G_SPEND), ("pgk", R.G_PGK), ("vcr", R.G_VCR)):
        for k in R.EDGE_SCALARS + (random.Random(3).randrange(RJ),):
            assert S.table_mul(table, k) == H.jubjub_mul(g, R._le(k)), (table, hex(k))
        assert S.table_mul(table, 0) == H.JUBJUB_IDENTITY
    for v in R.key_vectors():       # ... and the reference's key vectors, through the tables
        assert S.table_mul("spend", R._int(bytes.fromhex(v["ask"]))) == bytes.fromhex(v["ak"])
        assert S.table_mul("pgk", R._int(bytes.fromhex(v["nsk"]))) == bytes.fromhex(v["nk"])


def test_wide_reduction_at_its_edges():
    top = (1 << 512) // RJ
    values = [0, RJ - 1, RJ, RJ + 1, (1 << 256) - 1, 1 << 256, (1 << 256) + 1, (1 << 512) - 1, (RJ - 1) << 256, RJ << 256, ((1 << 256) - 1) << 256]
    values += [k * RJ + d for k in (1, 2, 16, (1 << 256) // RJ, (1 << 256) // RJ + 1, top // 2, top - 1, top) for d in (-1, 0, 1) if k * RJ + d < 1 << 512]
    rng = random.Random(11)
    values += [rng.getrandbits(512) for _ in range(200)]
    for x in values:
        assert S.reduce_wide(x) == x % RJ, hex(x)


def test_s_with_wraparound_and_zero_keys():
    rng = random.Random(12)
    cases = [(RJ - 1, RJ - 1, RJ - 1), (5, 7, 0), (0, 0, 0), (RJ - 1, 0, RJ - 1), (0, RJ - 1, 1), (1, 1, RJ - 1)]
    cases += [tuple(rng.randrange(RJ) for _ in range(3)) for _ in range(50)]
    for r, c, k in cases:
        assert S.mul_add(r, c, k) == (r + c * k) % RJ, (r, c, k)


def _words(part, n, size, at, count=8):
    """bytes [at, at + 4 count) of each of the first n state items"""
    return [part[i * size + at:i * size + at + 4 * count].tobytes() for i in range(n)]


def test_every_signing_stage_against_the_reference():
    edge, edge_want = R.references("edge_items", R.edge_items, R.sign_reference)
    rnd, rnd_want = R.sign_batch(24)
    items, want = edge + rnd, edge_want + rnd_want
    n = len(items)
    assert {w[0] for w in want} == {0, 1, 2}
    arrays = R.sign_arrays(items)
    good = [i for i, w in enumerate(want) if w[0] == 0]
    rsk = [(R._int(it["sk"]) + R._int(it["alpha"] or bytes(32))) % RJ for it in items]
    assert 0 in [rsk[i] for i in good]                      # sk + alpha at exactly r_J
    block = S.sign.stage_host(1, arrays, S.sign.new_block(n))
    state, size = S.sign.parts(block, n)
    state = state["state"]
    assert size == 132
    assert [int.from_bytes(s, "little") for s in _words(state, n, size, 128, 1)] == [w[0] for w in want]
    assert [_words(state, n, size, 0)[i] for i in good] == [R._le(rsk[i]) for i in good]
    assert [_words(state, n, size, 64)[i] for i in good] == [want[i][1] for i in good]
    block = S.sign.stage_host(2, arrays, block)
    state = S.sign.parts(block, n)[0]["state"]
    assert [_words(state, n, size, 32)[i] for i in good] == [R._le(R.h_star(items[i]["T"], want[i][1], items[i]["sighash"])) for i in good]
    block = S.sign.stage_host(3, arrays, block)
    state = S.sign.parts(block, n)[0]["state"]
    assert [_words(state, n, size, 96)[i] for i in good] == [want[i][2][:32] for i in good]
    block = S.sign.stage_host(4, arrays, block)
    R.check_signs(S.sign_results(block, n), want)
    state = S.sign.parts(block, n)[0]["state"]
    assert not any(any(s) for s in _words(state, n, size, 0, 16))          # rsk and r are gone from the state
    # all four at once, and without alphas
    R.check_signs(S.sign_results(S.sign.stage_host(0, arrays, S.sign.new_block(n)), n), want)
    plain = [R.good_item(1800 + i, alpha=False) for i in range(3)]
    R.check_signs(S.sign_results(S.sign.stage_host(0, R.sign_arrays(plain, alphas=False), S.sign.new_block(3)), 3), [R.sign_reference(it) for it in plain])


def test_every_spend_stage_against_the_reference():
    cases = R.status_spends()
    spends = [p for b, bad, _ in cases for p in (b, bad)] + [d for d, _ in R.double_spends()] + R.references("edge_spends", R.edge_spends)[0][:9]
    want = [R.reference(p) for p in spends]
    n = len(spends)
    assert {w[0] for w in want} == set(range(10))
    arrays = R.arrays(spends)
    good = [i for i, w in enumerate(want) if w[0] == 0]
    block = S.spend.stage_host(2, arrays, S.spend.stage_host(1, arrays, S.spend.new_block(n)))
    state, size = S.spend.parts(block, n)
    state = state["state"]
    assert [_words(state, n, size, size - 72)[i] for i in good] == [want[i][5] for i in good]       # nk
    assert [_words(state, n, size, size - 40)[i] for i in good] == [want[i][2] for i in good]       # rk
    block = S.spend.stage_host(3, arrays, block)
    p = S.spend.parts(block, n)[0]
    assert p["status"][:n].tolist() == [w[0] for w in want]
    assert [p["cmu"][32 * i:32 * i + 32].tobytes() for i in range(n)] == [w[4] for w in want]
    assert not p["cv"].any() and not p["nf"].any()
    block = S.spend.stage_host(4, arrays, block)
    p = S.spend.parts(block, n)[0]
    for f, k in (("cv", 1), ("rk", 2), ("nk", 5)):
        assert [p[f][32 * i:32 * i + 32].tobytes() for i in range(n)] == [w[k] for w in want], f
    assert not p["nf"].any()
    block = S.spend.stage_host(5, arrays, block)
    R.check(S.spend_results(block, n), want)
    R.check(S.spend_results(S.spend.stage_host(0, arrays, S.spend.new_block(n)), n), want)
