"""Subset rows behind the MSM window tables (masp_amd/csrc/device/msm_geom.h MsmSubset, device/msm_sort.hpp msm_unit_lanes): an aligned
block of k = 4 / 8 consecutive scalars that are all 0 or 1 becomes ONE entry of bucket 0, the precomputed sum of the block's bases selected
by its bit pattern.  Through the building-block entry points (masp_hip_msm_g1_multi_ex / _g2_multi_ex), bit-exactly against the oracle's
multiexp: G1 and G2, a lone MSM and a batch of nine (the bucket tree in front), 7-bit windows (single-pass k_msm_scatter) and 12-bit windows
(k_msm_partition / k_msm_bucketize), k off / 4 / 8, a covered range that starts at index 0 and at index 5 (not a multiple of k: the merged
h + l table).  n = 301: 37 whole blocks of 8 and a partial one.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import oracle_lib as O
from pyref import R

pytestmark = pytest.mark.gpu

N = 301
NP = 9
EQUAL = (41, 42)        # two equal bases inside one block of 4 (and of 8): a doubling among the block's subset sums
OPPOSITE = (64, 65)     # P and -P inside one block: a subset sums to the point at infinity, the block takes the plain path
BAD_FIRST_INDEX = 64


def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), np.uint8)


def _bases(rng, mul_gen):
    ks = [rng.randrange(1, R) for _ in range(N)]
    ks[EQUAL[1]] = ks[EQUAL[0]]
    ks[OPPOSITE[1]] = R - ks[OPPOSITE[0]]
    return mul_gen(np.stack([_le(k) for k in ks]))


def _scalars(rng):
    """NP vectors of N scalars (as Python ints), blocks numbered in eights"""
    out = []
    for p in range(NP):
        v = [rng.randrange(2) for _ in range(N)]              # random boolean blocks, the trailing partial block (296 .. 300) among them
        if p < 4:
            v[0:8] = [0] * 8                                   # an all-zero block (the other proofs: booleans in front of a range that starts at 5)
        v[8:16] = [1] * 8                                      # all-one blocks: the first covered one when the range starts at 5 ...
        v[16:24] = [1] * 8
        v[24:32] = [0, 1, 0, 0, 1, 1, 0, 1]
        v[35] = rng.randrange(1 << 250, R)                     # a block with one full-width scalar
        v[50] = 2                                              # a block that contains the scalar 2
        v[EQUAL[0]] = v[EQUAL[1]] = 1                          # both equal bases selected
        # the block with P and -P.  Proof 0 (also the lone MSM) and proof 4 select exactly P and -P: the one pattern whose row is the point
        # at infinity for k = 8 and for k = 4 — the result is exact only if the sort leaves the bad block to the plain path
        v[64:72] = [1, 1, 0, 0, 0, 0, 0, 0] if p in (0, 4) else [1, 1, 0, 1, 1, 0, 1, 1] if p % 2 == 0 else [rng.randrange(2) for _ in range(8)]
        if p == 1:
            v = [1] * N                                        # every scalar 1
        if p == 2:
            v[100:140] = [rng.randrange(R) for _ in range(40)]  # blocks without a boolean
        if p == 3:
            v[288:296] = [1] * 8                               # the last whole block of 8
            v[296:301] = [1] * 5
        out.append(v)
    return out


def _digits_of_magnitude_one(s, c):
    """windows of scalar s whose signed c-bit digit is +1 or -1 (MsmDigitIter, device/msm_sort.hpp)"""
    W = (256 + c - 1) // c
    carry, cnt = 0, 0
    for j in range(W):
        v = ((s >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 0
        if v > (1 << (c - 1)):
            v = (1 << c) - v
            carry = 1
        cnt += v == 1
    return cnt


def _bucket0_entries(v, c, bits, lo, hi):
    """the block rule: block b = scalars k b .. k b + k - 1 by absolute index, covered if it lies wholly inside [lo, hi) and no subset of its
    bases sums to the point at infinity; a covered block of scalars that are all 0 or 1 is one entry if it holds a 1.  Every other unit scalar
    is one entry, every other scalar one entry per digit of magnitude 1."""
    k = 1 << bits if bits else 0
    done = [False] * len(v)
    total = 0
    if k:
        for b in range(len(v) // k + 1):
            i0, i1 = b * k, b * k + k
            if i0 < lo or i1 > hi or i0 <= BAD_FIRST_INDEX < i1:
                continue
            if all(s <= 1 for s in v[i0:i1]):
                total += any(v[i0:i1])
                for i in range(i0, i1):
                    done[i] = True
    for i, s in enumerate(v):
        if not done[i]:
            total += 1 if s == 1 else 0 if s == 0 else _digits_of_magnitude_one(s, c)
    return total


class Rig:
    def __init__(self):
        import masp_amd
        self.ctx = masp_amd.Context(0)
        rng = random.Random(20240)
        self.v = _scalars(rng)
        self.sc = np.stack([np.stack([_le(s) for s in v]) for v in self.v])
        self.bases = {"g1": _bases(rng, O.g1_mul_gen_many), "g2": _bases(rng, O.g2_mul_gen_many)}
        msm = {"g1": O.msm_g1, "g2": O.msm_g2}
        # the reference, once: shared by every case below and never changed
        self.want = {g: [msm[g](self.bases[g], self.sc[p]) for p in range(NP)] for g in ("g1", "g2")}

    def run(self, group, np_, window_bits, block_bits, lo):
        fn = self.ctx.msm_g1_multi_ex if group == "g1" else self.ctx.msm_g2_multi_ex
        return fn(self.bases[group], self.sc[:np_], window_bits=window_bits, block_bits=block_bits, sub_lo=lo)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.ctx.close()


@pytest.mark.parametrize("lo", [0, 5])
@pytest.mark.parametrize("block_bits", [0, 2, 3])
@pytest.mark.parametrize("window_bits", [7, 12])
@pytest.mark.parametrize("np_", [1, 9])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_msm_with_subset_rows_matches_the_oracle(rig, group, np_, window_bits, block_bits, lo):
    got, _ = rig.run(group, np_, window_bits, block_bits, lo)
    assert got == rig.want[group][:np_]


@pytest.mark.parametrize("lo", [0, 5])
@pytest.mark.parametrize("block_bits", [0, 2, 3])
@pytest.mark.parametrize("window_bits", [7, 12])
def test_bucket0_entry_count_follows_the_block_rule(rig, window_bits, block_bits, lo):
    """the number of bucket-0 entries the sort produced = the count by the block rule, for every proof of the batch: the all-boolean blocks
    are found, the bad block (P, -P) and the blocks outside the range are left alone, nothing is counted twice"""
    _, cnt = rig.run("g1", NP, window_bits, block_bits, lo)
    want = [_bucket0_entries(v, window_bits, block_bits, lo, N) for v in rig.v]
    print("bucket-0 entries", cnt, "expected", want)
    assert cnt == want
    if block_bits:
        plain = [_bucket0_entries(v, window_bits, 0, 0, N) for v in rig.v]
        assert all(w < p for w, p in zip(want, plain))      # (the test's scalars do exercise the rule)


def test_context_setting_reaches_the_circuit_tables(rig):
    """masp_hip_ctx_set_boolean_block_bits: -1 off, 2 / 3, 0 the build's default, for circuits loaded afterwards: the same proof bytes,
    a lone proof and a batch of nine, whatever the block width"""
    import toy_r1cs
    ctx = rig.ctx
    default = ctx.boolean_block_bits
    assert default in (0, 2, 3)
    cs, inputs, aux, vals = toy_r1cs.make(4321, n_inputs=5, n_free=300, n_constraints=900, bool_share=0.7)
    tw = toy_r1cs.toxic(4321)
    params = ctx.generate_parameters(cs, tw)
    rs = [(5000 + 2 * k, 5001 + 2 * k) for k in range(9)]
    P = O.Params(params)
    want_one = O.create_proof(P, cs, inputs, aux, 77, 88)
    want = [O.create_proof(P, cs, inputs, aux, r, s) for r, s in rs]
    try:
        for bits, resolved in ((-1, 0), (2, 2), (3, 3), (0, default)):
            ctx.set_boolean_block_bits(bits)
            assert ctx.boolean_block_bits == resolved
            ctx.load_circuit(0, params, cs)
            assert ctx.prove(0, inputs, aux, 77, 88) == want_one
            assert ctx.prove_batch([(0, inputs, aux, r, s) for r, s in rs]) == want
        with pytest.raises(Exception):
            ctx.set_boolean_block_bits(5)
    finally:
        ctx.set_boolean_block_bits(0)
