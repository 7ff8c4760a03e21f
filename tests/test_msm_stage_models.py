"""The models the MSM stage tests compare the kernels with (tests/msm_stage_models.py), checked without a GPU against things they share no
code with: the digits against the scalar they spell, the tree's levels against the plain sum of a bucket, the entries — pushed through bucket
sums and the weighted sum — against sum s_i P_i by double-and-add."""
import random

import pytest

import msm_stage_models as M
from msm_stage_models import edge_scalars
from pyref import F1, F2, G1, G2, R, ec_add, ec_mul

WIDTHS = [4, 7, 8, 9, 12, 16]


@pytest.mark.parametrize("c", WIDTHS)
def test_digits_spell_the_scalar_and_never_carry_out_of_the_top_window(c):
    rng = random.Random(c)
    W, nb = M.geom(c)
    for s in edge_scalars(c, rng, 40):
        ds, carry = M.digits_carry(s, c)
        assert carry == 0, hex(s)
        assert all(0 <= j < W and 0 <= b < nb and neg in (0, 1) for j, b, neg in ds)
        assert len({j for j, _, _ in ds}) == len(ds)
        assert sum((-1 if neg else 1) * (b + 1) << (c * j) for j, b, neg in ds) == s, hex(s)
    assert M.digits(0, c) == []


def test_digit_thresholds():
    # a window equal to 2^(c-1) stays positive (bucket 2^(c-1) - 1); one more is negative with a carry
    assert M.digits(8, 4) == [(0, 7, 0)]
    assert M.digits(9, 4) == [(0, 6, 1), (1, 0, 0)]
    assert M.digits(15, 4) == [(0, 0, 1), (1, 0, 0)]
    assert M.digits(0xFF, 4) == [(0, 0, 1), (2, 0, 0)]   # the middle window becomes 16 = 0 with a carry: no entry


def _rand_points(F, gen, rng, n):
    return [ec_mul(F, gen, rng.randrange(1, R)) for _ in range(n)]


@pytest.mark.parametrize("F,gen", [(F1, G1), (F2, G2)], ids=["g1", "g2"])
def test_folding_tree_levels_is_the_plain_sum_of_the_bucket(F, gen):
    rng = random.Random(5)
    base = _rand_points(F, gen, rng, 6)
    for length in list(range(0, 19)) + [31, 32, 33]:
        pts = []
        for k in range(length):
            kind = rng.randrange(6)
            p = base[rng.randrange(len(base))]
            if kind == 0:
                pts.append(M.inf(F))
            elif kind == 1 and pts:
                pts.append(pts[-1])                               # a doubling where the pair falls on it
            elif kind == 2 and pts and not M.is_inf(F, pts[-1]):
                pts.append(M.neg(F, pts[-1]))                     # P - P
            else:
                pts.append(p)
        want = None
        for p in pts:
            want = ec_add(F, want, M.to_ref(F, p))
        cur, level = pts, 0
        while len(cur) > 1:
            nxt = M.tree_level(F, cur)
            assert len(nxt) == (len(cur) + 1) // 2
            cur = nxt
            level += 1
        got = cur[0] if cur else M.inf(F)
        assert M.to_ref(F, got) == want, length
    # the G1 point (0, 2): x = 0 but not infinity
    if F is F1:
        T = (0, 2)
        assert M.affine_add(F, T, T) == ec_add(F, T, T) == (0, F.neg(2))
        assert M.affine_add(F, T, M.neg(F, T)) == M.inf(F)
        assert M.affine_add(F, M.inf(F), T) == T and M.affine_add(F, T, M.inf(F)) == T


def _via_model(F, bases, scalars, c, subset):
    n = len(bases)
    rows = list(M.table(F, tuple(M.from_ref(F, p) for p in bases), c))
    if subset is not None:
        bits, b_first, b_end, bad = subset
        k = 1 << bits
        for blk in range(b_first, b_end):
            for pattern in range(1, 1 << k):
                acc = None
                for t in range(k):
                    if (pattern >> t) & 1:
                        acc = ec_add(F, acc, bases[blk * k + t])
                rows.append(M.from_ref(F, acc))
    per_bucket = M.entries(scalars, n, c, subset)
    sums = [M.bucket_sum(F, [M.entry_point(F, rows, e) for e in run]) for run in per_bucket]
    return M.to_ref(F, M.weighted_sum(F, sums)), per_bucket


@pytest.mark.parametrize("F,gen,c", [(F1, G1, 4), (F1, G1, 7), (F1, G1, 9), (F2, G2, 4)], ids=["g1-c4", "g1-c7", "g1-c9", "g2-c4"])
@pytest.mark.parametrize("with_subset", [False, True])
def test_entries_through_bucket_sums_give_the_msm(F, gen, c, with_subset):
    rng = random.Random(100 + c)
    n = 20
    bases = _rand_points(F, gen, rng, n)
    edge = edge_scalars(c, rng)
    scalars = [rng.choice(edge) for _ in range(n)]
    scalars[0:4] = [1, 0, 1, 1]        # a boolean block
    scalars[4:8] = [0, 0, 0, 0]        # pattern 0
    scalars[8:12] = [1, 1, 5, 0]       # one non-boolean scalar in the block
    scalars[12:16] = [1, 1, 1, 1]      # a bad block when the subset marks it
    subset = (2, 0, 4, {3}) if with_subset else None
    got, per_bucket = _via_model(F, bases, scalars, c, subset)
    want = None
    for s, p in zip(scalars, bases):
        want = ec_add(F, want, ec_mul(F, p, s))
    assert got == want
    W, _ = M.geom(c)
    flat = [e for run in per_bucket for e in run]
    assert len(set(flat)) == len(flat)
    if with_subset:
        assert W * n + 0 * 15 + 0b1101 - 1 in per_bucket[0]               # the block 1, 0, 1, 1 as one subset row
        assert not any(W * n + 15 <= e < W * n + 30 for e in per_bucket[0])  # pattern 0: no entry
        assert {8, 9} <= set(per_bucket[0]) and {12, 13, 14, 15} <= set(per_bucket[0])  # the mixed block and the bad block: row by row
    else:
        assert {0, 2, 3, 8, 9, 12, 13, 14, 15} <= set(per_bucket[0])


def test_layout_and_scan():
    start, words = M.layout([[1, 2, 3], [], [4], [5, 6, 7, 8]], 2, 16)
    assert start == [0, 4, 4, 8, 12]
    assert words == [1, 2, 3, M.PAD_ENTRY, 4, M.PAD_ENTRY, M.PAD_ENTRY, M.PAD_ENTRY, 5, 6, 7, 8] + [M.POISON] * 4
    assert M.scan([3, 0, 2]) == [0, 3, 3, 5]
