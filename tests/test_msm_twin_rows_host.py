"""Doubled window rows (masp_amd/csrc/device/msm_geom.h: msm_geom_twin): the recoding of a digit magnitude into (row multiple, bucket), as
a Python model written from its definition (tests/msm_twin_models.py) and as the header computes it (through tests/native/msm_twin_host.hip,
host code only), for every window width the sort takes, c = 3 .. 16 — both parities of c - 1.  No GPU.

The number of buckets: B = {4^s o <= H}, H = 2^(c-1), has H / 2 + H / 8 + ... members, which is 2 H / 3 rounded to the NEAREST integer,
(2 H + 1) // 3 — the ceiling of 2 H / 3 where c - 1 is even (11 of 16), its floor where c - 1 is odd (21 845 of 32 768, 5 of 8)."""
import pytest

import msm_stage_models as M
import msm_twin_models as TM

WIDTHS = list(range(3, 17))


@pytest.fixture(scope="module")
def shim():
    import msm_twin_shim
    msm_twin_shim.load_host()
    return msm_twin_shim


def valuation(v):
    return (v & -v).bit_length() - 1


@pytest.mark.parametrize("c", WIDTHS)
def test_every_magnitude_is_a_row_multiple_times_a_bucket_value_of_even_valuation(c):
    H = 1 << (c - 1)
    seen = set()
    for v in range(1, H + 1):
        mult, value = TM.recode(v)
        assert mult in (1, 2) and mult * value == v
        assert valuation(value) % 2 == 0
        seen.add(value)
    assert seen == set(TM.values(c))          # every bucket is some magnitude's, and no magnitude lacks one


@pytest.mark.parametrize("c", WIDTHS)
def test_bucket_ids_are_a_bijection_and_count_two_thirds(c):
    H = 1 << (c - 1)
    vals = TM.values(c)
    assert len(set(vals)) == len(vals) == (2 * H + 1) // 3
    assert sorted(TM.bucket_id(c, v) for v in vals) == list(range(len(vals)))
    assert TM.bucket_id(c, 1) == 0            # unit scalars and subset rows keep landing in bucket id 0
    if (c - 1) % 2 == 0:
        assert len(vals) == -(-2 * H // 3)    # the ceiling ...
    else:
        assert len(vals) == 2 * H // 3        # ... or the floor
    assert len(TM.values(16)) == 21845


@pytest.mark.parametrize("c", WIDTHS)
def test_classes_are_dense_odd_weights_of_power_of_two_sizes(c):
    H = 1 << (c - 1)
    vals = TM.values(c)
    cls = TM.classes(c)
    assert sum(size for _, size, _ in cls) == len(vals)
    for s, (off, size, weight) in enumerate(cls):
        assert weight == 4 ** s and size & (size - 1) == 0
        assert size == max(1, (H >> (2 * s)) // 2)
        assert off % size == 0                # a class of whole weighted-sum chunks starts on a chunk boundary
        assert vals[off:off + size] == [weight * (2 * k + 1) for k in range(size)]


@pytest.mark.parametrize("c", WIDTHS)
def test_the_header_agrees_with_the_model(shim, c):
    H = 1 << (c - 1)
    g, plain = shim.geom(c), shim.geom(c, twin=False)
    W, nb = TM.geom(c)
    assert (g["c"], g["W"], g["twin"], g["tables"]) == (c, W, 1, 2 * W)
    assert g["buckets"] == len(TM.values(c)) and g["nb"] == nb and nb >= g["buckets"] and (nb < 128 or nb % 128 == 0)
    assert (plain["c"], plain["W"], plain["nb"], plain["twin"], plain["tables"]) == (c, M.geom(c)[0], H, 0, W)   # msm_geom(c) is as it was
    cls = TM.classes(c)
    assert g["classes"] == len(cls)
    assert [shim.klass(c, s) for s in range(len(cls))] == cls
    for v in range(1, H + 1):
        mult, value = TM.recode(v)
        assert shim.bucket(c, v) == (mult, TM.bucket_id(c, value)), v


def test_model_entries_name_rows_whose_multiple_times_value_is_the_digit():
    """the model's digit list against the scalar itself: sum over its entries of sign * row multiple * 2^(c j) * bucket value = s"""
    import random
    rng = random.Random(5)
    for c in (4, 5, 8, 13, 16):
        W, nb = TM.geom(c)
        vals = TM.values(c)
        scalars = M.edge_scalars(c, rng)
        n = len(scalars)
        runs = TM.entries(scalars, n, c)
        total = [0] * n
        for b, run in enumerate(runs):
            for e in run:
                row, sign = e & 0x7FFFFFFF, -1 if e >> 31 else 1
                t, i = divmod(row, n)
                assert t < 2 * W
                total[i] += sign * (2 if t >= W else 1) * (1 << (c * (t % W))) * vals[b]
        carries = [M.digits_carry(s, c)[1] for s in scalars]
        assert [t + (k << (c * W)) for t, k in zip(total, carries)] == scalars
