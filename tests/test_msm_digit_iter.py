"""The sort's digit iterator (masp_amd/csrc/device/msm_sort.hpp: MsmDigitIter) on the host, through tests/native/msm_digits_dev.hip: the
iterator holds the scalar's eight words and shifts them window by window, so what it hands out — (table, bucket, neg) per window — is compared
here, window for window, with the models that take the digits from the integer itself: tests/msm_stage_models.py (plain geometry, every width
from 4 to 16 bits: W = 64 .. 16) and tests/msm_twin_models.py (doubled rows).  No GPU."""
import random

import pytest

import msm_stage_models as M
import msm_twin_models as TM
from pyref import R


@pytest.fixture(scope="module")
def shim():
    import msm_digits_shim
    msm_digits_shim.load()
    return msm_digits_shim


def scalars_for(c):
    rng = random.Random(4000 + c)
    return M.edge_scalars(c, rng, 8) + [0, 1, 2, R - 1, R - 2, (1 << 255) - 1] + [rng.randrange(R) for _ in range(200)]


def plain_windows(s, c):
    """the model's digit list as one (table, bucket, neg) or None per window"""
    W, _ = M.geom(c)
    out = [None] * W
    for j, b, neg in M.digits(s, c):
        out[j] = (j, b, neg)
    return out


def twin_windows(s, c):
    W, _ = M.geom(c)
    out = [None] * W
    for j, b, neg in M.digits(s, c):
        mult, value = TM.recode(b + 1)
        out[j] = (j + (W if mult == 2 else 0), TM.bucket_id(c, value), neg)
    return out


def compare(got, want, where):
    assert len(got) == len(want), where
    for j, (g, w) in enumerate(zip(got, want)):
        table, bucket, neg, nz = g
        if w is None:
            assert nz == 0, (where, j)
        else:
            assert (table, bucket, neg, nz) == w + (1,), (where, j)


@pytest.mark.parametrize("c", range(4, 17))
def test_plain_digits_are_the_models(shim, c):
    scalars = scalars_for(c)
    got = shim.digits(scalars, c)
    for s, per in zip(scalars, got):
        compare(per, plain_windows(s, c), "c=%d s=%#x" % (c, s))


@pytest.mark.parametrize("c", [4, 5, 12, 13, 15, 16])
def test_doubled_row_digits_are_the_models(shim, c):
    scalars = scalars_for(c)
    got = shim.digits(scalars, c, twin=True)
    for s, per in zip(scalars, got):
        compare(per, twin_windows(s, c), "twin c=%d s=%#x" % (c, s))


def test_the_window_that_starts_below_bit_256_sees_zeros_above_it(shim):
    """c = 5, 13, 15: the last window reaches beyond the scalar; all 256 bits set, its digit is the scalar's top bits plus the carry alone"""
    for c in (5, 13, 15):
        W, _ = M.geom(c)
        s = (1 << 256) - 1
        top = (s >> (c * (W - 1))) + 1                       # the bits below 256 that the window holds, and the carry into it
        assert top <= 1 << (c - 1)
        per = shim.digits([s], c)[0]
        assert per[W - 1] == (W - 1, top - 1, 0, 1)
        assert per[0] == (0, 0, 1, 1) and all(q[3] == 0 for q in per[1:W - 1])   # -1, then all-ones windows + carry = 2^c -> digit 0, carry


def test_scalar_classes(shim):
    assert [shim.scalar_class(s) for s in (0, 1, 2, 1 << 32, 1 << 255, (1 << 32) + 1, R - 1)] == [0, 1, 2, 2, 2, 2, 2]
