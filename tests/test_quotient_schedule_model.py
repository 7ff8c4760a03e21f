"""The index arithmetic of the evaluation-form quotient's three kernels (tests/quotient_model.py: tile membership, the twiddle index of
every stage, the bit-reversed scale index), lane by lane over a small prime field, against the same stages written plainly and against
direct interpolation on H followed by evaluation on g H.  No GPU."""
import random

import pytest

import quotient_model as Q

F = Q.SMALL


def _shapes():
    """tiles of 2^4 with 1, 2, 3 and 4 (= LT) top stages, tiles of 2^6 with 1, 2, 3"""
    return [(4, 4 + d) for d in (1, 2, 3, 4)] + [(6, 6 + d) for d in (1, 2, 3)]


def _row_counts(lt, logm):
    """1, the three counts around the first element of the second tile's second tile row (the zero fill starts just before, at, and just
    behind a tile's column boundary), m - 1 and m"""
    m, cols = 1 << logm, 1 << (2 * lt - logm)
    edge = (1 << lt) | cols
    assert edge + 1 < m
    return sorted({1, edge - 1, edge, edge + 1, m - 1, m})


CASES = [(lt, logm, nrows) for lt, logm in _shapes() for nrows in _row_counts(lt, logm)]


def test_the_cases_cover_what_they_should():
    assert sorted({logm - lt for lt, logm, _ in CASES if lt == 4}) == [1, 2, 3, 4]
    for lt, logm, _ in CASES:
        assert lt < logm <= 2 * lt
    assert pow(F.root, 1 << (F.two_adicity - 1), F.p) == F.p - 1                     # the root's order is 2^two_adicity exactly
    assert pow(F.gen, (F.p - 1) // 2, F.p) == F.p - 1                                # the shift lies outside every 2-power subgroup


@pytest.mark.parametrize("lt,logm,nrows", CASES)
def test_three_kernels_equal_direct_interpolation_and_evaluation(lt, logm, nrows):
    rng = random.Random(1000 * logm + nrows + lt)
    m, stride = 1 << logm, nrows + 3
    a = [rng.randrange(F.p) for _ in range(stride)]                                   # the three behind the row are never read
    b = ([0, 1, F.p - 1] + [rng.randrange(F.p) for _ in range(stride)])[:stride]
    xa, xb = Q.kernel_dif_top(F, a, nrows, logm, lt), Q.kernel_dif_top(F, b, nrows, logm, lt)
    assert xa == Q.dif_top(F, a, nrows, logm, lt) and xb == Q.dif_top(F, b, nrows, logm, lt), "first kernel"
    ya, yb = Q.kernel_mid(F, xa, logm, lt), Q.kernel_mid(F, xb, logm, lt)
    assert ya == Q.mid(F, xa, logm, lt) and yb == Q.mid(F, xb, logm, lt), "middle kernel"
    e = Q.kernel_dit_top_ab(F, ya, yb, logm, lt)
    assert e == Q.dit_top_ab(F, ya, yb, logm, lt), "last kernel"
    assert e == Q.direct(F, a, b, nrows, logm), "the chain"


@pytest.mark.parametrize("lt,logm", _shapes())
def test_inverse_half_leaves_scaled_coefficients_in_bit_reversed_order(lt, logm):
    """all of the inverse transform (first kernel, then the middle kernel's first half, here in its plain form): m x coefficient rev(i) at i"""
    rng = random.Random(logm)
    m, p = 1 << logm, F.p
    coef = [rng.randrange(p) for _ in range(m)]
    w = F.omega(logm)
    ev = [sum(c * pow(w, j * k % m, p) for j, c in enumerate(coef)) % p for k in range(m)]
    x = Q.kernel_dif_top(F, ev, m, logm, lt)
    tw_inv = F.tables(logm)[1]
    for s in range(lt - 1, -1, -1):
        Q.stage(x, p, tw_inv, logm, s, True)
    assert x == [m * coef[Q.rev(i, logm)] % p for i in range(m)]
