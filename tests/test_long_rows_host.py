"""tests/long_rows.py itself, without a GPU: its circuits are satisfied, its named shapes have the rows they claim, and its big-integer
evaluation — the reference of tests/test_gpu_prove_stages.py — is the oracle's."""
import numpy as np
import pytest

import long_rows
import oracle_lib as O
from pyref import R


@pytest.fixture(scope="module", params=long_rows.SHAPES)
def made(request):
    return request.param, long_rows.named(request.param), long_rows.named(request.param, witness_seed=2)


def test_the_circuits_are_satisfied(made):
    _, (cs, inputs, aux, values), (cs2, inputs2, aux2, values2) = made
    assert O.r1cs_unsatisfied(cs, inputs, aux) == 0
    assert O.r1cs_unsatisfied(cs, inputs2, aux2) == 0          # the second witness, under the FIRST call's constraint system
    assert values != values2 and values[0] == values2[0] == 1
    for (rp, col, coef), (rp2, col2, coef2) in zip(cs.mats, cs2.mats):
        assert (rp == rp2).all() and (col == col2).all() and (coef == coef2).all()
    n_in = cs.n_inputs
    assert values[n_in:n_in + 3] == [0, 1, R - 1]
    assert [int.from_bytes(aux[k].tobytes(), "little") for k in range(cs.n_aux)] == values[n_in:]


def test_the_reference_evaluation_is_the_oracles(made):
    _, (cs, inputs, aux, values), _ = made
    ref = long_rows.reference_eval(cs, values)
    got = O.r1cs_eval(cs, inputs, aux)[:3]
    for name, mine, theirs in zip("abc", ref, got):
        assert mine == [int.from_bytes(theirs[k].tobytes(), "little") for k in range(cs.nrows)], name
    assert [x * y % R for x, y in zip(ref[0], ref[1])] == ref[2]


def test_the_named_shapes(made):
    name, (cs, _, _, _), _ = made
    lens = [long_rows.row_lengths(cs, which) for which in range(3)]
    spec = long_rows.shape(name)
    assert lens == [spec["a_lens"], spec["b_lens"], spec["c_lens"]]
    n_long = tuple(long_rows.row_order(cs, which)[1] for which in range(3))
    assert n_long == long_rows.N_LONG[name]
    assert cs.nrows <= 128 and cs.logm <= 7
    for which in range(3):
        order, nl = long_rows.row_order(cs, which)
        assert sorted(order) == list(range(cs.n_constraints))
        by_len = [lens[which][r] for r in order]
        assert by_len == sorted(by_len, reverse=True) and all(k >= 64 for k in by_len[:nl]) and all(k < 64 for k in by_len[nl:])
        # stable: rows of one length keep their order
        assert all(order[i] < order[i + 1] for i in range(len(order) - 1) if by_len[i] == by_len[i + 1])
    if name in ("MIXED", "FULL"):
        for which in range(3):
            assert set(long_rows.E) <= set(lens[which])
            assert set(lens[which]) - set(long_rows.E) - {191, 192, 193} <= {0, 1, 2, 3}
        assert 0 in lens[0] and 0 in lens[1]
        assert n_long[0] > n_long[1] > n_long[2] > 0
    # launch_r1cs_eval: 64 lanes per long row of the matrix with the most, one per remaining row, in blocks of 128
    lanes = lambda n_mat: cs.nrows + 63 * max(n_long[:n_mat])
    if name == "MIXED":          # the lanes end within one lane per long row of a block's start: a grid short by that much loses the block
        assert all(1 <= lanes(n_mat) % 128 <= max(n_long[:n_mat]) for n_mat in (2, 3))
    if name == "C_HEAVY":        # no spare lanes behind the last row when C is evaluated
        assert n_long == (0, 2, 9) and max(lens[0]) == 63 and lanes(3) % 128 == 0
    if name == "ALL_LONG":       # ... and none here with or without C
        assert cs.n_constraints == 5 and all(64 <= k <= 200 for m in lens for k in m) and n_long == (5, 5, 5)
        assert lanes(2) % 128 == lanes(3) % 128 == 0
    if name == "FULL":
        assert cs.nrows == 1 << cs.logm == 128
