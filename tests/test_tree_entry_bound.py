"""The entry bound by which the scratch of the bucket tree is sized (include/masp_hip.h: masp_hip_r1cs_boolean_variables,
masp_hip_tree_entry_bound) against digit lists counted with Python integers.  No GPU: both entry points are host code."""
import random

import numpy as np

import toy_r1cs
from masp_amd import hip, host as H, workload
from pyref import R


def digits(v, c):
    """the non-zero signed digits of v on c-bit windows, as MsmDigitIter (masp_amd/csrc/device/msm_sort.hpp) takes them:
    [(window, magnitude, negative)]"""
    out, carry, half = [], 0, 1 << (c - 1)
    for j in range((256 + c - 1) // c):
        d = ((v >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 0
        if d > half:
            d, carry = (1 << c) - d, 1
            out.append((j, d, True))
        elif d:
            out.append((j, d, False))
    assert carry == 0                                   # (r < 2^255: the top window never overflows)
    return out


def entries(values, c):
    return sum(len(digits(v, c)) for v in values)


def densities(cs):
    """(a_var, b_var) as masp_hip_circuit_load derives them"""
    nv = cs.n_inputs + cs.n_aux
    in_a, in_b = np.zeros(nv, bool), np.zeros(nv, bool)
    in_a[cs.mats[0][1]] = True
    in_b[cs.mats[1][1]] = True
    in_a[:cs.n_inputs] = True
    return np.flatnonzero(in_a), np.flatnonzero(in_b)


def ints(a):
    return [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]


def test_digits_are_the_scalar():
    rng = random.Random(5)
    for c in (2, 7, 10, 12, 15, 16):
        for v in [0, 1, 2, (1 << (c - 1)), (1 << (c - 1)) + 1, R - 1] + [rng.randrange(R) for _ in range(20)]:
            assert sum((-d if neg else d) << (c * j) for j, d, neg in digits(v, c)) == v
        assert digits(0, c) == [] and digits(1, c) == [(0, 1, False)]


def test_the_bound_is_the_documented_sum():
    for c in (2, 7, 12, 16):
        W = (256 + c - 1) // c
        assert hip.tree_entry_bound(1000, c, 0, 0, 30) == 1000 * W                       # no witness scalar: every one full width
        assert hip.tree_entry_bound(1000, c, 600, 0, 100) == 1000 * W                    # nothing proven, nothing assumed
        assert hip.tree_entry_bound(1000, c, 600, 600, 1) == 400 * W + 600
        assert hip.tree_entry_bound(1000, c, 600, 100, 30) == (400 + 150) * W + 450
        assert hip.tree_entry_bound(1000, c, 600, 99, 1) == (400 + 6) * W + 594          # ceil(501 / 100) = 6
        assert hip.tree_entry_bound(1000, c, 2000, 5000, 100) == 1000                    # counts are cut to what the set holds
    assert hip.tree_entry_bound(1000, 1, 0, 0, 30) == 0 and hip.tree_entry_bound(1000, 17, 0, 0, 30) == 0
    # 0: the build's default share
    assert hip.tree_entry_bound(1000, 12, 600, 100, 1) <= hip.tree_entry_bound(1000, 12, 600, 100, 0) <= hip.tree_entry_bound(1000, 12, 600, 100, 100)


def test_toy_circuit_booleans():
    cs, inputs, aux, vals = toy_r1cs.make(77, n_inputs=5, n_free=60, n_constraints=200, bool_share=0.7)
    proven = hip.r1cs_boolean_variables(cs)
    assert proven.shape == (cs.n_inputs + cs.n_aux,) and proven[0] == 1 and not proven[1:cs.n_inputs].any()
    # every (1 - b) b = 0 of the generator is found ...
    rp = [m[0] for m in cs.mats]
    alloc = [int(cs.mats[1][1][rp[1][i]]) for i in range(cs.n_constraints) if rp[2][i + 1] == rp[2][i]]
    assert len(alloc) > 20 and all(proven[v] for v in alloc)
    # ... and whatever else is proven (a product of two of them) holds 0 or 1
    assert all(vals[v] in (0, 1) for v in np.flatnonzero(proven))
    assert int(proven.sum()) < 1 + len(alloc) + 40


def test_a_coefficient_that_does_not_cancel_proves_nothing():
    cs, *_ = toy_r1cs.make(78, n_inputs=3, n_free=30, n_constraints=60, bool_share=0.9)
    before = hip.r1cs_boolean_variables(cs)
    rp, col, coef = cs.mats[0]
    i = next(i for i in range(cs.n_constraints) if cs.mats[2][0][i + 1] == cs.mats[2][0][i])
    v = int(col[rp[i] + 1])
    assert before[v] == 1
    coef[rp[i] + 1] = np.frombuffer((R - 2).to_bytes(32, "little"), np.uint8)            # (1 - 2 v) v = 0: v = 0 or 1 / 2
    after = hip.r1cs_boolean_variables(cs)
    assert after[v] == 0 and int(after.sum()) <= int(before.sum()) - 1


def test_masp_witnesses_stay_within_the_bound():
    """Output (the smallest of the three circuits), three instances: every variable proven boolean holds 0 or 1, and the digit lists of
    the l, a and b scalars — counted with Python integers on the window widths the batch MSMs use — have no more entries than the
    bound with every unproven scalar at full width, which is the default."""
    cs = H.circuit("output")[0]
    proven = hip.r1cs_boolean_variables(cs).astype(bool)
    assert proven.sum() > cs.n_aux // 2                                                  # the gadgets' results too, not only allocated bits
    a_var, b_var = densities(cs)
    aux_var = np.arange(cs.n_inputs, cs.n_inputs + cs.n_aux)
    for inputs, aux in workload.instances("output", 3, first_seed=11, threads=2):
        vals = ints(inputs) + ints(aux)
        assert all(vals[v] in (0, 1) for v in np.flatnonzero(proven))
        for var, c in ((aux_var, 15), (aux_var, 16), (a_var, 12), (b_var, 12), (b_var, 10)):
            bound = hip.tree_entry_bound(len(var), c, len(var), int(proven[var].sum()), 100)
            have = entries([vals[v] for v in var], c)
            assert have <= bound < len(var) * ((256 + c - 1) // c), (c, have, bound)
            # a share that is too small is a bound that a real witness exceeds: what the device has to survive
            assert have > hip.tree_entry_bound(len(var), c, len(var), int(proven[var].sum()), 1)
