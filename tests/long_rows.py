"""Seeded R1CS instances with rows of a chosen length each, and satisfying witnesses: circuits whose rows reach the wave path of
k_r1cs_eval (masp_amd/csrc/device/r1cs.hpp: rows of R1CS_LONG_ROW = 64 terms and more), which tests/toy_r1cs.py never builds.  Plain
Python: no GPU and no product code beyond the R1cs container.  Also the big-integer reference of the evaluation and the row order
that masp_hip_circuit_load documents, for tests/test_long_rows_host.py and tests/test_gpu_prove_stages.py."""
import random

import numpy as np

from pyref import R
from oracle_lib import R1cs

LONG_ROW = 64                    # masp_amd/csrc/launch.h: R1CS_LONG_ROW


def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), dtype=np.uint8)


def make(seed, n_inputs, n_seed_aux, a_lens, b_lens, c_lens, witness_seed=None):
    """returns (R1cs, inputs u8[n_inputs,32], aux u8[n_aux,32], values list[int]) like toy_r1cs.make.  Row i of A, B, C has exactly
    a_lens[i], b_lens[i], c_lens[i] terms: the A and B terms over distinct variables among those that exist so far, the C row over
    c_lens[i] - 1 of those plus one fresh aux variable whose value is solved so that the row holds.  The constraint system (columns
    and coefficients) comes from `seed` alone; the free values (inputs, the n_seed_aux first aux) from `witness_seed`, so that two
    witness seeds give two statements of one circuit."""
    assert len(a_lens) == len(b_lens) == len(c_lens) and n_inputs >= 1 and n_seed_aux >= 3
    assert min(c_lens) >= 1 and min(a_lens) >= 0 and min(b_lens) >= 0
    rng = random.Random(seed)                                             # the structure
    vrng = random.Random(seed if witness_seed is None else witness_seed * 104729 + 7)   # the free values
    vals = [1] + [vrng.randrange(R) for _ in range(n_inputs - 1)]         # inputs (ONE first), then aux
    vals += [0, 1, R - 1] + [vrng.randrange(R) for _ in range(n_seed_aux - 3)]
    rows = {"a": [], "b": [], "c": []}

    def coef():
        return rng.choice([1, 1, R - 1, 2, rng.randrange(1, R)])

    def lc(k):
        assert k <= len(vals), "a row of %d terms over %d variables" % (k, len(vals))
        return [(v, coef()) for v in sorted(rng.sample(range(len(vals)), k))]

    def lc_val(terms):
        return sum(c * vals[v] for v, c in terms) % R

    for la_n, lb_n, lc_n in zip(a_lens, b_lens, c_lens):
        la, lb, rest = lc(la_n), lc(lb_n), lc(lc_n - 1)
        k = rng.randrange(1, R)
        fresh = len(vals)
        # rest + k * fresh = a * b
        vals.append((lc_val(la) * lc_val(lb) - lc_val(rest)) * pow(k, -1, R) % R)
        rows["a"].append(la)
        rows["b"].append(lb)
        rows["c"].append(rest + [(fresh, k)])
    n_aux = len(vals) - n_inputs
    mats = []
    seen = set()
    for name in "abc":
        rp, col, cf = [0], [], []
        for terms in rows[name]:
            for v, c in terms:
                col.append(v)
                cf.append(_le(c))
            rp.append(len(col))
        seen.update(col)
        mats.append((np.array(rp, np.uint32), np.array(col, np.uint32), np.stack(cf) if cf else np.zeros((0, 32), np.uint8)))
    # an aux variable absent from all three matrices has the point at infinity in the l query, which no loader accepts
    missing = [v for v in range(n_inputs, n_inputs + n_aux) if v not in seen]
    assert not missing, "seed %r leaves aux variables %r unconstrained: pick another" % (seed, missing[:8])
    cs = R1cs(n_inputs, n_aux, len(a_lens), mats)
    return cs, np.stack([_le(v) for v in vals[:n_inputs]]), np.stack([_le(v) for v in vals[n_inputs:]]), vals


# ---- the named shapes (all with n_constraints + n_inputs <= 128: logm <= 7) -----------------------------------------------------
E = (1, 2, 63, 64, 65, 127, 128, 129, 577)          # the lengths around the threshold and around multiples of 64; A and B also get 0


def _spread(n, special, seed):
    """n row lengths: `special` at seeded positions, 1 to 3 terms everywhere else"""
    rng = random.Random(seed)
    lens = [rng.randint(1, 3) for _ in range(n)]
    for at, k in zip(rng.sample(range(n), len(special)), special):
        lens[at] = k
    return lens


def _mixed(n, tag):
    return dict(a_lens=_spread(n, (0,) + E + (191, 192, 193), tag + 1),          # 9 long rows
                b_lens=_spread(n, (0,) + E + (192,), tag + 2),                   # 7
                c_lens=_spread(n, E, tag + 3))                                   # 6


def shape(name):
    """the keyword arguments of make() for a named shape, without the seed"""
    if name == "MIXED":          # every length of E in every matrix; n_long differs per matrix and A has the most
        # 78 rows + 9 x 63 lanes = 5 blocks of 128 and 5 lanes: a grid that is short by one lane per long row loses the sixth block
        return dict(n_inputs=4, n_seed_aux=600, **_mixed(74, 10))
    if name == "C_HEAVY":        # A without a long row, B with two, C with nine: a launch of A and B alone sizes its grid without C
        # 73 rows + 9 x 63 lanes = 5 blocks exactly when C is evaluated: no spare lane computes a row that the lanes proper missed
        return dict(n_inputs=4, n_seed_aux=600, a_lens=_spread(69, (0, 63, 63), 21), b_lens=_spread(69, (0, 63, 64, 577), 22),
                    c_lens=_spread(69, (63, 64, 65, 127, 128, 129, 191, 192, 193, 577), 23))
    if name == "ALL_LONG":       # every row of every matrix is long: n_long == n_constraints
        # 64 inputs: 69 rows + 5 x 63 lanes = 3 blocks exactly, whether C is evaluated or not
        return dict(n_inputs=64, n_seed_aux=200, a_lens=[64, 65, 127, 128, 200], b_lens=[200, 64, 129, 100, 192],
                    c_lens=[65, 193, 64, 128, 199])
    if name == "FULL":           # MIXED-like with n_constraints + n_inputs == 2^7 exactly
        return dict(n_inputs=4, n_seed_aux=600, **_mixed(124, 40))
    raise KeyError(name)


SHAPES = ("MIXED", "C_HEAVY", "ALL_LONG", "FULL")
# n_long of A, B, C
N_LONG = {"MIXED": (9, 7, 6), "C_HEAVY": (0, 2, 9), "ALL_LONG": (5, 5, 5), "FULL": (9, 7, 6)}
# structure seeds with which every aux variable is constrained (make() asserts it)
SEED = {"MIXED": 1, "C_HEAVY": 1, "ALL_LONG": 1, "FULL": 1}


def named(name, witness_seed=None):
    return make(SEED[name], witness_seed=witness_seed, **shape(name))


# ---- the reference -------------------------------------------------------------------------------------------------------------
def row_lengths(cs, which):
    rp = cs.mats[which][0]
    return [int(rp[i + 1]) - int(rp[i]) for i in range(cs.n_constraints)]


def row_order(cs, which):
    """(order, n_long) as masp_hip_circuit_load derives them: the constraint rows in a stable sort by decreasing length, and how many
    of them have LONG_ROW terms or more"""
    lens = row_lengths(cs, which)
    order = sorted(range(cs.n_constraints), key=lambda r: -lens[r])      # sorted() is stable
    return order, sum(1 for k in lens if k >= LONG_ROW)


def reference_eval(cs, values):
    """a, b, c as lists of n_constraints + n_inputs ints: row = sum(coef * w[col]) mod r, then bellperson's input rows a = w[i], b = c = 0"""
    out = []
    for which, (rp, col, coef) in enumerate(cs.mats):
        cf = [int.from_bytes(coef[t].tobytes(), "little") for t in range(coef.shape[0])]
        rows = [sum(cf[t] * values[int(col[t])] for t in range(int(rp[i]), int(rp[i + 1]))) % R for i in range(cs.n_constraints)]
        out.append(rows + [values[i] % R if which == 0 else 0 for i in range(cs.n_inputs)])
    return out
