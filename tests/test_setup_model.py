"""tests/setup_model.py against the oracle, on the CPU: parameter generation by definition (the Lagrange basis as the inverse transform of
the powers of tau, as bellperson computes it) gives the bytes that oracle/groth16_oracle.cpp gives by the closed formula
l_k = (Z / m) w^k / (tau - w^k) — row order, the extra Input(i) * 0 = 0 rows and the identity filter included.  Everything is integers
and bytes: equality, no tolerance."""
import random

import pytest

import oracle_lib as O
import setup_model as M
import toy_r1cs
from pyref import R


def _toxic(seed, tau):
    return [tau % R] + toy_r1cs.toxic(seed)[1:]


def _taus(logm, seed):
    """off the domain: 0, 2, w_m + 1 and a random one"""
    return [0, 2, M.omega(logm) + 1, random.Random(seed).randrange(2, R)]


def test_lagrange_basis_interpolates():
    """the model's basis, by what a Lagrange basis is: sum_k l_k(tau) f(w^k) = f(tau) for every f of degree < m.  With f = X this pins
    row k to the point w^k, whatever formula computes l_k."""
    rng = random.Random(11)
    for logm in (1, 2, 5):
        m, w = 1 << logm, M.omega(logm)
        assert pow(w, m, R) == 1 and pow(w, m // 2, R) == R - 1
        f = [rng.randrange(R) for _ in range(m)]
        ev = lambda x: sum(c * pow(x, i, R) for i, c in enumerate(f)) % R
        for tau in _taus(logm, logm) + [R - 2]:
            lag = M.lagrange_at(tau % R, logm)
            assert sum(lag) % R == 1
            assert sum(l * pow(w, k, R) for k, l in enumerate(lag)) % R == tau % R
            assert sum(l * ev(pow(w, k, R)) for k, l in enumerate(lag)) % R == ev(tau % R)


def test_closed_formula_agrees_off_the_domain():
    """the formula the kernel, the oracle and pyclosed share, against the definition"""
    for logm in (1, 3, 6):
        m, w = 1 << logm, M.omega(logm)
        for tau in _taus(logm, 5 + logm) + [R - 2]:
            tau %= R
            z_over_m = (pow(tau, m, R) - 1) * pow(m, -1, R) % R
            closed = [z_over_m * pow(w, k, R) * pow(tau - pow(w, k, R), -1, R) % R for k in range(m)]
            assert closed == M.lagrange_at(tau, logm)


def test_on_the_domain_the_basis_is_a_delta_and_z_is_zero():
    """tau = w^j: l_k = [k == j] and Z(tau) = 0 — every h point would be the identity and l, ic collapse to single rows.  The closed
    formula with inv(0) = 0 gives all zeros there instead; masp_hip_generate_parameters refuses such a tau (MASP_HIP_E_UNEXPECTED_IDENTITY)."""
    for logm in (1, 2, 4):
        m, w = 1 << logm, M.omega(logm)
        for j in sorted({0, 1, m // 2, m - 1}):
            tau = pow(w, j, R)
            assert M.lagrange_at(tau, logm) == [1 if k == j else 0 for k in range(m)]
            assert (pow(tau, m, R) - 1) % R == 0
    cs, _ = M.sparse_system(2)
    s = M.parameter_scalars(cs, _toxic(3, M.omega(3)))          # tau = w: row 1
    assert s["h"] == [0] * 7
    assert M.parameter_scalars(cs, _toxic(3, 1))["h"] == [0] * 7 and M.parameter_scalars(cs, _toxic(3, R - 1))["h"] == [0] * 7


def _hand_systems():
    one = M.r1cs_from_rows(1, 1, [([(0, 1)], [(1, 1)], [(1, 1)])])                       # one constraint, ONE alone as input: m = 2
    no_aux = M.r1cs_from_rows(2, 0, [([(0, 3), (1, 1)], [(1, 1)], [(0, 5)]), ([(1, R - 1)], [(0, 1)], [(1, R - 1)])])   # m = 4
    return [("one_constraint", one), ("no_aux", no_aux)]


@pytest.mark.parametrize("name", ["one_constraint", "no_aux", "sparse"])
def test_model_matches_oracle_hand_built(name):
    for tau in _taus(3 if name == "sparse" else 1 if name == "one_constraint" else 2, 17):
        if name == "sparse":
            cs, (n_a, n_b) = M.sparse_system(tau)
        else:
            cs = dict(_hand_systems())[name]
        tw = _toxic(29, tau)
        want = O.generate_parameters(cs, tw).tobytes()
        got = M.generate_parameters(cs, tw)
        assert got == want, (name, tau)
        if name == "sparse":
            sec = M.section_offsets(got)
            assert (sec["a"][2], sec["b_g1"][2], sec["b_g2"][2]) == (n_a, n_b, n_b)
            assert sec["ic"][2] == 3 and sec["l"][2] == 4 and sec["h"][2] == 7


@pytest.mark.parametrize("which", ["0", "2", "w+1", "random"])
@pytest.mark.parametrize("shape", [(2, 4, 9), (4, 10, 61)])
def test_model_matches_oracle_toy(shape, which):
    """both toy shapes (m = 16 and m = 128) at every tau of _taus, a case each"""
    n_in, n_free, nc = shape
    cs = toy_r1cs.make(100 + nc, n_in, n_free, nc)[0]
    logm = M.log2_ceil(cs.n_constraints + cs.n_inputs)
    assert cs.logm == logm
    tau = dict(zip(["0", "2", "w+1", "random"], _taus(logm, nc)))[which]
    tw = _toxic(nc, tau)
    assert M.generate_parameters(cs, tw) == O.generate_parameters(cs, tw).tobytes(), (shape, tau)


def test_alpha_and_beta_zero():
    """degenerate but legal toxic waste: alpha_g1 / beta_g1 / beta_g2 at infinity"""
    cs = toy_r1cs.make(7, 2, 4, 9)[0]
    for alpha, beta in ((0, 5), (5, 0), (0, 0)):
        tw = toy_r1cs.toxic(7)
        tw[1], tw[2] = alpha, beta
        got = M.generate_parameters(cs, tw)
        assert got == O.generate_parameters(cs, tw).tobytes()
        assert (got[0] == 0x40) == (alpha == 0) and (got[96] == 0x40) == (beta == 0) and (got[192] == 0x40) == (beta == 0)
