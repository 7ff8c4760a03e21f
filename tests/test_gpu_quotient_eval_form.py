"""The quotient in evaluation form (masp_hip_ctx_set_quotient_form): the bases the loader derives — the h query through a
group-valued inverse DFT, C's share folded into the l query — against the oracle, point by point and two ways; the proofs of batches in
both forms against each other and against the toxic-waste closed form; and the fallback of a circuit one of whose derived bases is the
point at infinity.  Toy circuits (tests/toy_r1cs.py) on a CRS of known toxic waste.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import oracle_lib as O
import toy_r1cs
from pyclosed import ROOT_OF_UNITY_2_32
from pyref import R

pytestmark = pytest.mark.gpu

GEN = 7                          # the coset is g H with g = 7 (masp_amd/csrc/device/consts.hpp: FrCfg::GEN)
EVALUATION, COEFFICIENT = 0, 1
AUX_MONTGOMERY = 1


def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), dtype=np.uint8)


def _c_columns(cs):
    """column -> [(row, coefficient)] of the matrix C"""
    rp, col, coef = cs.mats[2]
    cols = {}
    for row in range(cs.n_constraints):
        for t in range(int(rp[row]), int(rp[row + 1])):
            cols.setdefault(int(col[t]), []).append((row, int.from_bytes(coef[t].tobytes(), "little")))
    return cols


def _interesting(cs):
    """the cases the derived bases must cover: a coefficient of C that is not +-1, an input column C uses and one it does not, an aux
    column absent from C"""
    cols = _c_columns(cs)
    coefs = {c for terms in cols.values() for _, c in terms}
    used_in = [v for v in range(cs.n_inputs) if v in cols]
    return bool(coefs - {1, R - 1}) and 0 < len(used_in) < cs.n_inputs and any(v not in cols for v in range(cs.n_inputs, cs.n_inputs + cs.n_aux))


def _every_aux_constrained(cs):
    """no aux variable is absent from all three matrices: its l query point would be the point at infinity, which no loader accepts"""
    seen = set()
    for _, col, _ in cs.mats:
        seen.update(int(v) for v in col)
    return all(v in seen for v in range(cs.n_inputs, cs.n_inputs + cs.n_aux))


def _circuit(first_seed, **shape):
    for seed in range(first_seed, first_seed + 400):
        made = toy_r1cs.make(seed, **shape)
        if _interesting(made[0]) and _every_aux_constrained(made[0]):
            return seed, made
    raise AssertionError("no seed gives a circuit with every case")


# logm 4 with n_constraints + n_inputs == m, logm 6 well below m; 8 and 10: the sizes the other GPU suites load
SHAPES = {4: dict(n_inputs=5, n_free=4, n_constraints=11, bool_share=0.5),
          6: dict(n_inputs=4, n_free=12, n_constraints=30, bool_share=0.5),
          8: dict(n_inputs=5, n_free=40, n_constraints=200, bool_share=0.6),
          10: dict(n_inputs=5, n_free=60, n_constraints=700, bool_share=0.7)}
N_JOBS = 17
LONG = "long"                    # a circuit with C columns of 64 entries and more: the wave path of the sparse combine
LONG_SHAPE = dict(n_inputs=4, n_free=20, n_constraints=90, bool_share=0.5)
LONG_COL = 64                    # masp_amd/csrc/host/eval_form.h: EvalLayout::LONG_COL


def _with_long_columns(cs):
    """the same constraint system with the constant-one input in 70 rows of C (well past the threshold, coefficients that are not all
    +-1) and the first aux column in exactly LONG_COL rows (at the threshold) — no witness satisfies it; none is needed for the bases"""
    from oracle_lib import R1cs
    rp, col, coef = cs.mats[2]
    cols = _c_columns(cs)
    one, aux0 = 0, cs.n_inputs
    want = {one: 70 - len(cols.get(one, [])), aux0: LONG_COL - len(cols.get(aux0, []))}
    new_rp, new_col, new_coef = [0], [], []
    for row in range(cs.n_constraints):
        for v in (one, aux0):
            if want[v] > 0:
                want[v] -= 1
                new_col.append(v)
                new_coef.append(_le((1, R - 1, 3 + row)[row % 3]))
        for t in range(int(rp[row]), int(rp[row + 1])):
            new_col.append(int(col[t]))
            new_coef.append(coef[t])
        new_rp.append(len(new_col))
    assert want == {one: 0, aux0: 0}
    mats = [cs.mats[0], cs.mats[1], (np.array(new_rp, np.uint32), np.array(new_col, np.uint32), np.stack(new_coef))]
    return R1cs(cs.n_inputs, cs.n_aux, cs.n_constraints, mats)


class Rig:
    """the same circuits on two contexts: one in evaluation form (the default), one in coefficient form"""

    def __init__(self):
        import masp_amd
        from masp_amd.synthetic import toxic_waste
        self.ctx = {EVALUATION: masp_amd.Context(0), COEFFICIENT: masp_amd.Context(0)}
        assert self.ctx[EVALUATION].quotient_form == EVALUATION       # the default
        self.ctx[COEFFICIENT].set_quotient_form(COEFFICIENT)
        assert self.ctx[COEFFICIENT].quotient_form == COEFFICIENT
        self.cs, self.toxic, self.params, self.slot, self.seed = {}, {}, {}, {}, {}
        for slot, (logm, shape) in enumerate(sorted(SHAPES.items())):
            self.seed[logm], (cs, _, _, _) = _circuit(100 * logm, **shape)
            assert cs.logm == logm
            self.cs[logm], self.slot[logm] = cs, slot
            self.toxic[logm] = toxic_waste(700 + logm)
            self.params[logm] = self.ctx[EVALUATION].generate_parameters(cs, self.toxic[logm])
            for c in self.ctx.values():
                c.load_circuit(slot, self.params[logm], cs)
        # ... and the circuit with long columns, in evaluation form only (slot 4 is the infinity test's)
        _, (base, _, _, _) = _circuit(7000, **LONG_SHAPE)
        self.cs[LONG], self.slot[LONG], self.toxic[LONG] = _with_long_columns(base), len(SHAPES) + 1, toxic_waste(777)
        self.params[LONG] = self.ctx[EVALUATION].generate_parameters(self.cs[LONG], self.toxic[LONG])
        self.ctx[EVALUATION].load_circuit(self.slot[LONG], self.params[LONG], self.cs[LONG])
        self._jobs = {}

    def jobs(self, logm):
        """N_JOBS distinct statements of the circuit with their closed-form proofs, computed once"""
        if logm not in self._jobs:
            rng = random.Random(9000 + logm)
            out = []
            for _ in range(N_JOBS):
                ins = [rng.randrange(R) for _ in range(SHAPES[logm]["n_inputs"] - 1)]
                cs, inputs, aux, _ = toy_r1cs.make(self.seed[logm], input_values=ins, **SHAPES[logm])
                r, s = rng.randrange(R), rng.randrange(R)
                out.append((inputs, aux, r, s, O.closed_form_proof(self.cs[logm], self.toxic[logm], inputs, aux, r, s)))
            self._jobs[logm] = out
        return self._jobs[logm]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def test_the_form_in_use_is_reported(rig):
    for logm in SHAPES:
        assert rig.ctx[EVALUATION].circuit_quotient_form(rig.slot[logm]) == EVALUATION
        assert rig.ctx[COEFFICIENT].circuit_quotient_form(rig.slot[logm]) == COEFFICIENT
        pts, cols = rig.ctx[COEFFICIENT].circuit_eval_bases(rig.slot[logm])
        assert pts.shape[0] == 0 and cols == []


def _sections(params, cs):
    """the h and l queries of a Parameters buffer: u8[n, 96] each, and the byte offset of l"""
    p = np.asarray(params, dtype=np.uint8)
    at = 864
    n_ic = int.from_bytes(p[at:at + 4].tobytes(), "big")
    at += 4 + 96 * n_ic
    n_h = int.from_bytes(p[at:at + 4].tobytes(), "big")
    h = p[at + 4:at + 4 + 96 * n_h].reshape(n_h, 96)
    at += 4 + 96 * n_h
    n_l = int.from_bytes(p[at:at + 4].tobytes(), "big")
    assert n_ic == cs.n_inputs and n_l == cs.n_aux and n_h >= (1 << cs.logm) - 1
    return h, p[at + 4:at + 4 + 96 * n_l].reshape(n_l, 96), at + 4


def _dft_rows(cs):
    """per derived base, its coefficients over H_0 .. H_{m-2}: T'_i -> g^-k w^-ik / m;  column j of C -> -sum_i C_ij w^-ik / (m (g^m - 1))"""
    logm = cs.logm
    m = 1 << logm
    w_inv = pow(pow(ROOT_OF_UNITY_2_32, 1 << (32 - logm), R), -1, R)
    g_inv, m_inv = pow(GEN, -1, R), pow(m, -1, R)
    wp = [pow(w_inv, e, R) for e in range(m)]
    t_rows = [[pow(g_inv, k, R) * wp[i * k % m] % R * m_inv % R for k in range(m - 1)] for i in range(m)]
    scale = -m_inv * pow(pow(GEN, m, R) - 1, -1, R) % R
    q_rows = {j: [scale * sum(c * wp[i * k % m] for i, c in terms) % R for k in range(m - 1)] for j, terms in _c_columns(cs).items()}
    return t_rows, q_rows


def _l_scalars(cs, toxic):
    """(beta A_j + alpha B_j + C_j)(tau) / delta for the aux columns, through the Lagrange basis at tau"""
    tau, alpha, beta, _, delta = [t % R for t in toxic]
    m = 1 << cs.logm
    omega = pow(ROOT_OF_UNITY_2_32, 1 << (32 - cs.logm), R)
    z_over_m = (pow(tau, m, R) - 1) * pow(m, -1, R) % R
    lag = [z_over_m * pow(omega, k, R) % R * pow(tau - pow(omega, k, R), -1, R) % R for k in range(cs.n_constraints)]
    out = [0] * (cs.n_inputs + cs.n_aux)
    for (rp, col, coef), weight in zip(cs.mats, (beta, alpha, 1)):
        for row in range(cs.n_constraints):
            for t in range(int(rp[row]), int(rp[row + 1])):
                out[int(col[t])] = (out[int(col[t])] + weight * int.from_bytes(coef[t].tobytes(), "little") % R * lag[row]) % R
    d_inv = pow(delta, -1, R)
    return [v * d_inv % R for v in out[cs.n_inputs:]]


@pytest.mark.parametrize("which", [4, 6, LONG])
def test_derived_bases_against_the_oracle(rig, which):
    """every derived point two ways: as the oracle's MSM over the h query with the DFT row as scalars (nothing of the toxic waste), and
    as a fixed-base multiple of the generator from the toxic-waste closed form.  `long`: an input column (the constant one) and an aux
    column that a wave sums (k_eval_combine_long), the aux one exactly at the threshold."""
    cs, toxic = rig.cs[which], rig.toxic[which]
    logm = cs.logm
    m, n_in, n_aux = 1 << logm, cs.n_inputs, cs.n_aux
    assert cs.nrows == m if which == 4 else cs.nrows < m * 3 // 4
    assert rig.ctx[EVALUATION].circuit_quotient_form(rig.slot[which]) == EVALUATION
    pts, used = rig.ctx[EVALUATION].circuit_eval_bases(rig.slot[which])
    cols = _c_columns(cs)
    if which == LONG:
        assert len(cols[0]) == 70 and len(cols[n_in]) == LONG_COL and max(len(cols[v]) for v in cols if v not in (0, n_in)) < LONG_COL
        assert {c for _, c in cols[0]} - {1, R - 1}
    assert used == [v for v in range(n_in) if v in cols] and 0 < len(used) < n_in
    assert pts.shape == (m + n_aux + len(used), 96)
    h, l, _ = _sections(rig.params[which], cs)
    h = h[:m - 1]
    t_rows, q_rows = _dft_rows(cs)
    # 1. MSMs over the CRS points themselves
    for i in range(m):
        assert pts[i].tobytes() == O.msm_g1(h, np.stack([_le(x) for x in t_rows[i]])), "T'[%d]" % i
    untouched = 0
    for j in range(n_aux):
        if n_in + j in q_rows:
            expect = O.msm_g1(np.concatenate([l[j:j + 1], h]), np.stack([_le(1)] + [_le(x) for x in q_rows[n_in + j]]))
        else:
            expect, untouched = l[j].tobytes(), untouched + 1     # absent from C: L' = L
        assert pts[m + j].tobytes() == expect, "L'[%d]" % j
    assert untouched > 0
    for t, v in enumerate(used):
        assert pts[m + n_aux + t].tobytes() == O.msm_g1(h, np.stack([_le(x) for x in q_rows[v]])), "input %d" % v
    # 2. the closed form: H_k = [tau^k Z(tau) / delta] G
    tau, delta = toxic[0] % R, toxic[4] % R
    hk = [pow(tau, k, R) * (pow(tau, m, R) - 1) % R * pow(delta, -1, R) % R for k in range(m - 1)]
    dot = lambda row: sum(a * b for a, b in zip(row, hk)) % R
    ls = _l_scalars(cs, toxic)
    scalars = [dot(t_rows[i]) for i in range(m)]
    scalars += [(ls[j] + (dot(q_rows[n_in + j]) if n_in + j in q_rows else 0)) % R for j in range(n_aux)]
    scalars += [dot(q_rows[v]) for v in used]
    assert all(scalars), "a derived base at infinity: pick another seed"
    expect = O.g1_mul_gen_many(np.stack([_le(x) for x in scalars]))
    assert pts.tobytes() == expect.tobytes()


def _prove(rig, form, logm, jobs):
    return rig.ctx[form].prove_batch([(rig.slot[logm],) + tuple(j) for j in jobs])


@pytest.mark.parametrize("n", [8, 9, 17, 7])
@pytest.mark.parametrize("logm", [4, 8, 10])
def test_proofs_are_the_same_bytes_in_both_forms(rig, logm, n):
    """8: the smallest batch; 9 and 17 cross ntt_sub_batch = 8 and 16; 7: lone proofs, which never use the evaluation form"""
    ref = rig.jobs(logm)[:n]
    jobs = [j[:4] for j in ref]
    got = {form: _prove(rig, form, logm, jobs) for form in (EVALUATION, COEFFICIENT)}
    assert got[EVALUATION] == got[COEFFICIENT]
    assert got[EVALUATION] == [j[4] for j in ref]


@pytest.mark.parametrize("logm", [4, 8])
def test_montgomery_aux_form(rig, logm):
    ref = rig.jobs(logm)[:9]
    mont = lambda aux: np.stack([_le(int.from_bytes(aux[k].tobytes(), "little") << 256) for k in range(aux.shape[0])])
    jobs = [(i, mont(a), r, s, None, AUX_MONTGOMERY) for i, a, r, s, _ in ref]
    got = {form: _prove(rig, form, logm, jobs) for form in (EVALUATION, COEFFICIENT)}
    assert got[EVALUATION] == got[COEFFICIENT] == [j[4] for j in ref]


@pytest.mark.parametrize("logm", [4, 8])
def test_a_violated_constraint_gives_the_same_bytes(rig, logm):
    """the identity is linear algebra in the witness: it does not assume that the witness satisfies the circuit"""
    cs = rig.cs[logm]
    jobs = [list(j[:4]) for j in rig.jobs(logm)[:9]]
    bad = jobs[3][1].copy()
    bad[cs.n_aux - 1] = _le(int.from_bytes(bad[cs.n_aux - 1].tobytes(), "little") + 1)   # the last aux: the output of the last constraint
    jobs[3][1] = bad
    assert O.r1cs_unsatisfied(cs, jobs[3][0], bad) != 0
    got = {form: _prove(rig, form, logm, jobs) for form in (EVALUATION, COEFFICIENT)}
    assert got[EVALUATION] == got[COEFFICIENT]
    assert got[EVALUATION][3] != rig.jobs(logm)[3][4]
    assert [p for k, p in enumerate(got[EVALUATION]) if k != 3] == [j[4] for k, j in enumerate(rig.jobs(logm)[:9]) if k != 3]


def test_a_call_that_mixes_jobs_with_their_own_abc(rig):
    """jobs with caller-supplied a, b, c cannot fold c: they keep the coefficient form, next to plain jobs in evaluation form"""
    logm = 8
    ref = rig.jobs(logm)
    jobs = []
    for k, (i, a, r, s, _) in enumerate(ref):
        abc = O.r1cs_eval(rig.cs[logm], i, a)[:3] if k % 2 else None
        jobs.append((i, a, r, s, abc))
    assert sum(1 for j in jobs if j[4] is None) >= 8 and sum(1 for j in jobs if j[4] is not None) >= 8
    got = {form: _prove(rig, form, logm, jobs) for form in (EVALUATION, COEFFICIENT)}
    assert got[EVALUATION] == got[COEFFICIENT] == [j[4] for j in ref]


def test_a_derived_base_at_infinity_keeps_the_coefficient_form(rig):
    """a toy CRS whose l query holds L_j = Q_j / (g^m - 1) for one aux column: L'_j is the point at infinity.  The load succeeds, the
    circuit reports the coefficient form and proves what the oracle proves from the same (doctored) parameters."""
    logm = 6
    cs, toxic = rig.cs[logm], rig.toxic[logm]
    m = 1 << logm
    _, q_rows = _dft_rows(cs)
    j = min(v for v in q_rows if v >= cs.n_inputs) - cs.n_inputs
    tau, delta = toxic[0] % R, toxic[4] % R
    hk = [pow(tau, k, R) * (pow(tau, m, R) - 1) % R * pow(delta, -1, R) % R for k in range(m - 1)]
    qs = sum(a * b for a, b in zip(q_rows[cs.n_inputs + j], hk)) % R
    assert qs != 0
    params = np.array(rig.params[logm], dtype=np.uint8, copy=True)
    _, _, l_at = _sections(params, cs)
    params[l_at + 96 * j:l_at + 96 * (j + 1)] = np.frombuffer(O.g1_mul_gen((-qs) % R)[0], dtype=np.uint8)
    ctx = rig.ctx[EVALUATION]
    slot = len(SHAPES)
    ctx.load_circuit(slot, params, cs)
    assert ctx.circuit_quotient_form(slot) == COEFFICIENT
    assert ctx.circuit_eval_bases(slot)[0].shape[0] == 0
    jobs = [j[:4] for j in rig.jobs(logm)[:9]]
    P = O.Params(params)
    assert ctx.prove_batch([(slot,) + tuple(jb) for jb in jobs]) == [O.create_proof(P, cs, *jb) for jb in jobs]
