"""The prover's front half — everything between "a witness arrives" and "scalars go into the MSMs" — kernel by kernel against Python big
integers (tests/native/prove_stages_dev.hip launches each kernel through the product's own launch wrapper), and end to end on circuits
whose rows reach the wave path of k_r1cs_eval (tests/long_rows.py).  Every comparison is exact.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import long_rows
import oracle_lib as O
import prove_stages_shim as S
import toy_r1cs
from pyref import R

pytestmark = pytest.mark.gpu

MARK = int.from_bytes(bytes([S.MARKER]) * 32, "little")      # a word nothing wrote
TOP = (1 << 256) - 1
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)
GEN = 7                                                      # masp_amd/csrc/device/consts.hpp: FrCfg::GEN
EVALUATION, COEFFICIENT = 0, 1
N_JOBS = 9
E_RANGE = 8                                                  # MASP_HIP_E_RANGE


def _le(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)


def _values(rng, n):
    """n field elements: the edges first, then random ones"""
    return ([0, 1, R - 1, 2, R - 2] + [rng.randrange(R) for _ in range(n)])[:n]


# ---- k_r1cs_eval -----------------------------------------------------------------------------------------------------------------
_made = {}


def _shape(name):
    """(cs, [values of three witnesses], [their reference a, b, c]) of a named shape, built once"""
    if name not in _made:
        cs = long_rows.named(name)[0]
        vals = [long_rows.named(name, witness_seed=k)[3] for k in (None, 2, 3)]
        _made[name] = (cs, vals, [long_rows.reference_eval(cs, v) for v in vals])
    return _made[name]


def _check_eval(cs, assignments, want, n_mat):
    """k_r1cs_eval over `assignments` against want[proof][matrix][row]; the first bad entry as (matrix, proof, row, row length)"""
    orders, n_long = zip(*[long_rows.row_order(cs, which) for which in range(3)])
    got, flag = S.r1cs_eval_gpu(cs, orders, n_long, assignments, n_mat)
    assert flag == 0 and len(got) == n_mat
    for which in range(n_mat):
        lens = long_rows.row_lengths(cs, which) + [1 if which == 0 else 0] * cs.n_inputs
        for p in range(len(assignments)):
            for row in range(cs.nrows):
                g, w = got[which][p][row], want[p][which][row]
                if g != w:
                    raise AssertionError("matrix %s, proof %d of %d, row %d of %d (%d terms; n_long %r, n_mat %d): got %#x, want %#x%s" % (
                        "abc"[which], p, len(assignments), row, cs.nrows, lens[row], n_long, n_mat, g, w, " (never written)" if g == MARK * MONT_INV % R else ""))


@pytest.mark.parametrize("n_mat", [3, 2])
@pytest.mark.parametrize("n_proofs", [1, 3])
@pytest.mark.parametrize("name", long_rows.SHAPES)
def test_r1cs_eval(name, n_proofs, n_mat):
    """n_mat = 2 is the launch of a batch in evaluation form: A and B only, null pointers for C, the grid sized without C's long rows"""
    cs, vals, ref = _shape(name)
    _check_eval(cs, vals[:n_proofs], ref[:n_proofs], n_mat)


def _cs_of(n_inputs, n_aux, rows):
    """an R1cs from rows[matrix][row] = [(column, coefficient)], columns in the order given (repeats allowed)"""
    mats = []
    for m in rows:
        rp, col, coef = [0], [], []
        for terms in m:
            col += [v for v, _ in terms]
            coef += [_le(c % R) for _, c in terms]
            rp.append(len(col))
        mats.append((np.array(rp, np.uint32), np.array(col, np.uint32), np.stack(coef)))
    return long_rows.R1cs(n_inputs, n_aux, len(rows[0]), mats)


@pytest.mark.parametrize("n_mat", [3, 2])
def test_r1cs_eval_every_term_is_minus_one(n_mat):
    """577 terms (nine full strides of a wave and one lane) with every coefficient and every variable r - 1: each partial sum and each
    step of the shuffle tree reduces; the row is 577"""
    n_vars = 600
    row = lambda k, at: [(at + t, R - 1) for t in range(k)]
    rows = [[row(577, 0), row(64, 3), row(3, 1)], [row(1, 599), row(577, 23), row(63, 0)], [row(65, 9), row(2, 0), row(577, 11)]]
    cs = _cs_of(2, n_vars - 2, rows)
    vals = [R - 1] * n_vars
    ref = long_rows.reference_eval(cs, vals)
    assert ref[0][0] == ref[1][1] == ref[2][2] == 577 and ref[0][1] == 64
    _check_eval(cs, [vals], [ref], n_mat)


@pytest.mark.parametrize("n_mat", [3, 2])
def test_r1cs_eval_a_row_that_repeats_a_column(n_mat):
    """rows that name one column several times (a loader merges them; the kernel must not care): 130 terms over five columns on the wave
    path, three terms over one column on the lane path"""
    rng = random.Random(5)
    n_vars = 12
    many = lambda k: [(2 + t % 5, rng.randrange(1, R)) for t in range(k)]
    rows = [[many(130), [(3, 1), (3, R - 1), (3, 2)], many(64)], [[(7, 5)] * 3, many(65), [(0, 1)]], [many(63), [(11, 1), (11, 1)], many(129)]]
    cs = _cs_of(3, n_vars - 3, rows)
    vals = [_values(rng, n_vars), [rng.randrange(R) for _ in range(n_vars)]]
    ref = [long_rows.reference_eval(cs, v) for v in vals]
    assert ref[0][0][1] == 2 * vals[0][3] % R
    _check_eval(cs, vals, ref, n_mat)


# ---- k_fr_to_mont, k_fr_split_forms ----------------------------------------------------------------------------------------------
RANGE_N, RANGE_STRIDE, RANGE_NP = 300, 307, 3                # two blocks, the second one 44 lanes; rows seven elements apart


def _assignments(rng):
    """RANGE_NP rows of RANGE_N values below r, RANGE_STRIDE apart; the gaps hold 2^256 - 1, which no kernel may read"""
    x = []
    for _ in range(RANGE_NP):
        row = _values(rng, RANGE_N)
        rng.shuffle(row)
        x += row + [TOP] * (RANGE_STRIDE - RANGE_N)
    return x


def _rows(x, stride, n):
    return [x[p * stride + k] for p in range(len(x) // stride) for k in range(n)]


def _check_split(x, mont_from, flag_want, skip=()):
    """k_fr_split_forms (mont_from None: k_fr_to_mont) over x; `skip`: positions of x whose own output is not looked at"""
    if mont_from is None:
        y, flag = S.to_mont_gpu(x, RANGE_STRIDE, RANGE_N, RANGE_NP)
        after, mont_from = x, RANGE_N
    else:
        y, after, flag = S.split_forms_gpu(x, RANGE_STRIDE, RANGE_N, mont_from, RANGE_NP)
    assert flag == flag_want
    for p in range(RANGE_NP):
        for k in range(RANGE_STRIDE):
            at = p * RANGE_STRIDE + k
            if at in skip:
                continue
            v = x[at]
            if k >= RANGE_N:
                assert after[at] == v, "the gap behind row %d was written" % p
            elif k < mont_from:
                assert y[p * RANGE_N + k] == v * MONT % R and after[at] == v, (p, k)
            else:
                assert y[p * RANGE_N + k] == v and after[at] == v * MONT_INV % R, (p, k)


@pytest.mark.parametrize("mont_from", [None, 0, 129, 256, RANGE_N])
def test_to_mont_and_split_forms_in_range(mont_from):
    """0, 1 and r - 1 among the values; 2^256 - 1 in the gaps between rows: the flag stays 0"""
    x = _assignments(random.Random(11))
    assert {0, 1, R - 1} <= set(_rows(x, RANGE_STRIDE, RANGE_N))
    _check_split(x, mont_from, 0)


LAST = (RANGE_NP - 1) * RANGE_STRIDE + RANGE_N - 1             # the last element of the last proof: the tail of the last block, blockIdx.y > 0


@pytest.mark.parametrize("bad", [R, R + 1, TOP], ids=["r", "r+1", "2^256-1"])
@pytest.mark.parametrize("mont_from,at", [(None, 0), (None, LAST), (129, 0), (129, LAST), (129, RANGE_STRIDE + 128), (129, RANGE_STRIDE + 129),
                                          (256, 2 * RANGE_STRIDE + 255), (256, 2 * RANGE_STRIDE + 256), (0, 0), (RANGE_N, LAST)])
def test_one_value_out_of_range_raises_the_flag(mont_from, at, bad):
    """one value >= r, alone, at the first element, at the last element of the last proof, and on either side of mont_from; with r - 1
    in its place the flag stays 0 (test_to_mont_and_split_forms_in_range has r - 1 elsewhere; here it sits exactly there)"""
    x = _assignments(random.Random(12))
    x[at] = R - 1
    _check_split(x, mont_from, 0)
    x[at] = bad
    _check_split(x, mont_from, 1, skip={at})


# ---- k_gather_scalars, the bit-reversal and the pointwise kernels ----------------------------------------------------------------
def _sizes():
    out = []
    for logm in (1, 2, 7, 9):
        m = 1 << logm
        for nrows in sorted({1, m - 1, m}):
            for n_proofs in (1, 3):
                out.append((logm, nrows, n_proofs))
    return out


SIZES = pytest.mark.parametrize("logm,nrows,n_proofs", _sizes())


def _rev(k, logm):
    return int(format(k, "0%db" % logm)[::-1], 2)


def _strided(y, stride, n, n_proofs):
    """the rows of a strided output; the words between them must be what the unit put there"""
    assert len(y) == n_proofs * stride
    for p in range(n_proofs):
        assert y[p * stride + n:(p + 1) * stride] == [MARK] * (stride - n), "the gap behind row %d was written" % p
    return [y[p * stride:p * stride + n] for p in range(n_proofs)]


@SIZES
def test_gather_scalars(logm, nrows, n_proofs):
    rng = random.Random(100 * logm + nrows)
    src_stride = (1 << logm) + 3
    src = [rng.randrange(1 << 256) for _ in range(n_proofs * src_stride)]     # copied as they are: any 256-bit word
    idx = [rng.randrange(src_stride) for _ in range(nrows)]
    idx[0] = src_stride - 1
    for dst_stride in (0, nrows + 5):
        got = S.gather_scalars_gpu(src, src_stride, idx, n_proofs, dst_stride)
        rows = _strided(got, dst_stride or nrows, nrows, n_proofs)
        assert rows == [[src[p * src_stride + i] for i in idx] for p in range(n_proofs)]


@SIZES
def test_load_and_copy_bitrev(logm, nrows, n_proofs):
    rng = random.Random(200 * logm + nrows)
    m, x_stride = 1 << logm, nrows + 5
    x = []
    for _ in range(n_proofs):
        x += _values(rng, nrows) + [rng.randrange(R) for _ in range(x_stride - nrows)]     # what lies behind a row is not part of it
    for montgomery_in in (False, True):
        got = S.bitrev_gpu(montgomery_in, x, x_stride, nrows, logm, n_proofs)
        want = []
        for p in range(n_proofs):
            row = [0] * m
            for k in range(nrows):
                row[_rev(k, logm)] = x[p * x_stride + k]
            want += row
        assert got == want, "copy" if montgomery_in else "load"


@SIZES
def test_scale_and_ab_bitrev(logm, nrows, n_proofs):
    """(these two have no nrows: every size runs the whole domain)"""
    rng = random.Random(300 * logm + nrows)
    m = 1 << logm
    a, b = _values(rng, n_proofs * m), [rng.randrange(R) for _ in range(n_proofs * m)]
    scale = [pow(GEN, k, R) for k in range(m)]                                             # the coset shift's table
    want_s, want_ab = [0] * (n_proofs * m), [0] * (n_proofs * m)
    for p in range(n_proofs):
        for k in range(m):
            want_s[p * m + _rev(k, logm)] = a[p * m + k] * scale[k] % R
            want_ab[p * m + _rev(k, logm)] = a[p * m + k] * b[p * m + k] % R
    assert S.scale_bitrev_gpu(a, scale, logm, n_proofs) == want_s
    assert S.ab_bitrev_gpu(a, b, logm, n_proofs) == want_ab


@SIZES
def test_pointwise_kernels_with_strided_output(logm, nrows, n_proofs):
    """k_ntt_ab_eval, k_fr_scale_sub, k_fr_scale over n = nrows elements per proof into rows y_stride > n apart"""
    rng = random.Random(400 * logm + nrows)
    n, m, y_stride = nrows, 1 << logm, nrows + 3
    a, b = _values(rng, n_proofs * n), [rng.randrange(R) for _ in range(n_proofs * n)]
    c = [rng.randrange(R) for _ in range(n_proofs * n - 1)] + [R - 1]
    g_inv, m_inv = pow(GEN, -1, R), pow(m, -1, R)
    scale = [pow(g_inv, k, R) * m_inv % R for k in range(n)]                                # the inverse coset transform's table
    cscale = pow(pow(GEN, m, R) - 1, -1, R)                                                 # 1 / (g^m - 1)
    rows = lambda f: [[f(p * n + k, k) for k in range(n)] for p in range(n_proofs)]
    assert _strided(S.ab_eval_gpu(a, b, cscale, n, n_proofs, y_stride), y_stride, n, n_proofs) == rows(lambda i, k: a[i] * b[i] * cscale % R)
    for stride in (y_stride, 0):
        got = S.fr_scale_gpu(a, scale, n, n_proofs, stride, c=c, cscale=cscale)
        assert _strided(got, stride or n, n, n_proofs) == rows(lambda i, k: (a[i] * scale[k] - c[i] * cscale) % R)
        got = S.fr_scale_gpu(a, scale, n, n_proofs, stride)
        assert _strided(got, stride or n, n, n_proofs) == rows(lambda i, k: a[i] * scale[k] % R)


# ---- end to end on the long-row circuits -----------------------------------------------------------------------------------------
class Rig:
    """the four shapes on two contexts, one in evaluation form (the default) and one in coefficient form; per shape nine jobs with
    distinct (r, s) over two witnesses, and both oracle proofs of each, computed when first asked for"""

    def __init__(self):
        import masp_amd
        self.ctx = {EVALUATION: masp_amd.Context(0), COEFFICIENT: masp_amd.Context(0)}
        self.ctx[COEFFICIENT].set_quotient_form(COEFFICIENT)
        self.slot = {name: k for k, name in enumerate(long_rows.SHAPES)}
        self._loaded, self._jobs = {}, {}

    def circuit(self, name):
        """(cs, toxic, params) of a shape, loaded into both contexts"""
        if name not in self._loaded:
            cs = long_rows.named(name)[0]
            toxic = toy_r1cs.toxic(500 + self.slot[name])
            params = self.ctx[EVALUATION].generate_parameters(cs, toxic)
            for c in self.ctx.values():
                c.load_circuit(self.slot[name], params, cs)
            self._loaded[name] = (cs, toxic, params, O.Params(params))
        return self._loaded[name][:3]

    def jobs(self, name):
        """[(inputs, aux, r, s)] x N_JOBS and their proofs"""
        if name not in self._jobs:
            cs, toxic, _ = self.circuit(name)
            rng = random.Random(600 + self.slot[name])
            witness = [long_rows.named(name, witness_seed=k)[1:3] for k in (None, 2)]
            jobs = [witness[k % 2] + (rng.randrange(R), rng.randrange(R)) for k in range(N_JOBS)]
            proofs = [O.closed_form_proof(cs, toxic, *j) for j in jobs]
            assert proofs == [self.oracle_proof(name, j) for j in jobs]
            self._jobs[name] = (jobs, proofs)
        return self._jobs[name]

    def oracle_proof(self, name, job):
        return O.create_proof(self._loaded[name][3], self._loaded[name][0], *job)

    def prove(self, form, name, jobs):
        return self.ctx[form].prove_batch([(self.slot[name],) + tuple(j) for j in jobs])

    def close(self):
        self._loaded.clear()
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.mark.parametrize("name", long_rows.SHAPES)
def test_parameters_and_forms_of_the_long_row_circuits(rig, name):
    cs, toxic, params = rig.circuit(name)
    assert params.tobytes() == O.generate_parameters(cs, toxic).tobytes()
    # (a derived base at infinity would keep the circuit in coefficient form, and the launch of A and B alone would never run: pick another seed)
    assert rig.ctx[EVALUATION].circuit_quotient_form(rig.slot[name]) == EVALUATION
    assert rig.ctx[COEFFICIENT].circuit_quotient_form(rig.slot[name]) == COEFFICIENT
    jobs, proofs = rig.jobs(name)
    public = [int.from_bytes(jobs[0][0][k].tobytes(), "little") for k in range(1, cs.n_inputs)]
    assert O.verify_proof(params, proofs[0], public) == 1


@pytest.mark.parametrize("n", [1, 7, 8, 9])
@pytest.mark.parametrize("form", [EVALUATION, COEFFICIENT], ids=["evaluation", "coefficient"])
@pytest.mark.parametrize("name", long_rows.SHAPES)
def test_proofs_of_the_long_row_circuits(rig, name, form, n):
    """1 and 7: lone proofs; 8: the smallest batch; 9 crosses ntt_sub_batch = 8"""
    jobs, proofs = rig.jobs(name)
    assert rig.ctx[form].circuit_quotient_form(rig.slot[name]) == form
    got = rig.prove(form, name, jobs[:n])
    bad = [k for k in range(n) if got[k] != proofs[k]]
    assert not bad, "%s, %d jobs: proofs %r differ from the oracle's" % (name, n, bad)


@pytest.mark.parametrize("form", [EVALUATION, COEFFICIENT], ids=["evaluation", "coefficient"])
@pytest.mark.parametrize("name", long_rows.SHAPES)
def test_range_boundary_in_a_batch(rig, name, form):
    """r at the last aux of the last job of nine, and at input 1 of job 4: refused; r - 1 there: the oracle's proofs"""
    import masp_amd
    cs = rig.circuit(name)[0]
    jobs, proofs = rig.jobs(name)
    for job, field, at in ((N_JOBS - 1, 1, cs.n_aux - 1), (4, 0, 1)):
        for value in (R, R - 1):
            changed = [list(j) for j in jobs]
            changed[job][field] = changed[job][field].copy()
            changed[job][field][at] = _le(value)
            if value == R:
                with pytest.raises(masp_amd.MaspHipError) as e:
                    rig.prove(form, name, changed)
                assert e.value.code == E_RANGE
            else:
                want = list(proofs)
                want[job] = rig.oracle_proof(name, tuple(changed[job]))
                assert want[job] != proofs[job]
                assert rig.prove(form, name, changed) == want
