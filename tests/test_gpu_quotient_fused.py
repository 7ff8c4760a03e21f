"""The evaluation-form quotient in three kernels (masp_amd/csrc/device/ntt.hpp): each kernel on its own against Python big
integers (tests/quotient_model.py's plain stages, which tests/test_quotient_schedule_model.py ties to direct interpolation and evaluation),
the whole chain bit for bit against the seven launches it replaces, and end to end: the same proof bytes with either schedule
(masp_hip_ctx_set_quotient_schedule), in coefficient form and from the toxic-waste closed form.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import oracle_lib as O
import quotient_fused_shim as S
import quotient_model as Q
import toy_r1cs
from pyref import R

pytestmark = pytest.mark.gpu

MARK = int.from_bytes(bytes([S.MARKER]) * 32, "little")      # a word nothing wrote
GEN = 7                                                      # masp_amd/csrc/device/consts.hpp: FrCfg::GEN
FR = Q.Field(R, pow(GEN, (R - 1) >> 32, R), 32, GEN)
LT = 10                                                      # masp_amd/csrc/device/ntt_geom.h: NTT_LT
EVALUATION, COEFFICIENT = 0, 1
FUSED, SEPARATE = 0, 1


def _values(rng, n):
    """n field elements: the edges first, then random ones"""
    return ([0, 1, R - 1, 2, R - 2] + [rng.randrange(R) for _ in range(n)])[:n]


def _row_counts(logm):
    """1, m - 1, m, and a count that ends in the middle of the second tile's second row (its zero fill starts inside a row of the tile)"""
    m, cols = 1 << logm, 1 << (2 * LT - logm)
    return [1, (1 << LT) + cols + cols // 2, m - 1, m]


def test_the_tile_and_where_the_schedule_applies():
    """10 and 21 take the separate passes: below, a transform is one tile and has no top stages; above, they do not fit one tile"""
    assert S.tile_log() == LT
    assert [S.fused_ok(logm) for logm in (10, 11, 15, 16, 17, 20, 21)] == [False, True, True, True, True, True, False]


@pytest.mark.parametrize("logn", [1, 5, 11])
def test_powers_in_bit_reversed_order(logn):
    scale = pow(1 << logn, -1, R)
    assert S.powers_bitrev_gpu(logn, GEN, scale) == [pow(GEN, Q.rev(i, logn), R) * scale % R for i in range(1 << logn)]


# logm 11, 12, 13: one, two and three top stages — the single-stage loop alone, the paired loop alone, and both
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("logm,nrows", [(logm, n) for logm in (11, 12, 13) for n in _row_counts(logm)])
def test_first_kernel(logm, nrows, q):
    rng = random.Random(100 * logm + nrows)
    m, in_stride = 1 << logm, nrows + 5
    a, b = [], []
    for _ in range(q):
        a += _values(rng, nrows) + [rng.randrange(R) for _ in range(in_stride - nrows)]   # what lies behind a row is not part of it
        b += [rng.randrange(R) for _ in range(in_stride - 1)] + [R - 1]
    got = S.dif_top_gpu(a, b, in_stride, nrows, logm, q)
    assert len(got) == 2 * q * m
    for k, src in enumerate([a] * q + [b] * q):
        p = k % q
        want = Q.dif_top(FR, src[p * in_stride:(p + 1) * in_stride], nrows, logm, LT)
        assert got[k * m:(k + 1) * m] == want, "%s of proof %d" % ("ab"[k // q], p)


@pytest.mark.parametrize("np_", [1, 3])
@pytest.mark.parametrize("logm", [11, 12, 13])
def test_middle_kernel(logm, np_):
    rng = random.Random(200 * logm + np_)
    m = 1 << logm
    x = _values(rng, np_ * m)
    x[m - 1] = R - 1
    got = S.mid_gpu(x, logm, np_)
    for p in range(np_):
        assert got[p * m:(p + 1) * m] == Q.mid(FR, x[p * m:(p + 1) * m], logm, LT), "transform %d" % p


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("logm", [11, 12, 13])
def test_last_kernel(logm, q):
    """[a | b] of q proofs; rows y_stride > m apart, the words between them untouched"""
    rng = random.Random(300 * logm + q)
    m, y_stride = 1 << logm, (1 << logm) + 3
    x = _values(rng, 2 * q * m)
    x[-1] = R - 1
    got = S.dit_top_ab_gpu(x, logm, q, y_stride)
    assert len(got) == q * y_stride
    for p in range(q):
        assert got[p * y_stride + m:(p + 1) * y_stride] == [MARK] * (y_stride - m), "the gap behind row %d was written" % p
        want = Q.dit_top_ab(FR, x[p * m:(p + 1) * m], x[(q + p) * m:(q + p + 1) * m], logm, LT)
        assert got[p * y_stride:p * y_stride + m] == want, "proof %d" % p


def test_three_kernels_in_a_row_equal_interpolation_and_evaluation():
    """logm 11, two proofs, rows shorter than m: the kernels chained by hand against the O(m) closed form of the same quotient values —
    interpolate on H, evaluate on g H (here by the model's plain transforms, which the CPU suite ties to the direct sums)"""
    logm, q, nrows = 11, 2, 1500
    rng = random.Random(7)
    m, in_stride = 1 << logm, nrows + 1
    a, b = _values(rng, q * in_stride), [rng.randrange(R) for _ in range(q * in_stride)]
    x = S.mid_gpu(S.dif_top_gpu(a, b, in_stride, nrows, logm, q), logm, 2 * q)
    got = S.dit_top_ab_gpu(x, logm, q, m)
    for p in range(q):
        ra, rb = a[p * in_stride:(p + 1) * in_stride], b[p * in_stride:(p + 1) * in_stride]
        ya, yb = Q.mid(FR, Q.dif_top(FR, ra, nrows, logm, LT), logm, LT), Q.mid(FR, Q.dif_top(FR, rb, nrows, logm, LT), logm, LT)
        assert got[p * m:(p + 1) * m] == Q.dit_top_ab(FR, ya, yb, logm, LT)


# ---- the whole chain against the seven launches it replaces ----------------------------------------------------------------------
_TOP_LIMB = R >> 224


def _residues(rng, n):
    """u8[n, 32]: n words below r (any of them is a Montgomery residue), the edges first"""
    limbs = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64)
    limbs[:, 7] = rng.integers(0, _TOP_LIMB, size=n, dtype=np.uint64)                  # a top limb below r's: the word is below r
    out = limbs.astype("<u4").view(np.uint8).reshape(n, 32).copy()
    for k, v in enumerate((0, 1, R - 1)[:n]):
        out[k] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    return out


@pytest.mark.parametrize("q", [1, 3, 8])
@pytest.mark.parametrize("logm", [15, 16, 17])
def test_whole_chain_equals_the_separate_passes(logm, q):
    """the sizes of the three MASP circuits; rows end five short of m, lie three apart, and the output rows two"""
    rng = np.random.default_rng(1000 * logm + q)
    m = 1 << logm
    nrows, in_stride, y_stride = m - 5, m - 2, m + 2
    a, b = _residues(rng, q * in_stride), _residues(rng, q * in_stride)
    fused, separate = S.chains_gpu(a, b, in_stride, nrows, logm, q, y_stride)
    rows = separate.reshape(q, y_stride, 32)
    assert (rows[:, m:] == S.MARKER).all() and not (rows[:, :m] == S.MARKER).all(axis=2).any()
    assert np.array_equal(fused, separate)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
# logm 11 and 12: one and two top stages; logm 10: a domain of one tile, which runs the separate passes whatever is set
SHAPES = {10: dict(n_inputs=5, n_free=60, n_constraints=700, bool_share=0.7),
          11: dict(n_inputs=5, n_free=60, n_constraints=1500, bool_share=0.7),
          12: dict(n_inputs=4, n_free=80, n_constraints=3000, bool_share=0.6)}
N_JOBS = 17


def _every_aux_constrained(cs):
    """(an aux variable absent from all three matrices has the point at infinity in the l query, which no loader accepts)"""
    seen = set()
    for _, col, _ in cs.mats:
        seen.update(int(v) for v in col)
    return all(v in seen for v in range(cs.n_inputs, cs.n_inputs + cs.n_aux))


class Rig:
    """the circuits on two contexts, one in evaluation form (the default) and one in coefficient form; N_JOBS statements of each with
    their closed-form proofs"""

    def __init__(self):
        import masp_amd
        # ntt_sub_batch = 4: the three-kernel schedule takes twice that, sub-batches of eight — 8, 9 and 17 jobs are then one full
        # sub-batch, a tail of one, and more than two sub-batches; the separate passes and the coefficient form cut them in fours
        self.ctx = {EVALUATION: masp_amd.Context(0, ntt_sub_batch=4), COEFFICIENT: masp_amd.Context(0, ntt_sub_batch=4)}
        self.ctx[COEFFICIENT].set_quotient_form(COEFFICIENT)
        self.cs, self.toxic, self.slot, self.seed, self._jobs = {}, {}, {}, {}, {}
        for slot, (logm, shape) in enumerate(sorted(SHAPES.items())):
            self.seed[logm] = next(s for s in range(40 * logm, 40 * logm + 400) if _every_aux_constrained(toy_r1cs.make(s, **shape)[0]))
            cs = toy_r1cs.make(self.seed[logm], **shape)[0]
            assert cs.logm == logm
            self.cs[logm], self.slot[logm], self.toxic[logm] = cs, slot, toy_r1cs.toxic(900 + logm)
            params = self.ctx[EVALUATION].generate_parameters(cs, self.toxic[logm])
            for c in self.ctx.values():
                c.load_circuit(slot, params, cs)

    def jobs(self, logm):
        if logm not in self._jobs:
            rng = random.Random(9100 + logm)
            out = []
            for _ in range(N_JOBS):
                ins = [rng.randrange(R) for _ in range(SHAPES[logm]["n_inputs"] - 1)]
                _, inputs, aux, _ = toy_r1cs.make(self.seed[logm], input_values=ins, **SHAPES[logm])
                r, s = rng.randrange(R), rng.randrange(R)
                out.append((inputs, aux, r, s, O.closed_form_proof(self.cs[logm], self.toxic[logm], inputs, aux, r, s)))
            self._jobs[logm] = out
        return self._jobs[logm]

    def prove(self, form, logm, n):
        return self.ctx[form].prove_batch([(self.slot[logm],) + j[:4] for j in self.jobs(logm)[:n]])

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def test_the_schedule_switch(rig):
    import masp_amd
    ctx = rig.ctx[EVALUATION]
    assert ctx.quotient_schedule == FUSED                      # the default
    ctx.set_quotient_schedule(SEPARATE)
    assert ctx.quotient_schedule == SEPARATE and rig.ctx[COEFFICIENT].quotient_schedule == FUSED
    ctx.set_quotient_schedule(FUSED)
    assert ctx.quotient_schedule == FUSED
    with pytest.raises(masp_amd.MaspHipError):
        ctx.set_quotient_schedule(2)
    for logm in SHAPES:
        assert ctx.circuit_quotient_form(rig.slot[logm]) == EVALUATION
        assert rig.ctx[COEFFICIENT].circuit_quotient_form(rig.slot[logm]) == COEFFICIENT


# on the three-kernel schedule 8: one full sub-batch; 9: a tail sub-batch of one; 17: more than two sub-batches (see Rig)
@pytest.mark.parametrize("n", [8, 9, 17])
@pytest.mark.parametrize("logm", sorted(SHAPES))
def test_proofs_are_the_same_with_either_schedule(rig, logm, n):
    want = [j[4] for j in rig.jobs(logm)[:n]]
    ctx = rig.ctx[EVALUATION]
    assert ctx.circuit_quotient_form(rig.slot[logm]) == EVALUATION
    got = {}
    try:
        for schedule in (FUSED, SEPARATE):
            ctx.set_quotient_schedule(schedule)                # read when the batch is enqueued: the same context, the same circuit
            got[schedule] = rig.prove(EVALUATION, logm, n)
    finally:
        ctx.set_quotient_schedule(FUSED)
    coefficient = rig.prove(COEFFICIENT, logm, n)
    for name, proofs in (("fused", got[FUSED]), ("separate", got[SEPARATE]), ("coefficient form", coefficient)):
        bad = [k for k in range(n) if proofs[k] != want[k]]
        assert not bad, "logm %d, %d jobs, %s: proofs %r differ from the closed form" % (logm, n, name, bad)
