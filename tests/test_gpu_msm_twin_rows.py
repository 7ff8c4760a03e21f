"""Doubled window rows (masp_amd/csrc/device/msm_geom.h: msm_geom_twin; masp_hip_ctx_set_window_row_multiples): a digit magnitude of odd
valuation is an entry of the window's doubled row in the bucket of half the magnitude, so an MSM has two thirds as many buckets.  Stage by
stage through tests/native/msm_twin_dev.hip against the Python model (tests/msm_twin_models.py) — the sort's digit list, the table the
loader builds, the bucket tails over the classes of odd weights —, then end to end: the same MSM and the same proofs with the mode on and
off, byte for byte, against the oracle.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import msm_stage_models as M
import msm_twin_models as TM
import oracle_lib as O
import toy_r1cs
from pyref import F1, F2, G1, G2, R, ec_mul

pytestmark = pytest.mark.gpu

N_SORT, NP_SORT = 200, 3
SUBSET = (2, 16, 24, {3})        # blocks of four scalars, blocks 16 .. 23 = scalars 64 .. 95, block 19 (relative 3) marked bad


@pytest.fixture(scope="module")
def shim():
    import msm_twin_shim
    return msm_twin_shim


def _digits_to_scalar(ds, c):
    return sum(d << (c * j) for j, d in enumerate(ds))


def sort_scalars(c, p):
    """proof p's 200 scalars: the edges the recoding can go wrong at, a block of booleans under the subset rows, random ones"""
    rng = random.Random(100 * c + p)
    half = 1 << (c - 1)
    v = [0, 1, R - 1, R - 2, 2, 3, 4, 8]
    v += [half, half + 1, half - 1, (half << c) | half, ((half + 1) << c) | (half + 1)]       # the sign threshold, and one above: a carry
    v += [_digits_to_scalar([1 << t, 0, 1 << t, 3 << t], c) for t in range(min(4, c - 1))]    # magnitudes of valuation 0, 1, 2, 3
    v += [_digits_to_scalar([(1 << c) - (1 << t)], c) for t in range(min(4, c - 1))]          # ... and negative ones: 2^c - 2^t -> -2^t, carry
    v += M.edge_scalars(c, rng, 4)[:40]
    v = v[:64] + [rng.randrange(R) for _ in range(64 - len(v))]
    assert len(v) == 64
    block = [rng.randrange(2) for _ in range(32)]                                              # scalars 64 .. 95: booleans
    block[0:4] = [1, 1, 1, 1]
    block[4:8] = [0, 0, 0, 0]
    block[8:12] = [0, 1, 0, 2] if p == 1 else block[8:12]                                      # a covered block that is not all boolean
    v += block
    v += [rng.randrange(2) for _ in range(20)]                                                 # booleans outside the covered range
    v += [rng.randrange(R) for _ in range(N_SORT - len(v))]
    return v


@pytest.mark.parametrize("subset", [None, SUBSET], ids=["plain", "subset"])
@pytest.mark.parametrize("c", [4, 5, 8, 12])
def test_sort_against_the_model(shim, c, subset):
    """entries (row, sign), starts and padded runs of three proofs; c = 12 takes the two-pass placement (k_msm_partition / k_msm_bucketize),
    the narrower windows k_msm_scatter.  With subset rows the first of them is row 2 W n, no longer W n."""
    scalars = [sort_scalars(c, p) for p in range(NP_SORT)]
    W, nb = TM.geom(c)
    pad_log = 2
    start, dense, words, stride = shim.sort(scalars, c, pad_log, subset)
    for p in range(NP_SORT):
        runs = TM.entries(scalars[p], N_SORT, c, subset)
        assert len(runs) == nb
        want_start, _ = M.layout(runs, pad_log)
        assert start[p] == want_start
        assert dense[p] == M.scan([len(r) for r in runs])
        for b, r in enumerate(runs):
            got = words[p][start[p][b]:start[p][b + 1]]
            assert sorted(got[:len(r)]) == r, (p, b)
            assert got[len(r):] == [M.PAD_ENTRY] * (len(got) - len(r)), (p, b)
        if subset is not None:
            sub = [e for e in runs[0] if 2 * W * N_SORT <= e < 1 << 31]           # (positive entries: bit 31 is the sign)
            assert sub and all(e < 2 * W * N_SORT + 8 * 15 for e in sub)


CURVE = {"g1": (F1, G1), "g2": (F2, G2)}
_bases = {}


def bases_of(curve, n):
    if (curve, n) not in _bases:
        F, gen = CURVE[curve]
        rng = random.Random(len(curve) + n)
        _bases[(curve, n)] = tuple(M.from_ref(F, ec_mul(F, gen, rng.randrange(1, R))) for _ in range(n))
    return _bases[(curve, n)]


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_doubled_rows_are_twice_the_window_rows(shim, curve):
    F = CURVE[curve][0]
    c, bases = 13, bases_of(curve, 6)
    W, nb = TM.geom(c)
    rows, info = shim.table(curve, bases, c)
    assert (info["twin"], info["W"], info["nb"], info["rows"], info["status"]) == (1, W, nb, 2 * W * 6, 0)
    assert rows == TM.table(F, bases, c)
    # subset rows move behind the doubled rows
    bases8 = bases_of(curve, 8)
    rows, info = shim.table(curve, bases8, c, sub_bits=2)
    assert info["twin"] == 1 and info["row0"] == 2 * W * 8 and info["rows"] == 2 * W * 8 + 2 * 15
    assert rows[:2 * W * 8] == TM.table(F, bases8, c)
    assert rows[2 * W * 8] == bases8[0] and rows[2 * W * 8 + 15] == bases8[4]


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_a_base_at_infinity_keeps_the_set_plain(shim, curve):
    """These curves have no point of order two, so the only row that doubles to infinity is one at infinity already: a set with such a base
    keeps the plain geometry (no entry of a twin set names a row at infinity), its table what it was."""
    F = CURVE[curve][0]
    c = 13
    bases = bases_of(curve, 6)[:3] + (M.inf(F),) + bases_of(curve, 6)[4:]
    rows, info = shim.table(curve, bases, c)
    W, nb = M.geom(c)
    assert (info["twin"], info["W"], info["nb"], info["rows"]) == (0, W, nb, W * 6)
    assert rows == M.table(F, bases, c)


def hand_made(curve, c, np_, rng, n_rows, fill):
    """per proof the bucket runs: a few entries in a scattering of buckets, every class's first and last bucket among them"""
    _, nb = TM.geom(c)
    nbk = len(TM.values(c))
    edge = sorted({b for off, size, _ in TM.classes(c) for b in (off, off + size - 1)})
    proofs = []
    for p in range(np_):
        runs = [[] for _ in range(nb)]
        if fill:
            for b in edge + [rng.randrange(nbk) for _ in range(12)]:
                runs[b] += [rng.randrange(n_rows) | (rng.randrange(2) << 31) for _ in range(1 + rng.randrange(3))]
        proofs.append(runs)
    return proofs


@pytest.mark.parametrize("fill", [True, False], ids=["filled", "empty"])
@pytest.mark.parametrize("np_,lone", [(1, True), (3, True), (3, False)])
@pytest.mark.parametrize("c", [4, 7, 12])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_tails_weigh_every_bucket_by_its_value(shim, curve, c, np_, lone, fill):
    """c = 4 and 7: every class is smaller than a chunk (the last workgroup's dense form alone); c = 12: class 0 is a whole chunk"""
    F = CURVE[curve][0]
    n = 3
    bases = bases_of(curve, n)
    W, nb = TM.geom(c)
    rows = TM.table(F, bases, c)
    rng = random.Random(1000 * c + np_ + (7 if lone else 0))
    proofs = hand_made(curve, c, np_, rng, len(rows), fill)
    laid = [M.layout(runs, 0) for runs in proofs]
    bkt, result = shim.tails(curve, bases, c, [w for _, w in laid], [s for s, _ in laid], 8, lone)
    for p, runs in enumerate(proofs):
        want = [M.bucket_sum(F, [M.entry_point(F, rows, e) for e in r]) for r in runs]
        assert bkt[p] == want
        assert result[p] == TM.weighted_sum(F, c, want)
        if not fill:
            assert result[p] == M.inf(F)


# ---- end to end ----
def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import masp_amd
    c = masp_amd.Context(0)
    yield c
    c.close()


N_MSM = 3000


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_an_msm_is_the_same_bytes_with_the_mode_on_and_off(ctx, group):
    """3 000 points, a lone MSM and a batch of nine (the bucket tree in front), 13- and 16-bit windows (16: class 0 is two chunks of the
    weighted sum), a witness-like mix of scalars"""
    rng = random.Random(31 + len(group))
    mul_gen, msm, fn = (O.g1_mul_gen_many, O.msm_g1, ctx.msm_g1_multi_ex) if group == "g1" else (O.g2_mul_gen_many, O.msm_g2, ctx.msm_g2_multi_ex)
    bases = mul_gen(np.stack([_le(rng.randrange(1, R)) for _ in range(N_MSM)]))
    vecs = [[rng.choice((0, 1, 1, rng.randrange(R), rng.randrange(R))) for _ in range(N_MSM)] for _ in range(9)]
    sc = np.stack([np.stack([_le(s) for s in v]) for v in vecs])
    want = [msm(bases, sc[p]) for p in range(9)]
    try:
        for mode, mask in ((-1, 0), (1, 3)):
            ctx.set_window_row_multiples(mode)
            assert ctx.window_row_multiples == mask
            for window_bits in (13, 16):
                for np_ in (1, 9):
                    got, _ = fn(bases, sc[:np_], window_bits=window_bits, block_bits=2)
                    assert got == want[:np_], (mode, window_bits, np_)
    finally:
        ctx.set_window_row_multiples(0)


def test_the_setting_and_its_values(ctx):
    default = ctx.window_row_multiples
    assert default in (0, 1, 3)
    try:
        for v, mask in ((-1, 0), (1, 3), (2, 1), (0, default)):
            ctx.set_window_row_multiples(v)
            assert ctx.window_row_multiples == mask
        for bad in (3, -2):
            with pytest.raises(Exception):
                ctx.set_window_row_multiples(bad)
    finally:
        ctx.set_window_row_multiples(0)


@pytest.mark.parametrize("form", [0, 1], ids=["evaluation", "coefficient"])
def test_a_small_circuit_proves_the_same_bytes_in_every_mode(ctx, form):
    """lone, and in batches of 1, 8 and 9; the mode off, on for every batch table and on for h + l only; against the closed form"""
    shape = dict(n_inputs=5, n_free=300, n_constraints=900, bool_share=0.7)
    cs, inputs, aux, _ = toy_r1cs.make(4321, **shape)
    tw = toy_r1cs.toxic(4321)
    params = ctx.generate_parameters(cs, tw)
    rs = [(6000 + 2 * k, 6001 + 2 * k) for k in range(9)]
    want = [O.closed_form_proof(cs, tw, inputs, aux, r, s) for r, s in rs]
    try:
        ctx.set_quotient_form(form)
        for mode in (-1, 1, 2):
            ctx.set_window_row_multiples(mode)
            ctx.load_circuit(0, params, cs)
            got = ctx.circuit_window_row_multiples(0)
            assert got & ~2 == {-1: 0, 1: 0b11101, 2: 0b00001}[mode]                    # what the tables really are ...
            assert bool(got & 2) == (mode != -1 and ctx.circuit_quotient_form(0) == 0)  # ... the evaluation form's, if it has one
            assert ctx.prove(0, inputs, aux, *rs[0]) == want[0]
            for n in (1, 8, 9):
                assert ctx.prove_batch([(0, inputs, aux, r, s) for r, s in rs[:n]]) == want[:n], (mode, n)
    finally:
        ctx.set_quotient_form(0)
        ctx.set_window_row_multiples(0)


def test_a_real_spend_batch_with_the_mode_on(ctx):
    """nine proofs of the real Spend circuit (16-bit windows for h + l: 21 845 buckets in 21 888), every batch table doubled"""
    from masp_amd import host as H
    from masp_amd.synthetic import toxic_waste
    from test_circuits import spend_instance
    cs, _ = H.circuit("spend")
    tw = toxic_waste(15)
    params = ctx.generate_parameters(cs, tw)
    jobs, want = [], []
    for k in range(9):
        inst, _, _ = spend_instance(400 + k, value=10 + k)
        inputs, aux, _, _, _ = H.spend_assignment(check=False, **inst)
        r, s = 70000 + k, 80000 + k
        jobs.append((0, inputs, aux, r, s))
        want.append(O.closed_form_proof(cs, tw, inputs, aux, r, s))
    try:
        ctx.set_window_row_multiples(1)
        ctx.load_circuit(0, params, cs)
        assert ctx.prove_batch(jobs) == want
    finally:
        ctx.set_window_row_multiples(0)
