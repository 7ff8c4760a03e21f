"""The batch-affine pre-reduction of the bucket runs (masp_amd/csrc/device/msm_tree.hpp: pairwise affine additions whose
inversions are shared across the grid) through the C ABI, in the regime that uses it (np >= 8 MSMs per launch sequence):
against the CPU restatement's multiexp on every exceptional case of the affine group law — P + P (a doubling inside the
shared inversion), P + (-P) (the point at infinity as a RESULT that later levels meet as an operand), bases at infinity,
buckets of every length around the powers of two — for G1 and G2, with the tree forced to more levels than any run is long,
switched off (the XYZZ accumulation alone must give the same points), and in sub-batches that do not divide the batch.
Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import oracle_lib as O
from pyref import F1, G1, R, ec_add, ec_mul, g1_unc

pytestmark = pytest.mark.gpu


def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), np.uint8)


def _rand(rng, n):
    return np.stack([_le(rng.randrange(R)) for _ in range(n)])


@pytest.fixture(scope="module")
def ctxs():
    import masp_amd
    made = {"auto": masp_amd.Context(0), "off": masp_amd.Context(0, bucket_tree_levels=-1),
            "deep": masp_amd.Context(0, bucket_tree_levels=11, bucket_tree_sub_batch=5)}
    assert made["off"].options["bucket_tree_levels"] == -1 and made["deep"].options["bucket_tree_sub_batch"] == 5
    yield made
    for c in made.values():
        c.close()


def _cases(rng, n, mul_gen):
    """-> bases, list of scalar vectors (one per proof of the batch)"""
    half = n // 2
    ks = _rand(rng, half)
    kneg = np.stack([_le(R - int.from_bytes(k.tobytes(), "little")) for k in ks])
    pm = mul_gen(np.concatenate([ks, kneg]))                 # P_0 .. P_{h-1}, -P_0 .. -P_{h-1}
    vec = []
    vec.append(np.tile(_le(3), (n, 1)))                      # every P meets its -P in the same bucket: infinity everywhere
    vec.append(np.tile(_le(0x1234567), (n, 1)))              # the same, on several windows
    same = _rand(rng, half)
    vec.append(np.concatenate([same, same]))                 # P and -P with the same random scalar
    v = _rand(rng, n)
    v[::7] = _le(0)
    v[1::7] = _le(1)
    v[2::7] = _le(R - 1)
    vec.append(v)                                            # zeros, ones, -1
    for _ in range(12):
        vec.append(_rand(rng, n))
    return pm, np.stack(vec)


@pytest.mark.parametrize("window_bits", [4, 7, 12])
@pytest.mark.parametrize("which", ["auto", "off", "deep"])
def test_g1_batch_of_msms_with_every_exceptional_pair(ctxs, which, window_bits):
    rng = random.Random(1000 + window_bits)
    n = 640
    pm, sc = _cases(rng, n, O.g1_mul_gen_many)
    want = [O.msm_g1(pm, sc[p]) for p in range(sc.shape[0])]
    assert ctxs[which].msm_g1_multi(pm, sc, window_bits=window_bits) == want
    # the same point n times: every pair of every level is a doubling
    one = O.g1_mul_gen_many(_rand(rng, 1))
    rep = np.tile(one, (n, 1))
    sc2 = np.stack([np.tile(_le(rng.randrange(R)), (n, 1)) for _ in range(8)] + [_rand(rng, n) for _ in range(3)])
    assert ctxs[which].msm_g1_multi(rep, sc2, window_bits=window_bits) == [O.msm_g1(rep, sc2[p]) for p in range(sc2.shape[0])]
    # bases at infinity among ordinary ones
    mixed = pm.copy()
    mixed[3::5, :] = 0
    mixed[3::5, 0] = 0x40
    assert ctxs[which].msm_g1_multi(mixed, sc[3:13], window_bits=window_bits) == [O.msm_g1(mixed, sc[p]) for p in range(3, 13)]


def _x_zero_case(rng, n, nvec):
    """bases t_i T + [k_i] G with T = (0, 2) of order 3 (on the curve, outside the subgroup, accepted by the loader, which checks
    flags and canonical encoding only): (0, 2), (0, p - 2) and their sums with ordinary points among ordinary bases, runs of them side
    by side.  x = 0 is what marks the point at infinity inside the bucket tree (k_tree_pass1 / k_tree_pass2: O::is_zero(c.x1)): these
    are the only inputs that reach that branch without being infinity.  -> bases, scalar vectors, expected results from pyref"""
    T = (0, 2)
    ts = [rng.choice([0, 1, 2]) for _ in range(n)]
    ts[:6] = [1, 1, 2, 2, 1, 2]
    ks = [0 if i < 6 else rng.randrange(1, R) for i in range(n)]
    pts = [ec_add(F1, ec_mul(F1, T, t), ec_mul(F1, G1, k)) for t, k in zip(ts, ks)]
    bases = np.stack([np.frombuffer(g1_unc(p), np.uint8) for p in pts])
    vecs = [np.tile(_le(s), (n, 1)) for s in (1, 3, 0x1234567)] + [_rand(rng, n) for _ in range(nvec - 3)]
    want = []
    for v in vecs:
        sc = [int.from_bytes(v[i].tobytes(), "little") for i in range(n)]
        want.append(g1_unc(ec_add(F1, ec_mul(F1, T, sum(s * t for s, t in zip(sc, ts)) % 3),
                                  ec_mul(F1, G1, sum(s * k for s, k in zip(sc, ks)) % R))))
    return bases, np.stack(vecs), want


@pytest.mark.parametrize("which", ["auto", "off", "deep"])
def test_g1_bases_with_x_zero(ctxs, which):
    rng = random.Random(3000)
    bases, sc, want = _x_zero_case(rng, 40, 10)
    assert [bytes(b) for b in ctxs[which].msm_g1_multi(bases, sc, window_bits=4)] == want
    assert [bytes(b) for b in ctxs[which].msm_g1_multi(bases, sc, window_bits=7)] == want
    # the lone path (msm_g1: one MSM)
    for p in range(4):
        assert ctxs[which].msm_g1(bases, sc[p]) == want[p], p


@pytest.mark.parametrize("which", ["auto", "off", "deep"])
def test_g2_batch_of_msms_with_every_exceptional_pair(ctxs, which):
    rng = random.Random(2000)
    n = 320
    pm, sc = _cases(rng, n, O.g2_mul_gen_many)
    sc = sc[:10]
    want = [O.msm_g2(pm, sc[p]) for p in range(sc.shape[0])]
    assert ctxs[which].msm_g2_multi(pm, sc, window_bits=7) == want
    one = O.g2_mul_gen_many(_rand(rng, 1))
    rep = np.tile(one, (n, 1))
    sc2 = np.stack([np.tile(_le(rng.randrange(R)), (n, 1)) for _ in range(6)] + [_rand(rng, n) for _ in range(2)])
    assert ctxs[which].msm_g2_multi(rep, sc2, window_bits=7) == [O.msm_g2(rep, sc2[p]) for p in range(sc2.shape[0])]


def test_bucket_runs_of_every_length_around_the_powers_of_two(ctxs):
    """Scalars chosen so that bucket b of the only window holds exactly b + 1 entries (b = 0 .. 63: lengths 1 .. 64, every
    odd / even / power-of-two pattern of pairs and pass-through points), by the discrete-log identity."""
    rng = random.Random(3000)
    digits = [d for d in range(1, 65) for _ in range(d)]          # digit d appears d times
    n = len(digits)
    k_int = [rng.randrange(R) for _ in range(n)]
    bases = O.g1_mul_gen_many(np.stack([_le(k) for k in k_int]))
    np_ = 9
    sc, totals = [], []
    for p in range(np_):
        order = digits[:]
        rng.shuffle(order)
        sc.append(np.stack([_le(d) for d in order]))
        totals.append(sum(a * b for a, b in zip(k_int, order)) % R)
    want = O.g1_mul_gen_many(np.stack([_le(t) for t in totals]))
    for which in ("auto", "deep", "off"):
        assert ctxs[which].msm_g1_multi(bases, np.stack(sc), window_bits=8) == [want[p].tobytes() for p in range(np_)]


def test_tree_scratch_that_does_not_fit_falls_back_instead_of_failing():
    """The tree's scratch is ~0.4 GB per Spend proof.  Where it does not fit (a smaller GPU, more slots, a second prover on the
    device — forced here with masp_hip_options::bucket_tree_scratch_mb) the sub-batch is halved, then the rest of the batch goes
    through the XYZZ accumulation: the same bytes, no error, and masp_hip_ctx_get_options says what happened (VERDICT r03 item 7,
    ADVICE r03)."""
    import masp_amd
    n, np_ = 8000, 40
    rng = random.Random(91)
    k_int = [rng.randrange(1, R) for _ in range(n)]
    bases = O.g1_mul_gen_many(np.stack([_le(k) for k in k_int]))
    sc = np.zeros((np_, n, 32), np.uint8)
    for p in range(np_):
        sc[p] = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(n)), np.uint8).reshape(n, 32)
    plain = masp_amd.Context(0, slots=1, bucket_tree_sub_batch=32)
    try:
        want = plain.msm_g1_multi(bases, sc, window_bits=12)
        assert plain.current_options()["bucket_tree_fallback_proofs"] == 0
    finally:
        plain.close()
    # (the scratch of this shape: ~565 / 282 / 141 MiB for sub-batches of 32 / 16 / 8 proofs)
    # 200 MiB: 32 and 16 proofs do not fit, 8 do -> halved twice, nothing falls back
    # 16 MiB: not even 8 proofs fit -> the whole batch through the XYZZ accumulation
    for mb, sub_after, fell_back in ((200, 8, False), (16, 8, True)):
        ctx = masp_amd.Context(0, slots=1, bucket_tree_sub_batch=32, bucket_tree_scratch_mb=mb)
        try:
            assert ctx.msm_g1_multi(bases, sc, window_bits=12) == want
            now = ctx.current_options()
            assert now["bucket_tree_sub_batch"] <= sub_after, now
            assert (now["bucket_tree_fallback_proofs"] > 0) == fell_back, now
        finally:
            ctx.close()
