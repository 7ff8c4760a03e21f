"""The MSM's accumulation and bucket tails on their own (msm_launch_accumulate with an nchunks of the test's, then msm_tails_enqueue:
k_msm_bucket_gather / k_msm_bucket_gather_split, k_msm_bucket_heavy, k_msm_heavy_join, k_msm_wsum_level, the block reductions, k_msm_combine),
through tests/native/msm_stages_dev.hip, over digit lists made by hand: `bkt` is read back and every bucket, the empty ones included,
compared with the model's bucket sum in affine coordinates, the result with the model's weighted sum.  The chunk length K = max(4,
ceil(total / nchunks)) is the test's choice, so a bucket can be placed to span a given number of chunks, to begin or end on a chunk boundary,
or to be a heavy bucket beyond the 256 that MSM_HEAVY_SPLIT workgroups share.  The workspace holds the byte 0xA5 before every call.
All four forms: G1 batch (FpOps, gather_split, heavy span 8), G1 lone (FpQuadOps, span 12, shared heavy buckets and their join), G2 batch
(Fp2PairOps), G2 lone (Fp2OctOps).
Run with `-m gpu` on an MI355X."""
import random

import pytest

import msm_stage_models as M
from pyref import F1, F2, G1, G2, R, ec_mul

pytestmark = pytest.mark.gpu

CURVE = {"g1": (F1, G1, 24), "g2": (F2, G2, 16)}
WIDTH = {8: 4, 128: 8, 256: 9, 2048: 12, 4096: 13}   # buckets -> window bits
HEAVY_SHARED = 2048 // 8                               # MSM_HEAVY_SLOTS / MSM_HEAVY_SPLIT


@pytest.fixture(scope="module")
def shim():
    import msm_stages_shim
    yield msm_stages_shim
    for curve in ("g1", "g2"):
        getattr(msm_stages_shim.load(curve), "mst_%s_release" % curve)()


_bases = {}


def bases_of(curve):
    if curve not in _bases:
        F, gen, n = CURVE[curve]
        rng = random.Random(len(curve) + n)
        _bases[curve] = tuple(ec_mul(F, gen, rng.randrange(1, R)) for _ in range(n))
    return _bases[curve]


def chunk_len(total, nchunks):
    return max(4, (total + nchunks - 1) // nchunks)   # msm_chunk_len


def span(start, b, K):
    """c1 - c0 of bucket b: the chunks its entries touch, less one"""
    return (start[b + 1] - 1) // K - start[b] // K


def length_for(pos, K, d, fill):
    """entries of a bucket that begins at `pos` and touches chunks c0 .. c0 + d: just into the last one, or to its end"""
    end_chunk = pos // K + d
    return (end_chunk + 1) * K - pos if fill else end_chunk * K + 1 - pos


class Lists:
    """digit lists of one proof, bucket after bucket, over the rows of a window table"""

    def __init__(self, nb, rows, rng):
        self.nb, self.rows, self.rng, self.runs = nb, rows, rng, [[] for _ in range(nb)]

    def entry(self):
        return self.rng.randrange(self.rows) | (self.rng.randrange(2) << 31)

    def fill(self, b, length):
        self.runs[b] += [self.entry() for _ in range(length)]

    def pos(self, b):
        return sum(len(r) for r in self.runs[:b])


def composite(nb, rows, rng, K, heavy_span):
    """eight buckets, the others empty: spans of heavy_span - 2 .. heavy_span + 1 chunk boundaries (a bucket is heavy from heavy_span on), buckets
    that begin and end exactly on a multiple of K, equal partials on both sides of a boundary (a doubling in the gather), P and -P alone in a
    bucket (its sum is infinity), and a bucket of one entry that is alone in the last chunk"""
    L = Lists(nb, rows, rng)
    at = [i * (nb // 8) for i in range(7)] + [nb - 1]
    for i, (d, fill) in enumerate([(heavy_span - 2, True), (heavy_span - 1, False), (heavy_span, True), (heavy_span + 1, True)]):
        L.fill(at[i], length_for(L.pos(at[i]), K, d, fill))
    assert L.pos(at[4]) % K == 0
    same = [L.entry() for _ in range(K)]
    L.runs[at[4]] = same + same[::-1]                     # chunk by chunk the same points: the two partials are equal
    r = rng.randrange(rows)
    L.runs[at[5]] = [r, r | 1 << 31]                      # P - P
    L.fill(at[6], K - L.pos(at[6]) % K)                   # up to the next multiple of K
    L.fill(at[7], 1)
    return L.runs


def one_bucket(nb, rows, rng, b, length):
    L = Lists(nb, rows, rng)
    L.fill(b, length)
    return L.runs


def scattered(nb, rows, rng, total):
    L = Lists(nb, rows, rng)
    for _ in range(total):
        L.runs[min(rng.randrange(nb), rng.randrange(nb))].append(L.entry())
    return L.runs


def check(shim, curve, c, proofs, nchunks, lone, heavy_span):
    """proofs: per proof the bucket runs -> the per-proof n_heavy the kernels counted (after comparing it with the rule)"""
    F = CURVE[curve][0]
    bases = tuple(M.from_ref(F, p) for p in bases_of(curve))
    rows = M.table(F, bases, c)
    laid = [M.layout(runs, 0) for runs in proofs]
    bkt, result, n_heavy = shim.tails(curve, bases, c, [w for _, w in laid], [s for s, _ in laid], nchunks, lone)
    nb = M.geom(c)[1]
    for p, runs in enumerate(proofs):
        want = [M.bucket_sum(F, [M.entry_point(F, rows, e) for e in run]) for run in runs]
        for b in range(nb):
            if bkt[p][b] != want[b]:
                assert bkt[p][b] == want[b], "proof %d bucket %d (%d entries at %d)" % (p, b, len(runs[b]), laid[p][0][b])
        assert result[p] == M.weighted_sum(F, want), "proof %d" % p
        start = laid[p][0]
        K = chunk_len(start[nb], nchunks)
        assert n_heavy[p] == sum(1 for b in range(nb) if runs[b] and span(start, b, K) >= heavy_span), "proof %d" % p
    return n_heavy


@pytest.mark.parametrize("nb", [8, 128, 256, 2048, 4096])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_batch_tails(shim, curve, nb):
    """np = 9: k_msm_bucket_gather_split, single-wave heavy buckets, g_log 3 .. 5 of the weighted sum (4096 buckets: 5)"""
    c, K, heavy_span = WIDTH[nb], 5, 8
    rng = random.Random(nb + len(curve))
    rows = len(bases_of(curve)) * M.geom(c)[0]
    first = composite(nb, rows, rng, K, heavy_span)
    total = sum(len(r) for r in first)
    nchunks = (total + K - 1) // K
    assert chunk_len(total, nchunks) == K and total % K == 1
    few = 40 if curve == "g2" else 150
    r = rng.randrange(rows)
    proofs = [first,
              one_bucket(nb, rows, rng, 0, total),                 # everything in bucket 0: one heavy bucket, all others empty
              one_bucket(nb, rows, rng, nb - 1, total - 3),        # ... in the last bucket
              [[] for _ in range(nb)],                             # no entries at all: the encoding of infinity
              [[r, r | 1 << 31]] + [[] for _ in range(nb - 1)],    # only P - P
              scattered(nb, rows, rng, few), scattered(nb, rows, rng, 3), composite(nb, rows, rng, 4, heavy_span), scattered(nb, rows, rng, 2 * few)]
    n_heavy = check(shim, curve, c, proofs, nchunks, False, heavy_span)
    assert n_heavy[0] == 2 and n_heavy[1] == 1 and n_heavy[3] == 0


@pytest.mark.parametrize("nb", [8, 128, 256, 2048])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_lone_tails(shim, curve, nb):
    """np = 1: the replicated forms, heavy span 12, every heavy bucket shared by eight workgroups and joined; 128 buckets: one weighted-sum
    workgroup (g_log 0), 256: g_log 2, 2048: a second level"""
    c, K, heavy_span = WIDTH[nb], 4, 12
    rng = random.Random(7 * nb + len(curve))
    rows = len(bases_of(curve)) * M.geom(c)[0]
    first = composite(nb, rows, rng, K, heavy_span)
    total = sum(len(r) for r in first)
    cases = [first, one_bucket(nb, rows, rng, 0, 70), one_bucket(nb, rows, rng, nb - 1, 61), [[] for _ in range(nb)], scattered(nb, rows, rng, 30)]
    heavy = []
    for runs in cases:
        t = sum(len(r) for r in runs)
        nchunks = max(1, (t + K - 1) // K)
        assert chunk_len(t, nchunks) == K
        heavy.append(check(shim, curve, c, [runs], nchunks, True, heavy_span)[0])
    assert heavy == [2, 1, 1, 0, 0]


@pytest.mark.parametrize("count", [256, 257, 300])
def test_lone_g1_heavy_buckets_beyond_the_shared_ones(shim, count):
    """2048 buckets, `count` of them heavy with 13 chunks each, the rest empty: beyond MSM_HEAVY_SLOTS / MSM_HEAVY_SPLIT = 256 a heavy bucket is
    summed by its first workgroup alone and k_msm_heavy_join must leave it alone.  (Through msm_tails_enqueue the join's grid holds min(nb, 256)
    buckets, so its own limit `lim` never decides: with `lim` taken as n_heavy the kernel computes the same, measured with such a build.)"""
    nb, c, K, heavy_span = 2048, 12, 4, 12
    rng = random.Random(count)
    rows = len(bases_of("g1")) * M.geom(c)[0]
    L = Lists(nb, rows, rng)
    for b in rng.sample(range(nb), count):
        L.fill(b, heavy_span * K + 1 + rng.randrange(K))   # ends in its 13th chunk; filled up to the next multiple of K below, so every run begins on one
    for b in range(nb):
        if L.runs[b]:
            L.fill(b, -len(L.runs[b]) % K)
    total = sum(len(r) for r in L.runs)
    nchunks = total // K
    assert total % K == 0 and chunk_len(total, nchunks) == K
    assert check(shim, "g1", c, [L.runs], nchunks, True, heavy_span) == [count]
    assert (count > HEAVY_SHARED) == (count in (257, 300))
