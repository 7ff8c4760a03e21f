"""The MSM's counting sort on its own (msm_sort_enqueue: k_msm_hist, k_msm_offsets_*, then k_msm_scatter or k_msm_coarse / k_msm_partition /
k_msm_bucketize), through tests/native/msm_stages_dev.hip: `start`, `dense` and `sorted` read back and compared, proof by proof and bucket by
bucket, with the entries model of tests/msm_stage_models.py — as multisets, because the order inside a run is decided by atomics.  Every buffer
of the MsmSortBuf holds the byte 0xA5 before the sort runs, so a kernel that relies on what a fresh allocation holds, or writes outside its
view, shows; the buffer is the same one from test to test, as it is from batch to batch in the product.
Not here: a table of more than 2^24 rows (`wide`, `tmpf`) cannot be small; it stays with
tests/test_gpu_parity.py::test_msm_g1_beyond_the_two_pass_sort_range.
Run with `-m gpu` on an MI355X."""
import random

import pytest

import msm_stage_models as M
from pyref import R

pytestmark = pytest.mark.gpu

# (c, np, pad_log): the placement is two-pass where nb >= 128 && W <= 30 && (nb >> 7) * np >= 8 (k_msm_sort.hip)
SHAPES = [
    (4, 1, 0),    # scatter, lone
    (7, 9, 2),    # scatter, batch
    (8, 9, 2),    # W = 32 > 30: still scatter
    (9, 4, 2),    # the smallest two-pass
    (9, 3, 2),    # one proof fewer: scatter again
    (12, 1, 0),   # two-pass
    (12, 9, 2),   # two-pass
    (16, 2, 2),   # nb = 32768: 32 scan blocks, 128 KiB histogram
]
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 5000]   # 5000: several scalar ranges, the last one partly filled


@pytest.fixture(scope="module")
def shim():
    import msm_stages_shim
    msm_stages_shim.load("g1")
    yield msm_stages_shim
    msm_stages_shim.sort_release()


def two_pass(c, np_):
    W, nb = M.geom(c)
    return nb >= 128 and W <= 30 and (nb >> 7) * np_ >= 8


def test_the_shapes_take_the_placements_they_are_named_for():
    assert [two_pass(c, np_) for c, np_, _ in SHAPES] == [False, False, False, True, False, True, True, True]
    assert (M.geom(9)[1] >> 7) * 4 == 8 and M.geom(8)[0] == 32 and M.geom(16)[1] == 32768


def scalar_vector(c, n, rng):
    """zeros and ones at 0.4 each, the rest from the edge scalars of this window width and random full-width values"""
    edge = [s for s in M.edge_scalars(c, rng, 8) if s > 1]
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(0 if u < 0.4 else 1 if u < 0.8 else rng.choice(edge) if u < 0.95 else rng.randrange(R))
    if n >= 63:   # every edge scalar at least once where there is room
        for k, s in enumerate(rng.sample(edge, min(len(edge), n // 3))):
            out[(3 * k + 1) % n] = s
    return out


def check_sorted(got, scalars, c, pad_log, subset=None, poisoned=True):
    """every property of the sort's result, for every proof (poisoned: the buffers held the poison before, so behind start[nb] only it or the
    scatter path's fill may stand; after an earlier sort without poison in between, what that sort left there is nobody's business)"""
    start, dense, words, stride = got
    n = len(scalars[0])
    W, nb = M.geom(c)
    unit = 1 << pad_log
    for p, vec in enumerate(scalars):
        want = M.entries(vec, n, c, subset)
        lens = [len(r) for r in want]
        where = "proof %d of c=%d n=%d np=%d pad_log=%d" % (p, c, n, len(scalars), pad_log)
        assert dense[p] == M.scan(lens), where                                    # the packed scan, dense[nb] the entry count
        assert start[p] == M.scan([(v + unit - 1) // unit * unit for v in lens]), where   # runs rounded up to 2^pad_log, start[nb] likewise
        w, st = words[p], start[p]
        for b in range(nb):
            run = w[st[b]:st[b] + lens[b]]
            if sorted(run) != want[b]:
                assert sorted(run) == want[b], "%s: bucket %d" % (where, b)
            gap = w[st[b] + lens[b]:st[b + 1]]
            if gap and any(e != M.PAD_ENTRY for e in gap):
                assert gap == [M.PAD_ENTRY] * len(gap), "%s: the gap behind bucket %d" % (where, b)
        assert st[nb] <= stride
        rest = set(w[st[nb]:]) if poisoned else set()
        assert rest <= {M.POISON, M.PAD_ENTRY}, "%s: behind start[nb]: %s" % (where, sorted(rest)[:4])


def vectors(c, np_, n, seed):
    rng = random.Random(seed)
    vecs = [scalar_vector(c, n, rng) for _ in range(np_)]   # different vectors: a proof that lands in another's slice shows
    if n == SIZES[-1] and np_ > 1:
        vecs[-1] = [0] * n   # a proof without any entry
    return vecs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c,np_,pad_log", SHAPES)
def test_sort_against_the_entries_model(shim, c, np_, pad_log, n):
    vecs = vectors(c, np_, n, 1000 * c + 10 * np_ + n)
    check_sorted(shim.sort(vecs, c, pad_log), vecs, c, pad_log)


@pytest.mark.parametrize("c,pad_log", [(4, 0), (12, 0), (7, 2)])
def test_a_lone_proof_without_entries(shim, c, pad_log):
    vecs = [[0] * 65]
    start, dense, words, _ = got = shim.sort(vecs, c, pad_log)
    check_sorted(got, vecs, c, pad_log)
    assert start[0] == [0] * (M.geom(c)[1] + 1) == dense[0]


def subset_vector(n, bits, b_first, b_end, bad, boundaries, rng, c):
    """mostly boolean scalars with every kind of block placed by hand"""
    k = 1 << bits
    edge = [s for s in M.edge_scalars(c, rng, 4) if s > 1]
    out = [0 if u < 0.45 else 1 if u < 0.9 else rng.choice(edge) for u in (rng.random() for _ in range(n))]
    def put(blk, vals):
        out[blk * k:blk * k + k] = vals
    blocks = list(range(b_first, b_end))
    put(blocks[1], [0] * k)                                     # pattern 0: no entry
    put(blocks[2], [1] * k)                                     # every base of the block
    put(blocks[3], [1] * (k - 1) + [edge[0]])                   # one scalar that is not boolean: row by row
    put(blocks[4], [edge[1]] + [1, 0] * (k // 2 - 1) + [1])
    put(b_first + sorted(bad)[0], [1, 0] * (k // 2))            # a bad block of booleans: row by row
    put(b_first - 1, [1] * k)                                   # the block in front of the covered range
    put(b_end, [1] * k)                                         # ... and the one behind it (b_end * k + k <= n)
    for edge_i in boundaries:                                   # all-boolean blocks in the last 64 scalars before a range boundary
        put(edge_i // k - 1, [1] + [0] * (k - 2) + [1])
        put(edge_i // k - 3, [0] * (k - 1) + [1])
    return out


@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("c,np_,pad_log", [(4, 1, 0), (7, 3, 2), (12, 3, 2), (12, 1, 0)])
def test_sort_with_subset_rows(shim, c, np_, pad_log, bits):
    n = 2200
    k = 1 << bits
    ng = shim.ranges_for(n, np_)
    assert ng == 3
    per = ((n + ng - 1) // ng + 63) & ~63                       # msm_range_len
    boundaries = [per, 2 * per]
    assert 2 * per < n
    b_first, b_end = 3, (n - 70) >> bits                        # covered: from a block above 0 to below n
    bad = {5, 17, (b_end - b_first) - 1, 40}
    rng = random.Random(77 * c + bits + np_)
    vecs = [subset_vector(n, bits, b_first, b_end, bad, boundaries, rng, c) for _ in range(np_)]
    subset = (bits, b_first, b_end, bad)
    W, _ = M.geom(c)
    model = M.entries(vecs[0], n, c, subset)
    assert any(e >= W * n for e in model[0]) and any(e < n for e in model[0])   # subset rows and plain unit rows side by side
    check_sorted(shim.sort(vecs, c, pad_log, subset), vecs, c, pad_log, subset)
    # without the subset rows the same scalars sort row by row
    check_sorted(shim.sort(vecs, c, pad_log), vecs, c, pad_log)


def test_a_second_sort_into_the_same_buffers_without_poison(shim):
    """a large shape, then smaller ones with another c, n and np into what it left (MsmSortBuf keeps its allocation: msm_host.h)"""
    big = vectors(12, 9, 1025, 1)
    check_sorted(shim.sort(big, 12, 2), big, 12, 2)
    for c, np_, n, pad_log in [(9, 4, 65, 2), (7, 3, 64, 2), (9, 3, 1023, 0), (12, 1, 63, 0), (4, 2, 1024, 1)]:
        vecs = vectors(c, np_, n, 2 + c)
        check_sorted(shim.sort(vecs, c, pad_log, poison=False), vecs, c, pad_log, poisoned=False)
