"""The MSM's counting sort at the window widths tests/test_gpu_msm_sort_stages.py and tests/test_gpu_msm_twin_rows.py leave out — 5, 6, 10, 11,
13, 14, 15 plain, 13 and 16 over doubled rows: the widths production runs (16 and 13 doubled, 15 for Output's h) among them.  The digit
iterator (MsmDigitIter) shifts the scalar's words by c per window, so every width is a path of its own through the same code.  Sizes 513 and
1537 cross the boundaries of a 512-scalar tile of k_msm_partition, 1025 those of a 1024-scalar one.  The checks are the existing files':
`check_sorted` against tests/msm_stage_models.py, `TM.entries` / `M.layout` for the doubled rows.  Run with `-m gpu` on an MI355X."""
import random

import pytest

import msm_stage_models as M
import msm_twin_models as TM
from test_gpu_msm_sort_stages import check_sorted, scalar_vector, two_pass
from test_gpu_msm_twin_rows import N_SORT, NP_SORT, SUBSET, sort_scalars

pytestmark = pytest.mark.gpu

# (c, np, pad_log, two-pass placement)
SHAPES = [
    (5, 3, 2, False),
    (6, 1, 0, False),
    (10, 1, 0, False),
    (10, 2, 2, True),
    (11, 1, 0, True),
    (13, 3, 2, True),
    (14, 1, 0, True),
    (15, 2, 2, True),
]
SIZES = [1, 64, 65, 513, 1025, 1537]


@pytest.fixture(scope="module")
def shim():
    import msm_stages_shim
    msm_stages_shim.load("g1")
    yield msm_stages_shim
    msm_stages_shim.sort_release()


@pytest.fixture(scope="module")
def twin_shim():
    import msm_twin_shim
    return msm_twin_shim


def test_the_shapes_take_the_placements_they_are_named_for():
    assert [two_pass(c, np_) for c, np_, _, _ in SHAPES] == [tp for _, _, _, tp in SHAPES]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c,np_,pad_log,tp", SHAPES)
def test_sort_against_the_entries_model(shim, c, np_, pad_log, tp, n):
    assert two_pass(c, np_) == tp
    rng = random.Random(7000 * c + 10 * np_ + n)
    vecs = [scalar_vector(c, n, rng) for _ in range(np_)]
    check_sorted(shim.sort(vecs, c, pad_log), vecs, c, pad_log)


@pytest.mark.parametrize("subset", [None, SUBSET], ids=["plain", "subset"])
@pytest.mark.parametrize("c", [13, 16])
def test_doubled_rows_sort_against_the_model(twin_shim, c, subset):
    """the scalars and the subset of tests/test_gpu_msm_twin_rows.py at the widths the batch path runs: both take the two-pass placement"""
    scalars = [sort_scalars(c, p) for p in range(NP_SORT)]
    W, nb = TM.geom(c)
    assert nb >= 128 and W <= 30 and (nb >> 7) * NP_SORT >= 8
    pad_log = 2
    start, dense, words, stride = twin_shim.sort(scalars, c, pad_log, subset)
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
