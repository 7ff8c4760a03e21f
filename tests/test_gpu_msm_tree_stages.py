"""The batch-affine bucket tree level by level (msm_tree_enqueue: k_tree_plan, k_tree_records, k_tree_pass1, k_binv_*, k_tree_pass2,
k_tree_copy), through tests/native/msm_stages_dev.hip, over digit lists made by hand: for T = 1, 2, 3, 4 and 6 levels the plan (D, Q), the
offsets the tails go by and every point of level T are read back and compared, bucket by bucket and index by index, with tree_level of
tests/msm_stage_models.py applied T times — affine coordinates, exactly.  Then k_msm_accumulate_pts over level T and the bucket tails must
give the MSM's point.  Runs aligned to four entries (levels 0 and 1 without records) and to two (records and k_tree_copy from level 1 on).
Inside a run the order of the entries is the test's: every exceptional pair of the affine law is placed as the first, a middle and the
last pair of a lane's software pipeline (pair q of a level belongs to lane q mod NT, at position q div NT), in lanes whose other pairs are
ordinary.  The arena and the workspace hold the byte 0xA5 before every call.
Run with `-m gpu` on an MI355X."""
import random

import pytest

import msm_stage_models as M
from pyref import F1, F2, G1, G2, P, R, ec_mul

pytestmark = pytest.mark.gpu

LEVELS = [1, 2, 3, 4, 6]
LENGTHS = list(range(1, 18)) + [31, 32, 33]


@pytest.fixture(scope="module")
def shim():
    import msm_stages_shim
    yield msm_stages_shim
    for curve in ("g1", "g2"):
        getattr(msm_stages_shim.load(curve), "mst_%s_release" % curve)()


# ---- bases ----
def fp_sqrt(a):
    s = pow(a % P, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def fp2_sqrt(a):
    a0, a1 = a
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a0)
        return None if s is None else (0, s)
    n = fp_sqrt(a0 * a0 + a1 * a1)
    if n is None:
        return None
    for nn in (n, P - n):
        x0 = fp_sqrt((a0 + nn) * pow(2, -1, P))
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, P) % P)
            if F2.mul(x, x) == (a0 % P, a1 % P):
                return x
    return None


def twist_point(make_x):
    """the first point of y^2 = x^3 + 4 (1 + u) with x = make_x(k), k = 1, 2, ...: one half of x is zero"""
    for k in range(1, 200):
        x = make_x(k)
        y = fp2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), (4, 4)))
        if y is not None:
            assert F2.mul(y, y) == F2.add(F2.mul(F2.mul(x, x), x), (4, 4))
            return (x, y)
    raise AssertionError("no such point")


class Setup:
    """a base set and its window table in the model: bases 0 and 1 at infinity, 2 and 3 with x = 0 (G1: (0, 2) of order three and its
    negative, tests/test_gpu_bucket_tree.py::_x_zero_case) or one half of x zero (G2: points of the twist, accepted by the loader, which checks
    flags and canonical encoding only), the others ordinary"""

    def __init__(self, curve, n, c):
        self.curve, self.n, self.c = curve, n, c
        self.F, gen = (F1, G1) if curve == "g1" else (F2, G2)
        rng = random.Random(n * c)
        special = [(0, 2), (0, P - 2)] if curve == "g1" else [twist_point(lambda k: (0, k)), twist_point(lambda k: (k, 0))]
        self.bases = tuple([M.inf(self.F)] * 2 + special + [ec_mul(self.F, gen, rng.randrange(1, R)) for _ in range(n - 4)])
        self.W, self.nb = M.geom(c)
        self.rows = M.table(self.F, self.bases, c)

    def ordinary(self, rng):
        return (rng.randrange(self.W) * self.n + rng.randrange(4, self.n)) | (rng.randrange(2) << 31)

    def row(self, base, rng):
        return rng.randrange(self.W) * self.n + base


_setups = {}


def setup_of(curve, n, c):
    if (curve, n, c) not in _setups:
        _setups[(curve, n, c)] = Setup(curve, n, c)
    return _setups[(curve, n, c)]


# ---- digit lists ----
NEG = 1 << 31


def exceptional_pairs(S, rng):
    """name -> the two entry words of a pair that leaves the common path of the two passes"""
    o, r = S.ordinary(rng), S.ordinary(rng)
    i0, i1, z0, z1 = S.row(0, rng), S.row(1, rng), S.row(2, rng), S.row(3, rng)
    kinds = {
        "P + P": (o, o),
        "P - P": (r, r ^ NEG),
        "infinity first": (i0, S.ordinary(rng)),
        "infinity second": (S.ordinary(rng), i1 | NEG),
        "two infinities": (i0, i1),
        "zero-x first": (z0, S.ordinary(rng)),
        "zero-x second": (S.ordinary(rng), z1 | NEG),
        "zero-x doubled": (z0, z0),
        "zero-x cancelled": (z0 | NEG, z0),
        "zero-x both": (z0, z1),
    }
    return kinds


def fill_runs(S, rng, first_bucket, lengths, entries_left, pad_log):
    """runs of the given lengths from first_bucket on while they fit, the last bucket taking what is left of `entries_left` (padded entries)"""
    unit = 1 << pad_log
    runs = {}
    b = first_bucket
    for length in lengths:
        padded = -(-length // unit) * unit
        if b >= S.nb - 1 or padded > entries_left:
            break
        runs[b] = [S.ordinary(rng) for _ in range(length)]
        entries_left -= padded
        b += 1
    if entries_left:
        runs[b] = [S.ordinary(rng) for _ in range(entries_left)]
    return runs


def whole_pairs(pairs, pad_log):
    """a proof's padded entries are a multiple of 2^pad_log: three pairs become four where runs are aligned to four entries"""
    half = max(1, (1 << pad_log) // 2)
    return -(-pairs // half) * half


def small_proof(S, rng, pairs, lengths, pad_log):
    pairs = whole_pairs(pairs, pad_log)
    runs = fill_runs(S, rng, 0, lengths, 2 * pairs, pad_log)
    return [runs.get(b, []) for b in range(S.nb)]


def big_proof(S, rng, pairs, NT, lengths, pad_log):
    """the proof whose lanes have the most pairs: three runs that end exactly where a pair (entry, padding) — and behind it, with runs aligned
    to four, a pair of two padding entries — is the first, a middle and the last pair of a lane; one of them holds half the proof.  Then every
    exceptional pair, written over ordinary entries at the same three positions of other lanes, and three patterns of four and eight entries
    that reach the deeper levels.  -> runs, {name: [(q, j)]} of what was placed"""
    unit = 1 << pad_log
    jlast = (pairs - 1) // NT
    js = sorted({0, jlast // 2, jlast})
    assert 6 + jlast * NT < pairs
    runs, pos = {}, 0
    for b, j in enumerate(js):
        q_end = 2 + 2 * b + j * NT                       # its last entry is the first of pair q_end; the second is padding
        runs[b] = [S.ordinary(rng) for _ in range(2 * q_end + 1 - pos)]
        pos = -(-(2 * q_end + 1) // unit) * unit
    runs.update(fill_runs(S, rng, len(js), lengths, 2 * pairs - pos, pad_log))
    runs = [runs.get(b, []) for b in range(S.nb)]
    start, words = M.layout(runs, pad_log)
    assert len(words) == 2 * pairs
    real = [e != M.PAD_ENTRY for e in words]
    placed, used = {}, set()

    def write(q, pair):
        words[2 * q], words[2 * q + 1] = pair

    lane = {j: 9 for j in js}
    for name, pair in exceptional_pairs(S, rng).items():
        for j in js:
            while True:
                t = lane[j]
                lane[j] += 1
                q = t + j * NT
                assert q < pairs, (name, j)
                if t not in used and real[2 * q] and real[2 * q + 1]:
                    break
            used.add(t)
            write(q, pair)
            placed.setdefault(name, []).append((q, j))
    # patterns relative to the start of the long run (bucket 1 where there is a middle position, else bucket 0 ... the longest)
    longest = max(range(S.nb), key=lambda b: len(runs[b]))
    base = start[longest] + 8 * 40
    assert base + 24 <= start[longest] + len(runs[longest]) and all((base // 2 + k) % NT not in used for k in range(12))
    a, b_, c_, d_ = (S.ordinary(rng) for _ in range(4))
    r, s = S.ordinary(rng), S.ordinary(rng)
    words[base:base + 8] = [r, r ^ NEG, a, b_, c_, d_, s, S.ordinary(rng)]             # level 1 meets (infinity, a + b)
    words[base + 8:base + 16] = [r, r ^ NEG, s, s ^ NEG, a, b_, c_, d_]                # level 2 meets (infinity, a + b + c + d)
    words[base + 16:base + 24] = [a, b_, c_, d_, a, b_, c_, d_]                        # level 2 meets two equal sums: a doubling
    # back to runs
    out = [words[start[b]:start[b] + len(runs[b])] for b in range(S.nb)]
    pads = {"entry + padding": [], "padding + padding": []}
    for q in range(pairs):
        if real[2 * q] and not real[2 * q + 1]:
            pads["entry + padding"].append((q, q // NT))
        if not real[2 * q] and not real[2 * q + 1]:
            pads["padding + padding"].append((q, q // NT))
    placed.update(pads)
    return out, placed, js


def model_levels(S, runs, pad_log, top):
    """[level][bucket] -> the points of a proof's bucket at every level 0 .. top (level 0: the padded run)"""
    unit = 1 << pad_log
    cur = [[M.entry_point(S.F, S.rows, e) for e in list(run) + [M.PAD_ENTRY] * (-len(run) % unit)] for run in runs]
    levels = [cur]
    for _ in range(top):
        cur = [M.tree_level(S.F, pts) for pts in cur]
        levels.append(cur)
    return levels


def msm_point(S, runs):
    return M.weighted_sum(S.F, [M.bucket_sum(S.F, [M.entry_point(S.F, S.rows, e) for e in run]) for run in runs])


CONFIGS = {
    # name: (curve, bases, window bits, pairs of the proofs at level 0; the first is one more where runs are aligned to four entries) — 48 bases
    # on 8-bit windows give the tree's views 1664 entries per proof with runs aligned to two, 832 pairs: the largest proof has 820 there (lanes
    # of 3 and 4 pairs); 16 G2 bases on 4-bit windows 524 pairs, and the G2 lists stay under 400 pairs
    "g1-c4": ("g1", 48, 4, [3, 300, 700, 1100, 0]),
    "g1-c8": ("g1", 48, 8, [3, 300, 700, 820, 0]),
    "g2-c4": ("g2", 16, 4, [3, 100, 200, 390, 0]),
}
_cases = {}


def case_of(shim, name, pad_log):
    """the five digit lists of a configuration and their model, made once and shared by the tests of every T"""
    if (name, pad_log) not in _cases:
        curve, n, c, pairs = CONFIGS[name]
        S = setup_of(curve, n, c)
        rng = random.Random(len(name) * 100 + c * 10 + pad_log)
        NT = shim.tree_lanes(curve, n, c, pad_log, 0)
        assert NT == 256
        pool = LENGTHS[:]
        proofs, placed, js = [], None, None
        for p, count in enumerate(pairs):
            lengths = pool[5 * p:] + pool[:5 * p]            # every proof begins somewhere else in the list of lengths
            if count == max(pairs):
                runs, placed, js = big_proof(S, rng, count, NT, [31, 32, 33, 17] + lengths, pad_log)
            else:
                runs = small_proof(S, rng, count, lengths, pad_log)
            proofs.append(runs)
        stride = shim.padded_entries(n, c, pad_log)
        assert max(pairs) * 2 <= shim.tree_entries(curve, n, c, pad_log) <= stride
        laid = [M.layout(runs, pad_log, stride) for runs in proofs]
        levels = [model_levels(S, runs, pad_log, max(LEVELS)) for runs in proofs]
        _cases[(name, pad_log)] = (S, proofs, laid, levels, placed, js, NT)
    return _cases[(name, pad_log)]


@pytest.mark.parametrize("pad_log", [2, 1])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_digit_lists_hold_what_they_are_made_for(shim, name, pad_log):
    S, proofs, laid, levels, placed, js, NT = case_of(shim, name, pad_log)
    pairs = [len([e for e in w if e != M.POISON]) // 2 for _, w in laid]
    assert pairs == [whole_pairs(v, pad_log) for v in CONFIGS[name][3]]
    per_lane = set()
    for count in pairs:                                      # pairs of lane t: those q < count with q = t mod NT
        per_lane |= {(count - t + NT - 1) // NT for t in range(NT) if count > t} | ({0} if count < NT else set())
    assert per_lane == set(range(0, (max(pairs) - 1) // NT + 2)), per_lane    # g1-c4: lanes of 0, 1, 2, 3, 4 and 5 pairs in one launch
    if name == "g1-c4":
        assert per_lane == {0, 1, 2, 3, 4, 5}
    want = set(exceptional_pairs(S, random.Random(0))) | {"entry + padding"} | ({"padding + padding"} if pad_log == 2 else set())
    assert set(placed) >= want
    for kind in want:
        assert {j for _, j in placed[kind]} >= set(js), (kind, placed[kind][:8])   # first, middle and last pair of a lane
    # what reaches the deeper levels: infinity as the first operand of a pair at level 1 and at level 2, two equal sums at level 2
    big = levels[pairs.index(max(pairs))]
    pairs_of = lambda L: [(pts[2 * j], pts[2 * j + 1]) for pts in big[L] for j in range(len(pts) // 2)]
    for L in (1, 2):
        assert any(M.is_inf(S.F, a) and not M.is_inf(S.F, b) for a, b in pairs_of(L)), L
    assert any(a == b and not M.is_inf(S.F, a) for a, b in pairs_of(2))
    lengths = {len(run) for runs in proofs for run in runs}
    if S.nb >= 128:
        assert lengths >= set(LENGTHS)
    assert lengths & set(LENGTHS) and max(len(run) for run in proofs[pairs.index(max(pairs))]) * 2 >= max(pairs) * 2 * 0.45   # ~half the proof in one bucket


@pytest.mark.parametrize("T", LEVELS)
@pytest.mark.parametrize("pad_log", [2, 1])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_point_of_level_T(shim, name, pad_log, T):
    S, proofs, laid, levels, placed, js, NT = case_of(shim, name, pad_log)
    out = shim.tree(S.curve, S.bases, S.c, [w for _, w in laid], [s for s, _ in laid], pad_log, T)
    nb = S.nb
    for p, runs in enumerate(proofs):
        start = laid[p][0]
        for L in range(T + 1):
            lens = [(start[b + 1] - start[b] + (1 << L) - 1) >> L for b in range(nb)]
            assert [len(pts) for pts in levels[p][L]] == lens
            assert out.D[L][p] == M.scan(lens), "D of level %d, proof %d" % (L, p)
            assert out.Q[L][p] == M.scan([v >> 1 for v in lens]), "Q of level %d, proof %d" % (L, p)
        DT = out.D[T][p]
        assert out.keep[p] == DT and out.over_start[p] == [0] * (nb + 1), p
        for b in range(nb):
            got = out.points[p][DT[b]:DT[b + 1]]
            want = levels[p][T][b]
            if got != want:
                bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
                assert got == want, "level %d, proof %d, bucket %d (run of %d): points %s differ" % (T, p, b, len(runs[b]), bad[:8])
        assert out.result[p] == msm_point(S, runs), "proof %d" % p
    # pairs of lane t at level 0, from the kernel's own Q and the launch's NT: those q < Q[nb] with q = t mod NT
    counts = [out.Q[0][p][nb] for p in range(len(proofs))]
    per_lane = {(count - t + NT - 1) // NT if count > t else 0 for count in counts for t in range(NT)}
    assert per_lane == set(range((max(counts) - 1) // NT + 2)) and (name != "g1-c4" or per_lane == {0, 1, 2, 3, 4, 5})
    assert out.over_count[0] == out.over_count[1]
    assert out.Q[0][proofs.index(max(proofs, key=lambda r: sum(map(len, r))))][nb] == max(CONFIGS[name][3])


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("pad_log", [2, 1])
def test_a_proof_over_the_entry_bound(shim, pad_log, T):
    """MsmBases::ent_bound cuts the tree's views below the sort's stride; a proof with more entries gets no points and no pairs on any level, its
    offsets go to over_start and to the tails' offsets, the counter rises by one — and the other four proofs' levels are what they are without it"""
    curve, n, c = "g1", 48, 4
    S = setup_of(curve, n, c)
    rng = random.Random(5 + pad_log)
    bound = 400
    E = shim.tree_entries(curve, n, c, pad_log, bound)
    stride = shim.padded_entries(n, c, pad_log)
    assert E < stride and shim.tree_lanes(curve, n, c, pad_log, 0, bound) == 256
    pairs = [3, 100, 750, E // 2, 0]                             # the third is over the bound; the fourth fills the views exactly
    over = 2
    proofs = [small_proof(S, rng, count, LENGTHS[3 * p:] + LENGTHS[:3 * p], pad_log) for p, count in enumerate(pairs)]
    laid = [M.layout(runs, pad_log, stride) for runs in proofs]
    assert [s[S.nb] > E for s, _ in laid] == [False, False, True, False, False]
    out = shim.tree(curve, S.bases, c, [w for _, w in laid], [s for s, _ in laid], pad_log, T, ent_bound=bound)
    nb = S.nb
    assert out.over_count[1] == out.over_count[0] + 1
    for p, runs in enumerate(proofs):
        start = laid[p][0]
        if p == over:
            assert all(out.D[L][p] == [0] * (nb + 1) == out.Q[L][p] for L in range(T + 1))
            assert out.over_start[p] == start and out.keep[p] == start
        else:
            levels = model_levels(S, runs, pad_log, T)
            for L in range(T + 1):
                lens = [len(pts) for pts in levels[L]]
                assert out.D[L][p] == M.scan(lens) and out.Q[L][p] == M.scan([v >> 1 for v in lens]), (L, p)
            DT = out.D[T][p]
            assert out.keep[p] == DT and out.over_start[p] == [0] * (nb + 1)
            for b in range(nb):
                assert out.points[p][DT[b]:DT[b + 1]] == levels[T][b], "proof %d, bucket %d" % (p, b)
        assert out.result[p] == msm_point(S, runs), "proof %d" % p
