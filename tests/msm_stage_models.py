"""Plain-integer models of what the MSM's stages leave between them (masp_amd/csrc/device/msm_sort.hpp, msm_tree.hpp, msm.hpp): the signed
window digits and the entry words of the counting sort, one level of the batch-affine bucket tree, the weighted sum of the bucket tails.
Field and curve arithmetic are pyref's; nothing here shares code with the kernels.  tests/test_msm_stage_models.py checks the models on
the CPU against things they do not share code with either (the scalar itself, ec_add, ec_mul); the GPU stage tests compare the kernels
with them, exactly.

A point is an affine pair, the point at infinity the pair of zeros — (0, 0) on G1, ((0, 0), (0, 0)) on G2 — as in the kernels."""
from pyref import F1, F2, R, ec_add

PAD_ENTRY = 0xFFFFFFFF      # MSM_PAD_ENTRY: the word behind a run that is aligned to 2^pad_log entries
POISON = 0xA5A5A5A5         # what the stage harness fills every buffer with before a stage runs


def geom(c):
    """(windows of a 256-bit scalar, buckets) of c-bit signed digits"""
    return (256 + c - 1) // c, 1 << (c - 1)


def digits_carry(s, c):
    """the signed window digits of s as MsmDigitIter takes them: [(window, bucket, negative)], and the carry out of the top window"""
    W, _ = geom(c)
    mask, half, carry, out = (1 << c) - 1, 1 << (c - 1), 0, []
    for j in range(W):
        v = ((s >> (c * j)) & mask) + carry
        carry = 0
        neg = 0
        if v > half:
            v = (1 << c) - v
            neg = carry = 1
        if v:
            out.append((j, v - 1, neg))
    return out, carry


def digits(s, c):
    return digits_carry(s, c)[0]


def entries(scalars, n, c, subset=None):
    """per bucket, the sorted list of the entry words (window * n + i) | sign << 31 of one proof's scalars.
    subset: None, or (bits, b_first, b_end, bad) — the subset rows of a base set (MsmSubset): blocks [b_first, b_end) of 2^bits scalars, `bad` the
    set of blocks (relative to b_first) that are treated as not covered."""
    assert len(scalars) == n
    W, nb = geom(c)
    out = [[] for _ in range(nb)]
    done = [False] * n
    if subset is not None:
        bits, b_first, b_end, bad = subset
        k = 1 << bits
        per = (1 << k) - 1
        for blk in range(b_first, b_end):
            if blk - b_first in bad:
                continue
            block = scalars[blk * k:blk * k + k]
            if len(block) != k or any(s > 1 for s in block):
                continue
            pattern = sum(s << t for t, s in enumerate(block))
            if pattern:
                out[0].append(W * n + (blk - b_first) * per + pattern - 1)
            for t in range(k):
                done[blk * k + t] = True
    for i, s in enumerate(scalars):
        if done[i] or s == 0:
            continue
        if s == 1:
            out[0].append(i)
            continue
        for j, b, neg in digits(s, c):
            out[b].append((j * n + i) | (neg << 31))
    return [sorted(v) for v in out]


# ---- points ----
def inf(F):
    return (F.zero, F.zero)


def is_inf(F, p):
    return p[0] == F.zero and p[1] == F.zero


def neg(F, p):
    return (p[0], F.neg(p[1]))


def affine_add(F, p, q):
    """the complete affine law on y^2 = x^3 + b: doubling, P - P -> infinity, infinity as either operand"""
    if is_inf(F, q):
        return p
    if is_inf(F, p):
        return q
    if p[0] != q[0]:
        lam = F.mul(F.sub(q[1], p[1]), F.inv(F.sub(q[0], p[0])))
    elif p[1] == q[1] and p[1] != F.zero:
        xx = F.mul(p[0], p[0])
        lam = F.mul(F.add(F.add(xx, xx), xx), F.inv(F.add(p[1], p[1])))
    else:
        return inf(F)
    x3 = F.sub(F.sub(F.mul(lam, lam), p[0]), q[0])
    return (x3, F.sub(F.mul(lam, F.sub(p[0], x3)), p[1]))


def tree_level(F, points):
    """a bucket's points -> the next level's: new[j] = old[2j] + old[2j + 1], an odd last point passes through"""
    out = [affine_add(F, points[2 * j], points[2 * j + 1]) for j in range(len(points) // 2)]
    if len(points) & 1:
        out.append(points[-1])
    return out


def to_ref(F, p):
    """-> pyref's convention (None = infinity)"""
    return None if is_inf(F, p) else p


def from_ref(F, p):
    return inf(F) if p is None else p


def bucket_sum(F, points):
    acc = None
    for p in points:
        acc = ec_add(F, acc, to_ref(F, p))
    return from_ref(F, acc)


def weighted_sum(F, bucket_sums):
    """sum over b of (b + 1) B_b, by the running sum from the top bucket down"""
    run = acc = None
    for B in reversed(bucket_sums):
        run = ec_add(F, run, to_ref(F, B))
        acc = ec_add(F, acc, run)
    return from_ref(F, acc)


# ---- window tables ----
_tables = {}


def table(F, bases, c):
    """row j * n + i = 2^(c j) P_i by repeated doubling (bases: tuple of points, infinity as zeros)"""
    key = (F, tuple(bases), c)
    if key not in _tables:
        W, _ = geom(c)
        rows, cur = [], [to_ref(F, p) for p in bases]
        for j in range(W):
            rows += [from_ref(F, p) for p in cur]
            if j + 1 < W:
                for _ in range(c):
                    cur = [ec_add(F, p, p) for p in cur]
        _tables[key] = rows
    return _tables[key]


def entry_point(F, rows, e):
    """the point an entry word names: the padding entry is infinity, bit 31 negates"""
    if e == PAD_ENTRY:
        return inf(F)
    p = rows[e & 0x7FFFFFFF]
    return neg(F, p) if e >> 31 and not is_inf(F, p) else p


def layout(runs, pad_log, stride=None):
    """bucket runs (lists of entry words) -> (start[nb + 1], the proof's slice of `sorted`): every run begins at a multiple of 2^pad_log,
    MSM_PAD_ENTRY behind it, the poison behind start[nb] up to `stride`"""
    unit = 1 << pad_log
    start, words = [], []
    for r in runs:
        start.append(len(words))
        words += list(r)
        words += [PAD_ENTRY] * (-len(r) % unit)
    start.append(len(words))
    if stride is not None:
        assert len(words) <= stride, (len(words), stride)
        words += [POISON] * (stride - len(words))
    return start, words


def scan(vals):
    out, acc = [], 0
    for v in vals:
        out.append(acc)
        acc += v
    return out + [acc]


# ---- scalars ----
def edge_scalars(c, rng, n_random=6):
    """the scalars a sort test mixes: small ones, r - 1, r - 2, powers of two around every window boundary, windows that sit exactly on the
    sign threshold, carries that ripple to the top, random full-width values"""
    W, _ = geom(c)
    out = [0, 1, 2, R - 1, R - 2]
    for j in range(1, W):
        for k in (c * j - 1, c * j, c * j + 1):
            if k < 255:
                out += [(1 << k) - 1, 1 << k]
    half = 1 << (c - 1)
    out.append(sum(half << (c * j) for j in range(W)) % (1 << 254))          # every window 2^(c-1): stays positive
    out.append(sum((half + 1) << (c * j) for j in range(W)) % (1 << 254))    # every window 2^(c-1) + 1: negative, a carry through every window
    out.append((1 << 254) - 1)                                                # all-ones windows: the carry ripples to the top
    out.append(((1 << 254) - 1) ^ ((1 << c) - 1) | 3)
    out += [rng.randrange(R) for _ in range(n_random)]
    return [s for s in out if s < R]
