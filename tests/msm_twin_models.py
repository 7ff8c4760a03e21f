"""Plain-integer model of doubled window rows (masp_amd/csrc/device/msm_geom.h: msm_geom_twin): next to every window row 2^(c j) P the table
holds 2 * 2^(c j) P, a digit magnitude v = 2^t o (o odd) is (row multiple 2^(t & 1), bucket value v >> (t & 1)), and only the values of even
valuation — B = {4^s o <= 2^(c-1)} — have a bucket.  Written from that definition alone: nothing here shares code with the header or the
kernels.  Builds on tests/msm_stage_models.py for digits, points and layouts."""
import msm_stage_models as M
from pyref import ec_add, ec_mul


def recode(v):
    """digit magnitude -> (row multiple, bucket value)"""
    t = (v & -v).bit_length() - 1
    return 1 << (t & 1), v >> (t & 1)


def values(c):
    """the bucket values by id: class after class (s = 0, 1, ...), inside a class by growing odd part"""
    H = 1 << (c - 1)
    out, s = [], 0
    while 4 ** s <= H:
        out += [4 ** s * o for o in range(1, H // 4 ** s + 1, 2)]
        s += 1
    return out


def classes(c):
    """[(first bucket id, buckets, 4^s)]"""
    H = 1 << (c - 1)
    out, off, s = [], 0, 0
    while 4 ** s <= H:
        size = len(range(1, H // 4 ** s + 1, 2))
        out.append((off, size, 4 ** s))
        off += size
        s += 1
    return out


_ids = {}


def bucket_id(c, value):
    if c not in _ids:
        _ids[c] = {v: k for k, v in enumerate(values(c))}
    return _ids[c][value]


def geom(c):
    """(windows, buckets the kernels index: |B|, in whole sorting bins of 128 from 128 on)"""
    W, _ = M.geom(c)
    nbk = len(values(c))
    return W, nbk if nbk < 128 else (nbk + 127) // 128 * 128


def entries(scalars, n, c, subset=None):
    """as msm_stage_models.entries over the doubled tables: row (j or W + j) * n + i, subset rows from 2 W n on"""
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
                out[0].append(2 * W * n + (blk - b_first) * per + pattern - 1)
            for t in range(k):
                done[blk * k + t] = True
    for i, s in enumerate(scalars):
        if done[i] or s == 0:
            continue
        if s == 1:
            out[0].append(i)
            continue
        for j, b, neg in M.digits(s, c):
            mult, value = recode(b + 1)
            out[bucket_id(c, value)].append(((j + (W if mult == 2 else 0)) * n + i) | (neg << 31))
    return [sorted(v) for v in out]


def table(F, bases, c):
    """the window rows, then their doubles: row (W + j) n + i = 2 * row j n + i"""
    rows = M.table(F, bases, c)
    return rows + [M.from_ref(F, ec_add(F, M.to_ref(F, p), M.to_ref(F, p))) for p in rows]


def weighted_sum(F, c, bucket_sums):
    """sum over the bucket ids of value * B"""
    acc = None
    for v, B in zip(values(c), bucket_sums):
        acc = ec_add(F, acc, ec_mul(F, M.to_ref(F, B), v))
    return M.from_ref(F, acc)
