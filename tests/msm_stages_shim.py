"""Loader of the test-only unit tests/native/msm_stages_dev.hip (the MSM's stages, each through the product's own driver: the
counting sort, the batch-affine bucket tree, the accumulation and the bucket tails), with the product's flags as native_build.py reads them
from the Makefile.  The unit is compiled once per curve, side by side —
_msm_stages_dev_g1.so (the sort and G1) and _msm_stages_dev_g2.so (-DMST_G2) —: as one library it compiles for as long as the two after each
other.  Measured: G1 81 s, G2 56 s, side by side 81 s (the two after each other 137 s).
Everything that goes in or comes out is plain: scalars as Python ints, entry words and offsets as lists of ints, points as affine pairs of
ints with the pair of zeros for the point at infinity (tests/msm_stage_models.py), on the wire as bellman uncompressed bytes."""
import ctypes as C

import numpy as np

import msm_stage_models as M
import native_build
from pyref import F1, F2, g1_unc, g2_unc

UNITS = {"g1": native_build.unit("msm_stages_dev", "_g1"), "g2": native_build.unit("msm_stages_dev", "_g2", ["-DMST_G2"])}
_libs = {}


def load(curve):
    if not _libs:
        _libs.update(zip(UNITS, native_build.load_all(UNITS.values())))
        _libs["g1"].mst_padded_entries.restype = C.c_uint64
        for name, lib in _libs.items():
            getattr(lib, "mst_%s_tree_entries" % name).restype = C.c_uint64
    return _libs[curve]


CURVES = {"g1": (F1, g1_unc, 96), "g2": (F2, g2_unc, 192)}
_U32 = C.c_uint32
_U64 = C.c_uint64


def _u32s(vals):
    return (_U32 * len(vals))(*vals)


def _wire(curve, pts):
    F, unc, _ = CURVES[curve]
    return b"".join(unc(M.to_ref(F, p)) for p in pts)


def _points(curve, raw):
    """wire bytes -> affine pairs, the identity as the pair of zeros"""
    F, _, w = CURVES[curve]
    out = []
    for i in range(len(raw) // w):
        b = raw[w * i:w * i + w]
        if b[0] & 0x40:
            assert not any(b[1:]) and b[0] == 0x40
            out.append(M.inf(F))
        elif curve == "g1":
            out.append((int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")))
        else:
            v = [int.from_bytes(b[48 * k:48 * k + 48], "big") for k in range(4)]
            out.append(((v[1], v[0]), (v[3], v[2])))
    return out


def padded_entries(n, c, pad_log):
    """MsmSortBuf::padded_entries: the words per proof of `sorted`"""
    return int(load("g1").mst_padded_entries(n, c, pad_log))


def ranges_for(n, np_):
    return int(load("g1").mst_ranges_for(n, np_))


def tree_entries(curve, n, c, pad_log, ent_bound=0):
    """MsmBases::tree_entries: the entries per proof the tree's views hold"""
    return int(getattr(load(curve), "mst_%s_tree_entries" % curve)(n, c, pad_log, _U64(ent_bound)))


def tree_lanes(curve, n, c, pad_log, level, ent_bound=0):
    """lanes per proof (NT) of the tree's two passes at `level`"""
    return int(getattr(load(curve), "mst_%s_tree_lanes" % curve)(n, c, pad_log, _U64(ent_bound), level))


def sort(scalars, c, pad_log, subset=None, poison=True):
    """scalars: np lists of n ints; subset: None or (bits, b_first, b_end, bad set) -> (start, dense, sorted, ent_stride): per proof lists of ints"""
    np_, n = len(scalars), len(scalars[0])
    assert all(len(v) == n for v in scalars)
    _, nb = M.geom(c)
    stride = padded_entries(n, c, pad_log)
    raw = b"".join([int(s).to_bytes(32, "little") for v in scalars for s in v])
    start, dense, out = (_U32 * (np_ * (nb + 1)))(), (_U32 * (np_ * (nb + 1)))(), (_U32 * (np_ * stride))()
    bits, b_first, b_end, bad = subset if subset is not None else (0, 0, 0, set())
    words = [0] * max(1, (b_end - b_first + 31) // 32)
    for rb in bad:
        words[rb >> 5] |= 1 << (rb & 31)
    rc = load("g1").mst_sort(raw, n, c, np_, pad_log, bits, b_first, b_end, _u32s(words), 1 if poison else 0, start, dense, out)
    assert rc == 0, rc
    cut = lambda a, w: np.frombuffer(a, np.uint32).reshape(np_, w).tolist()
    return cut(start, nb + 1), cut(dense, nb + 1), cut(out, stride), stride


def sort_release():
    load("g1").mst_sort_release()


class TreeOut:
    pass


def tree(curve, bases, c, sorted_words, start, pad_log, T, ent_bound=0):
    """bases: affine pairs; sorted_words: np slices of padded_entries(n, c, pad_log) words; start: np lists of nb + 1 -> TreeOut with
    D[L][p], Q[L][p] (lists of nb + 1), keep[p], over_start[p], over_count (before, after), points[p] (level T's, by index), result[p]"""
    np_, n = len(start), len(bases)
    _, nb = M.geom(c)
    stride = padded_entries(n, c, pad_log)
    assert all(len(s) == stride for s in sorted_words) and all(len(s) == nb + 1 for s in start) and len(sorted_words) == np_
    F, _, w = CURVES[curve]
    row = np_ * (nb + 1)
    D, Q = (_U32 * ((T + 1) * row))(), (_U32 * ((T + 1) * row))()
    keep, over_start, over_count = (_U32 * row)(), (_U32 * row)(), (_U32 * 2)()
    cap = max(max(s[nb] for s in start), 1)   # level T has no more points than level 0 has entries
    pts, result, pts_stride = C.create_string_buffer(w * cap * np_), C.create_string_buffer(w * np_), _U64(0)
    rc = getattr(load(curve), "mst_%s_tree" % curve)(_wire(curve, bases), n, c, _u32s([e for s in sorted_words for e in s]), _u32s([v for s in start for v in s]),
                                                     np_, pad_log, T, _U64(ent_bound), D, Q, keep, over_start, over_count, pts, _U64(cap), C.byref(pts_stride),
                                                     result)
    assert rc == 0, rc
    o = TreeOut()
    lv = lambda a, L, p: list(a[(L * np_ + p) * (nb + 1):(L * np_ + p + 1) * (nb + 1)])
    o.D = [[lv(D, L, p) for p in range(np_)] for L in range(T + 1)]
    o.Q = [[lv(Q, L, p) for p in range(np_)] for L in range(T + 1)]
    o.keep = [lv(keep, 0, p) for p in range(np_)]
    o.over_start = [lv(over_start, 0, p) for p in range(np_)]
    o.over_count = (over_count[0], over_count[1])
    o.pts_stride = pts_stride.value
    take = min(cap, o.pts_stride)
    o.points = [_points(curve, pts.raw[w * cap * p:w * (cap * p + take)]) for p in range(np_)]
    o.result = _points(curve, result.raw)
    return o


def tails(curve, bases, c, sorted_words, start, nchunks, lone):
    """-> (bkt[p][b], result[p], n_heavy[p]) after msm_launch_accumulate with `nchunks` and msm_tails_enqueue over packed runs"""
    np_, n = len(start), len(bases)
    _, nb = M.geom(c)
    stride = max(max(len(s) for s in sorted_words), 1)
    flat = [e for s in sorted_words for e in list(s) + [M.POISON] * (stride - len(s))]
    F, _, w = CURVES[curve]
    bkt, result, n_heavy = C.create_string_buffer(w * nb * np_), C.create_string_buffer(w * np_), (_U32 * np_)()
    rc = getattr(load(curve), "mst_%s_tails" % curve)(_wire(curve, bases), n, c, _u32s(flat), _u32s([v for s in start for v in s]), np_, _U64(stride), nchunks,
                                                      1 if lone else 0, bkt, result, n_heavy)
    assert rc == 0, rc
    all_b = _points(curve, bkt.raw)
    return [all_b[nb * p:nb * p + nb] for p in range(np_)], _points(curve, result.raw), list(n_heavy)
