"""Loader of the test-only units over doubled window rows: tests/native/msm_twin_host.hip (the geometry, host code only: needs no
device) and tests/native/msm_twin_dev.hip (the sort, the table, the accumulation and the tails through the product's drivers; once per
curve, side by side, as tests/msm_stages_shim.py builds its unit), with the product's flags as native_build.py reads them from the Makefile.
Everything that goes in or comes out is plain: Python ints, lists of ints, points as affine pairs with the pair of zeros for the point at
infinity."""
import ctypes as C

import numpy as np

import msm_stage_models as M
import msm_twin_models as TM
import native_build
from pyref import F1, F2, g1_unc, g2_unc

HOST = native_build.unit("msm_twin_host")
UNITS = {"g1": native_build.unit("msm_twin_dev", "_g1"), "g2": native_build.unit("msm_twin_dev", "_g2", ["-DMTW_G2"])}
CURVES = {"g1": (F1, g1_unc, 96), "g2": (F2, g2_unc, 192)}
_U32, _U64 = C.c_uint32, C.c_uint64
_libs = {}


def load_host():
    return native_build.load(HOST)


def geom(c, twin=True):
    """-> dict of MsmGeom's fields for msm_geom_twin(c) / msm_geom(c), |B| and the number of classes"""
    out = (_U32 * 7)()
    load_host().mtw_geom(c, 1 if twin else 0, out)
    return dict(zip(("c", "W", "nb", "twin", "tables", "buckets", "classes"), list(out)))


def klass(c, s):
    out = (_U32 * 3)()
    load_host().mtw_class(c, s, out)
    return tuple(out)


def bucket(c, v):
    """digit magnitude -> (row multiple, bucket id)"""
    mult = _U32(0)
    b = load_host().mtw_bucket(c, v, C.byref(mult))
    return 1 << mult.value, int(b)


def load(curve):
    if not _libs:
        _libs.update(zip(UNITS, native_build.load_all(UNITS.values())))
        _libs["g1"].mtw_padded_entries.restype = _U64
    return _libs[curve]


def _u32s(vals):
    return (_U32 * len(vals))(*vals)


def _wire(curve, pts):
    F, unc, _ = CURVES[curve]
    return b"".join(unc(M.to_ref(F, p)) for p in pts)


def _points(curve, raw):
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
    return int(load("g1").mtw_padded_entries(n, c, pad_log))


def sort(scalars, c, pad_log, subset=None):
    """scalars: np lists of n ints; subset: None or (bits, b_first, b_end, bad set) -> (start, dense, sorted, ent_stride): per proof lists"""
    np_, n = len(scalars), len(scalars[0])
    _, nb = TM.geom(c)
    stride = padded_entries(n, c, pad_log)
    raw = b"".join([int(s).to_bytes(32, "little") for v in scalars for s in v])
    start, dense, out = (_U32 * (np_ * (nb + 1)))(), (_U32 * (np_ * (nb + 1)))(), (_U32 * (np_ * stride))()
    bits, b_first, b_end, bad = subset if subset is not None else (0, 0, 0, set())
    words = [0] * max(1, (b_end - b_first + 31) // 32)
    for rb in bad:
        words[rb >> 5] |= 1 << (rb & 31)
    rc = load("g1").mtw_sort(raw, n, c, np_, pad_log, bits, b_first, b_end, _u32s(words), start, dense, out)
    assert rc == 0, rc
    cut = lambda a, w: np.frombuffer(a, np.uint32).reshape(np_, w).tolist()
    return cut(start, nb + 1), cut(dense, nb + 1), cut(out, stride), stride


def table(curve, bases, c, sub_bits=0):
    """-> (rows as affine pairs, info dict) of the table MsmBases::load_host builds when asked for doubled rows"""
    n = len(bases)
    W, _ = M.geom(c)
    cap = 2 * W * n + (n >> 2) * 255 + 8
    w = CURVES[curve][2]
    rows, info = C.create_string_buffer(w * cap), (_U32 * 6)()
    rc = getattr(load(curve), "mtw_%s_table" % curve)(_wire(curve, bases), n, c, sub_bits, rows, _U64(cap), info)
    assert rc == 0, rc
    d = dict(zip(("twin", "W", "nb", "rows", "row0", "status"), list(info)))
    return _points(curve, rows.raw[:w * d["rows"]]), d


def tails(curve, bases, c, sorted_words, start, nchunks, lone):
    """-> (bkt[p][b], result[p]) after msm_launch_accumulate with `nchunks` and msm_tails_enqueue over packed runs on the doubled tables"""
    np_, n = len(start), len(bases)
    _, nb = TM.geom(c)
    stride = max(max(len(s) for s in sorted_words), 1)
    flat = [e for s in sorted_words for e in list(s) + [M.POISON] * (stride - len(s))]
    w = CURVES[curve][2]
    bkt, result = C.create_string_buffer(w * nb * np_), C.create_string_buffer(w * np_)
    rc = getattr(load(curve), "mtw_%s_tails" % curve)(_wire(curve, bases), n, c, _u32s(flat), _u32s([v for s in start for v in s]), np_, _U64(stride), nchunks,
                                                      1 if lone else 0, bkt, result)
    assert rc == 0, rc
    all_b = _points(curve, bkt.raw)
    return [all_b[nb * p:nb * p + nb] for p in range(np_)], _points(curve, result.raw)
