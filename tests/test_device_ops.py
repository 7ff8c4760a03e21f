"""The layers of masp_amd/csrc/device/ above the base-field ops, op by op, against python big integers (tests/pyref.py): the
inversions and the power, the register-argument products, Fp2 in one lane (Fp2Ops) and over a lane pair (Fp2PairOps /
Fp2PairCold), the XYZZ group law over FpOps / Fp2Ops / Fp2PairOps, over quads (FpQuadOps, device/quad.hpp) and octs
(Fp2OctOps, device/oct.hpp), and the grid-wide batch inversion of the bucket trees (k_binv_*).  Every case that an MSM reaches
only when random points happen to hit it is named here: the bingcd operands that stress its 64-bit approximations, the halves
of an Fp2 that are zero or equal on their own, the same-x branches reached through projective equality.  The test shim
(tests/native/device_math_host.hip) is built with the product's flags; the host-compiled forms are checked without a GPU,
the rest with -m gpu."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import device_shim
from pyref import F1, F2, G1, G2, P, R, ec_add, ec_mul

RP, RR = 1 << 384, 1 << 256   # Montgomery radices of Fp, Fr
BLOCKS = (64, 256)


@pytest.fixture(scope="module")
def mh():
    return device_shim.load()


def _fmt(v):
    if isinstance(v, int):
        return hex(v)
    if v is None:
        return "inf"
    return "(" + ", ".join(_fmt(x) for x in v) + ")"


def _first_bad(got, want, inputs, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            raise AssertionError("%s: first failing index %d of %d, input %s: got %s, want %s" % (what, i, len(got), _fmt(inputs[i]), _fmt(g), _fmt(w)))
    assert len(got) == len(want)


def _enc(vals, nb):
    return b"".join(v.to_bytes(nb, "little") for v in vals)


def _dec(raw, nb, n):
    return [int.from_bytes(raw[nb * i:nb * (i + 1)], "little") for i in range(n)]


def _enc2(vals):
    return b"".join(a.to_bytes(48, "little") + b.to_bytes(48, "little") for a, b in vals)


def _dec2(raw, n):
    v = _dec(raw, 48, 2 * n)
    return [(v[2 * i], v[2 * i + 1]) for i in range(n)]


# ---- A. inversions and the power -------------------------------------------------------------------------------------------
def _inv_operands(mod, nb, rng, nrand=2000):
    """the edge values of test_field_ops, the shapes that stress the binary gcd's 64-bit approximations (powers of two and their
    neighbours, p - 2^k, long runs of ones, (p >> k) | 1) and random values"""
    bits = mod.bit_length()
    edge = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2, 0xffffffff, 1 << 32, (1 << (8 * nb - 8)) % mod]
    special = [1 << k for k in range(1, bits - 1)] + [(1 << k) + 1 for k in range(1, bits - 1, 5)] + [(1 << k) - 1 for k in range(2, bits - 1)] + \
              [mod - (1 << k) for k in range(0, bits - 2)] + [((1 << 62) + 1) << k for k in range(0, bits - 64, 7)] + \
              [(mod >> k) | 1 for k in range(1, 200, 3)]
    return edge + [x % mod for x in special] + [rng.randrange(mod) for _ in range(nrand)] + [rng.randrange(1 << rng.randrange(1, bits)) for _ in range(200)]


def _check_inversions(run, ops, which, nsub=None):
    """run(which, op, values, exponent words) -> values; ops: the op codes to check (0 fe_inv_bingcd 1 fe_inv_bingcd_nc 2 fe_inv
    3 fe_inv_fermat 4 fe_pow)"""
    mod, nb = ((P, 48), (R, 32))[which]
    rng = random.Random(40 + which)
    vals = _inv_operands(mod, nb, rng)
    names = {0: "fe_inv_bingcd", 1: "fe_inv_bingcd_nc", 2: "fe_inv", 3: "fe_inv_fermat"}
    for op in ops:
        if op == 4:
            continue
        vs = vals if nsub is None or op == 0 else vals[:nsub]
        got = run(which, op, vs, [0])
        _first_bad(got, [pow(a, -1, mod) if a else 0 for a in vs], vs, "%s %s" % ("Fp" if which == 0 else "Fr", names[op]))
    if 4 in ops:
        vs = vals[:10] + [rng.randrange(mod) for _ in range(100 if nsub is None else 20)]
        for e in (0, 1, 2, 3, mod - 1, mod - 2, (mod - 1) // 2, 1 << 200, rng.randrange(mod)):
            words = [(e >> (32 * i)) & 0xffffffff for i in range(nb // 4)]
            got = run(which, 4, vs, words)
            _first_bad(got, [pow(a, e, mod) for a in vs], vs, "%s fe_pow e = %s" % ("Fp" if which == 0 else "Fr", hex(e)))


def _inv_runner(fn):
    def run(which, op, vals, words):
        nb = 48 if which == 0 else 32
        out = C.create_string_buffer(nb * len(vals))
        e = (C.c_uint32 * len(words))(*words)
        assert fn(which, op, _enc(vals, nb), e, len(words), out, len(vals)) == 0
        return _dec(out.raw, nb, len(vals))
    return run


@pytest.mark.parametrize("which", [0, 1])
def test_inversions_host(mh, which):
    """the same source compiled for the host: the divsteps' ctz64 and __int128 take their portable forms there"""
    _check_inversions(_inv_runner(mh.mh_inv_ops), (0, 1, 2, 3, 4), which, nsub=150)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_inversions_on_the_device(mh, which):
    """fe_inv_bingcd (the shared inversions of every bucket tree), its out-of-line form, fe_inv (divsteps: __ffsll and __int128
    on the device), fe_inv_fermat and fe_pow (chains of register-argument products) on the GPU"""
    _check_inversions(_inv_runner(mh.mh_inv_ops_gpu), (0, 1, 2, 3, 4), which)


# ---- B. the register-argument products -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_register_argument_products_on_the_device(mh):
    """fe_mul_nc / fe_sqr_nc (fp_mul_call / fp_sqr_call: operands in VGPR vectors) and fe_mul_ref (Fr): the output contract of
    fe_mul on the same inputs — canonical operands and, for Fp, raw operands anywhere in [0, 2p) — byte for byte"""
    rng = random.Random(41)
    top = (2 * P) >> 352
    for which, mod, nb, RM in ((0, P, 48, RP), (1, R, 32, RR)):
        rinv = pow(RM, -1, mod)
        edge = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2, 0xffffffff, 1 << 32, (1 << (8 * nb - 8)) % mod, mod - (1 << 32)]
        if which == 0:
            edge += [P, P + 1, 2 * P - 1, 2 * P - 2, (1 << 381) - 1, 1 << 381, (1 << 352) - 1, (top << 352), (top << 352) | 0xffffffff,
                     ((top - 1) << 352) | ((1 << 352) - 1)]
        lim = 2 * mod if which == 0 else mod
        pairs = [(a, b) for a in edge for b in edge] + [(rng.randrange(lim), rng.randrange(lim)) for _ in range(3000)]
        A, B = _enc([a for a, _ in pairs], nb), _enc([b for _, b in pairs], nb)
        n = len(pairs)
        out = C.create_string_buffer(nb * n)
        res = {}
        for op in (0, 1, 2, 3, 4):
            assert mh.mh_cold_products_gpu(which, op, A, B, out, n) == 0
            res[op] = _dec(out.raw, nb, n)
        name = "Fp" if which == 0 else "Fr"
        _first_bad(res[2], [a * b * rinv % mod for a, b in pairs], pairs, name + " fe_mul")
        _first_bad(res[0], res[2], pairs, name + " fe_mul_nc against fe_mul")
        _first_bad(res[4], res[2], pairs, name + " fe_mul_ref against fe_mul")
        _first_bad(res[3], [a * a * rinv % mod for a, _ in pairs], pairs, name + " fe_sqr")
        _first_bad(res[1], res[3], pairs, name + " fe_sqr_nc against fe_sqr")


# ---- C. Fp2 ------------------------------------------------------------------------------------------------------------------
def _fp2_cases():
    """(a, b) pairs: halves zero on their own, (x, +-x), (1, 1), (p - 1, p - 1); b equal to a, equal in one half only, random"""
    rng = random.Random(42)
    xs = [1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 0xffffffff, 1 << 32, 1 << 200] + [rng.randrange(P) for _ in range(6)]
    els = [(0, 0), (1, 0), (0, 1), (1, 1), (P - 1, P - 1)]
    for x in xs:
        els += [(0, x), (x, 0), (x, x), (x, P - x)]
    els += [(rng.randrange(P), rng.randrange(P)) for _ in range(1500)]
    pairs = []
    for a in els:
        pairs.append((a, a))
        pairs.append((a, (a[0], (a[1] + 1) % P)))
        pairs.append((a, ((a[0] + 1) % P, a[1])))
        pairs.append((a, rng.choice(els)))
    return pairs


def _fp2_want(op, a, b):
    inv = lambda a: (0, 0) if a == (0, 0) else F2.inv(a)
    flags = lambda a, b: ((1 if a == (0, 0) else 0) | (2 if a == b else 0), 0)
    return {0: lambda: F2.add(a, b), 1: lambda: F2.sub(a, b), 2: lambda: F2.neg(a), 3: lambda: F2.add(a, a), 4: lambda: F2.mul(a, b),
            5: lambda: F2.mul(a, a), 6: lambda: inv(a), 7: lambda: inv(a), 8: lambda: inv(a), 9: lambda: flags(a, b), 10: lambda: F2.mul(a, b)}[op]()


FP2_NAMES = {0: "add", 1: "sub", 2: "neg", 3: "dbl", 4: "mul", 5: "sqr", 6: "inv", 7: "inv_lone", 8: "inv_gcd", 9: "is_zero | eq", 10: "mul_lazy"}


def _check_fp2ops(fn):
    pairs = _fp2_cases()
    n = len(pairs)
    A, B = _enc2([a for a, _ in pairs]), _enc2([b for _, b in pairs])
    out = C.create_string_buffer(96 * n)
    for op in range(11):
        ps = pairs if op not in (6, 7) else pairs[::8]
        if op in (6, 7):
            A_, B_ = _enc2([a for a, _ in ps]), _enc2([b for _, b in ps])
        else:
            A_, B_ = A, B
        assert fn(op, A_, B_, out, len(ps)) == 0
        _first_bad(_dec2(out.raw, len(ps)), [_fp2_want(op, a, b) for a, b in ps], ps, "Fp2Ops::" + FP2_NAMES[op])


def test_fp2ops_host(mh):
    _check_fp2ops(mh.mh_fp2_ops)


@pytest.mark.gpu
def test_fp2ops_on_the_device(mh):
    """Fp2Ops on the GPU: Karatsuba over register-argument products, the three inversions of the norm"""
    _check_fp2ops(mh.mh_fp2_ops_gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_fp2_pair_ops_on_the_device(mh, block):
    """Fp2PairOps / Fp2PairCold (c0 on the even lane, c1 on the odd lane, the partner's half by a DPP quad permutation): both
    halves stored.  is_zero / eq must hold on BOTH lanes and only when both halves agree (cases with one half zero or equal)"""
    pairs = _fp2_cases()
    n = len(pairs)
    A, B = _enc2([a for a, _ in pairs]), _enc2([b for _, b in pairs])
    out = C.create_string_buffer(96 * n)
    names = {0: "mul", 1: "mul_lazy", 2: "sqr", 3: "one", 4: "is_zero | eq", 5: "inv_gcd", 6: "Fp2PairCold::mul", 7: "Fp2PairCold::sqr"}
    for op in range(8):
        assert mh.mh_fp2pair_ops_gpu(op, A, B, out, n, block) == 0
        got = _dec2(out.raw, n)
        if op == 4:
            f = [_fp2_want(9, a, b)[0] for a, b in pairs]
            want = [(x, x) for x in f]   # the flag word on both lanes
        else:
            want = [_fp2_want({0: 4, 1: 4, 2: 5, 5: 8, 6: 4, 7: 5}[op], a, b) if op != 3 else (1, 0) for a, b in pairs]
        _first_bad(got, want, pairs, "Fp2PairOps::%s (block %d)" % (names[op], block))


# ---- D, E, F. the group law ------------------------------------------------------------------------------------------------
# forms: (which, field, LANES, PARTS, bytes of a lane's part, ops)
ALL_OPS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
FORMS = {"FpOps": (0, F1, 1, 1, 48, ALL_OPS), "Fp2Ops": (1, F2, 1, 1, 96, ALL_OPS), "Fp2PairOps": (2, F2, 2, 2, 48, (0, 1, 2, 3, 4, 5, 6, 7, 10)),
         "FpQuadOps": (3, F1, 4, 1, 48, (5, 6, 10)), "Fp2OctOps": (4, F2, 8, 2, 48, (5, 6, 10))}
PT_NAMES = {0: "xyzz_madd", 1: "xyzz_madd(negate)", 2: "xyzz_madd_nc", 3: "xyzz_madd_nc(negate)", 4: "xyzz_add", 5: "xyzz_add_nc", 6: "xyzz_dbl",
            7: "xyzz_dbl_affine", 8: "xyzz_to_affine<O, false>", 9: "xyzz_to_affine<O, true>", 10: "xyzz_mul_scalar"}


def _rnd(F, rng):
    return rng.randrange(1, P) if F is F1 else (rng.randrange(P), rng.randrange(1, P))


def _neg_pt(F, p):
    return None if p is None else (p[0], F.neg(p[1]))


def _rep(F, p, rng):
    """a random XYZZ representative of affine p (random Z); infinity: all zero"""
    if p is None:
        return (F.zero, F.zero, F.zero, F.zero)
    z = _rnd(F, rng)
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    return (F.mul(p[0], zz), F.mul(p[1], zzz), zz, zzz)


def _aff_rep(F, p):
    return (F.zero, F.zero, F.one, F.one) if p is None else (p[0], p[1], F.one, F.one)


_POINTS = {}


def _points(F):
    if F not in _POINTS:
        rng = random.Random(43 if F is F1 else 44)
        g = G1 if F is F1 else G2
        base = [ec_mul(F, g, rng.randrange(1, R)) for _ in range(4)]
        _POINTS[F] = base + [ec_add(F, base[i], base[(i + 1) % 4]) for i in range(4)]
    return _POINTS[F]


def _pt_cases(F, op, rng):
    """(acc, b, scalar) affine cases of op: generic, infinity as either or both operands, acc = +-b as points in different
    representatives (the same-x branches), the doubling of a point"""
    pts = _points(F)
    if op == 10:
        return [(p, None, k) for p in pts[:3] + [None] for k in (0, 1, 2, R - 1, rng.randrange(R))]
    if op == 7:
        return [(None, p, 0) for p in pts + [None]]
    if op in (6, 8, 9):
        return [(p, None, 0) for p in pts + [None]] + [(pts[0], None, 0)] * 2
    cases = [(pts[i], pts[(i + 3) % len(pts)], 0) for i in range(len(pts))]
    cases += [(pts[0], None, 0), (None, pts[1], 0), (None, None, 0)]
    cases += [(p, p, 0) for p in pts[:4]] + [(p, _neg_pt(F, p), 0) for p in pts[:4]]
    return cases


def _pt_want(F, op, acc, b, k):
    if op in (0, 2, 4, 5):
        return ec_add(F, acc, b)
    if op in (1, 3):
        return ec_add(F, acc, _neg_pt(F, b))
    if op == 6:
        return ec_add(F, acc, acc)
    if op == 7:
        return ec_add(F, b, b) if b is not None else None
    if op in (8, 9):
        return acc
    return ec_mul(F, acc, k) if acc is not None else None


def _to_aff(F, X, Y, ZZ, ZZZ):
    """affine point of an XYZZ result (None: infinity); checks ZZ^3 = ZZZ^2"""
    if ZZ == F.zero:
        return None
    if F.mul(F.mul(ZZ, ZZ), ZZ) != F.mul(ZZZ, ZZZ):
        return ("not an XYZZ point: ZZ^3 != ZZZ^2", X, Y, ZZ, ZZZ)
    return (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))


def _enc_el(F, v):
    return v.to_bytes(48, "little") if F is F1 else v[0].to_bytes(48, "little") + v[1].to_bytes(48, "little")


def _check_points(fn, form, block=None, reps=1):
    which, F, LANES, PARTS, TB, ops = FORMS[form]
    rng = random.Random(45 + which)
    for op in ops:
        cases = _pt_cases(F, op, rng) * reps
        rng.shuffle(cases)   # every case at every position of a row, in later rows and waves
        n = len(cases)
        accs = [_rep(F, a, rng) for a, _, _ in cases]
        bs = [(_aff_rep(F, b) if op in (0, 1, 2, 3, 7) else _rep(F, b, rng)) for _, b, _ in cases]
        A = b"".join(_enc_el(F, e) for p in accs for e in p)
        B = b"".join(_enc_el(F, e) for p in bs for e in p)
        K = b"".join((k % R).to_bytes(32, "little") for _, _, k in cases)
        out = C.create_string_buffer(n * LANES * 4 * TB)
        rc = fn(which, op, A, B, K, out, n) if block is None else fn(which, op, A, B, K, out, n, block)
        assert rc == 0, (form, op, rc)
        raw = out.raw
        got = []
        for g in range(n):
            copies = []
            for c in range(LANES // PARTS):
                parts = []
                for h in range(PARTS):
                    base = ((g * LANES) + c * PARTS + h) * 4 * TB
                    parts.append([int.from_bytes(raw[base + j * TB:base + j * TB + 48], "little") for j in range(4)] if TB == 48 else
                                 [(int.from_bytes(raw[base + j * TB:base + j * TB + 48], "little"),
                                   int.from_bytes(raw[base + j * TB + 48:base + j * TB + 96], "little")) for j in range(4)])
                copies.append(parts[0] if PARTS == 1 else [(parts[0][j], parts[1][j]) for j in range(4)])
            assert all(cp == copies[0] for cp in copies), "%s %s: the lanes of group %d disagree: %s" % (form, PT_NAMES[op], g, copies)
            X, Y, ZZ, ZZZ = copies[0]
            if op in (8, 9):
                got.append(None if (X, Y) == (F.zero, F.zero) else (X, Y))
            else:
                got.append(_to_aff(F, X, Y, ZZ, ZZZ))
        want = [_pt_want(F, op, a, b, k) for a, b, k in cases]
        _first_bad(got, want, [(a, b, k, acc_r, b_r) for (a, b, k), acc_r, b_r in zip(cases, accs, bs)],
                   "%s %s%s" % (form, PT_NAMES[op], "" if block is None else " (block %d)" % block))


@pytest.mark.parametrize("form", ["FpOps", "Fp2Ops"])
def test_group_law_host(mh, form):
    """the group law as the host compiles it, every form and case (the same-x branches through projective equality)"""
    _check_points(mh.mh_pt_ops, form)


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("form", list(FORMS))
def test_group_law_on_the_device(mh, form, block):
    """the group law on the GPU: FpOps and Fp2Ops (inline and register-argument products, the out-of-line same-x cases of G2),
    lane pairs, quads (DPP quad broadcasts) and octs (quad_perm + row_shr:4 / row_shl:4 under bank masks): every lane of a group
    stores its copy, all copies must agree"""
    _check_points(mh.mh_pt_ops_gpu, form, block, reps=3)


# ---- G. the batch inversion ------------------------------------------------------------------------------------------------
# (n, BINV_C, BINV_MID): the product's constants, and scaled down so that small sizes reach both paths of batch_invert
# (n <= 4 BINV_MID: k_binv_mid alone; above: k_binv_fwd -> k_binv_mid -> k_binv_bwd), n = 1, n < M, n = M, n = k M +- 1, M not a
# multiple of 64
BINV_SHAPES = [(1, 16, 4096), (5, 16, 4096), (3000, 16, 4096), (1, 4, 37), (20, 4, 37), (37, 4, 37), (38, 4, 37), (73, 4, 37), (74, 4, 37),
               (75, 4, 37), (111, 4, 37), (148, 4, 37), (149, 4, 37), (150, 4, 37), (1000, 4, 37), (257, 16, 64), (2000, 16, 64), (21, 3, 5),
               (100, 3, 5), (257, 16, 100), (401, 16, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_batch_inversion_on_the_device(mh, which):
    """out[i] in[i] = 1 in Montgomery form (raw limbs: out * in = R^2 mod p) and out canonical.  FpOps inputs include values in
    [p, 2p): the lazily reduced chain totals of pass 1 are what batch_invert receives"""
    rng = random.Random(46 + which)
    r2 = RP * RP % P
    edge = [1, 2, P - 1, (P - 1) // 2, 1 << 32, 1 << 380, P - (1 << 64)]
    for n, bc, bm in BINV_SHAPES:
        if which == 0:
            vals = [rng.choice(edge) if rng.random() < 0.1 else rng.randrange(1, P) for _ in range(n)]
            vals = [v + P if rng.random() < 0.3 else v for v in vals]   # raw values in [p, 2p)
            inp = _enc(vals, 48)
        else:
            vals = [rng.choice([(0, rng.randrange(1, P)), (rng.randrange(1, P), 0), (1, 1), (P - 1, P - 1)]) if rng.random() < 0.2 else
                    (rng.randrange(P), rng.randrange(1, P)) for _ in range(n)]
            inp = _enc2(vals)
        nb = 48 if which == 0 else 96
        out = C.create_string_buffer(nb * n)
        assert mh.mh_binv_gpu(which, inp, n, bc, bm, out) == 0
        if which == 0:
            got = _dec(out.raw, 48, n)
            _first_bad([(g < P, g * v % P) for g, v in zip(got, vals)], [(True, r2)] * n, vals,
                       "FpOps batch inversion n = %d BINV_C = %d BINV_MID = %d" % (n, bc, bm))
        else:
            got = _dec2(out.raw, n)
            _first_bad([(g[0] < P and g[1] < P, F2.mul(g, v)) for g, v in zip(got, vals)], [(True, (r2, 0))] * n, vals,
                       "Fp2PairOps batch inversion n = %d BINV_C = %d BINV_MID = %d" % (n, bc, bm))


# ---- the long-branch hazard ------------------------------------------------------------------------------------------------
def test_shim_device_code_is_free_of_the_long_branch_hazard(tmp_path):
    """the shim's device assembly with the product's flags through tools/check_codeobj.py: the out-of-line calls it instantiates
    (fe_inv*, fe_pow, the same-x cases, the register-argument products) stay clear of the relaxed long branches described at the
    top of device/field.hpp before the shim ever reaches a GPU"""
    s = str(tmp_path / "device_math_host.s")
    subprocess.check_call(device_shim.asm_command(s))
    r = subprocess.run([sys.executable, os.path.join(device_shim.ROOT, "tools", "check_codeobj.py"), s], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_shim_is_built_with_the_product_flags():
    """the build command of the shim, and of every other unit the *_shim modules declare, carries FLAGS of masp_amd/csrc/Makefile, in
    order, and stays a shared, position-independent library; the shim's recorded dependencies are the headers it includes"""
    flags = device_shim.makefile_flags()
    assert "-O3" in flags and "-Wall" in flags and "--offload-arch=gfx950" in flags
    units = device_shim.native_build.declared_units()
    assert device_shim.UNIT in units and len(units) >= 22
    for unit in units:
        cmd = unit.command()
        i = cmd.index(flags[0])
        assert cmd[i:i + len(flags)] == flags, unit.so
        assert "-shared" in cmd and "-fPIC" in cmd, unit.so
        assert not any(f.startswith("-O") and f != "-O3" for f in cmd), unit.so
    device_shim.load()
    deps = device_shim.UNIT.dependencies()
    for h in ("field.hpp", "curve.hpp", "quad.hpp", "oct.hpp", "msm_tree.hpp", "msm_geom.h", "io.hpp", "consts.hpp", "fp28.hpp"):
        assert any(os.path.basename(d) == h for d in deps), h
