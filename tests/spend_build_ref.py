"""The spend-building and signing tests' other side and their shared inputs.  `reference` composes what the builder puts around a Spend
proof, and `sign_reference` a RedJubjub signature, from one-call primitives that the reference's vectors pin (H.jubjub_mul, H.jubjub_add,
H.value_commitment, nullifier_ref), hashlib's BLAKE2b and Python integers mod r_J: it goes through neither masp_host_sapling_build_spends
nor masp_host_redjubjub_sign_batch, and it imports nothing from masp_amd.redjubjub, so that the product's Python signer is tested against
it too.  The cases (edge scalars, one bad item per status, random batches) are computed once and shared by the host, the device-header and
the GPU files."""
import hashlib
import json
import os
import random

import numpy as np

import nullifier_ref as NR
from masp_amd import host as H

RJ = H.JUBJUB_ORDER
G_PGK = H.point_bytes(*H.generator_uv(0))       # proof_generation_key_generator
G_VCR = H.point_bytes(*H.generator_uv(3))       # value_commitment_randomness_generator
G_SPEND = H.point_bytes(*H.generator_uv(4))     # spending_key_generator
BASE = (G_SPEND, G_VCR)                         # by kind
ZERO = bytes(32)


def _le(k, n=32):
    return int(k).to_bytes(n, "little")


def _int(b):
    return int.from_bytes(b, "little")


# the scalars at which a four-bit fixed-base table can go wrong: zero, the first digit's ends, the second digit, the largest scalar, every
# digit 15 below r_J's top digit, digits alternating 0 and 15
EDGE_SCALARS = (0, 1, 15, 16, RJ - 1, (1 << 248) - 1, (((RJ >> 248) - 1) << 248) | ((1 << 248) - 1), int("0f" * 31, 16), int("f0" * 31, 16))
assert all(k < RJ for k in EDGE_SCALARS)


def key_vectors():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zip32_key_vectors.json")))["vectors"]


# ---- signatures ----
def h_star(*parts):
    return _int(hashlib.blake2b(b"".join(parts), digest_size=64, person=b"MASP__RedJubjubH").digest()) % RJ


def sign_reference(it):
    """it: dict(sk, alpha or None, sighash, kind, T) -> (status, vk, sig); the outputs are zeros where the status is not 0"""
    sk, alpha = _int(it["sk"]), _int(it["alpha"]) if it["alpha"] is not None else 0
    if sk >= RJ:
        return 1, ZERO, bytes(64)
    if alpha >= RJ:
        return 2, ZERO, bytes(64)
    g = BASE[it["kind"]]
    rsk = (sk + alpha) % RJ
    vk = H.jubjub_mul(g, _le(rsk))
    r = h_star(it["T"], vk, it["sighash"])
    rbar = H.jubjub_mul(g, _le(r))
    s = (r + h_star(rbar, vk, it["sighash"]) * rsk) % RJ
    return 0, vk, rbar + _le(s)


def good_item(seed, kind=None, alpha=True):
    rng = random.Random(seed)
    return dict(sk=_le(rng.randrange(RJ)), alpha=_le(rng.randrange(RJ)) if alpha else None, sighash=rng.randbytes(32),
                kind=rng.randrange(2) if kind is None else kind, T=rng.randbytes(80))


def spoil_item(it, status, variant=0):
    bad = (_le(RJ), _le((1 << 256) - 1), _le(RJ + 1))[variant % 3]
    return dict(it, sk=bad) if status == 1 else dict(it, alpha=bad)


def edge_items():
    """every edge scalar as sk without alpha on either basepoint, as rsk through sk + alpha, the wraparound, and rsk = 0 both ways"""
    out = []
    for j, k in enumerate(EDGE_SCALARS):
        for kind in (0, 1):
            out.append(dict(good_item(500 + j, kind), sk=_le(k), alpha=None))
        out.append(dict(good_item(520 + j), sk=_le((k - 5) % RJ), alpha=_le(5)))
    out.append(dict(good_item(540, 0), sk=_le(RJ - 1), alpha=_le(RJ - 1)))
    out.append(dict(good_item(541, 0), sk=_le(RJ - 7), alpha=_le(7)))       # sk + alpha is exactly r_J: rsk = 0, vk the identity
    out.append(dict(good_item(542, 1), sk=ZERO, alpha=ZERO))
    return out


def status_items():
    """[(control, spoiled, status)]"""
    return [(b, spoil_item(b, s, v), s) for s in (1, 2) for v in range(3) for b in [good_item(600 + 10 * s + v)]]


def double_items():
    base = good_item(650)
    return [(spoil_item(spoil_item(base, 2), 1), 1)]


def random_items(n, seed, bad_share=0.1):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        it = good_item(seed * 100000 + i)
        if rng.random() < bad_share:
            it = spoil_item(it, 1 + rng.randrange(2), rng.randrange(3))
        out.append(it)
    return out


def sign_arrays(items, alphas=True):
    """the five input arrays of either redjubjub_sign_batch call, in the C ABI's order.  alphas=False: None (the items must have none)"""
    n = len(items)
    cat = lambda f, w: np.frombuffer(b"".join(f(it) for it in items), np.uint8).reshape(n, w).copy()
    return (cat(lambda it: it["sk"], 32), cat(lambda it: it["alpha"] if it["alpha"] is not None else ZERO, 32) if alphas else None,
            cat(lambda it: it["sighash"], 32), np.array([it["kind"] for it in items], np.uint8), cat(lambda it: it["T"], 80))


def check_signs(got, want):
    """got: (status, vks or None, sigs) arrays; want: [sign_reference(item)]"""
    status, vks, sigs = got
    assert status.tolist() == [w[0] for w in want]
    if vks is not None:
        bad = [i for i, (g, w) in enumerate(zip(vks, want)) if g.tobytes() != w[1]]
        assert not bad, ("vk", bad[:8])
    bad = [i for i, (g, w) in enumerate(zip(sigs, want)) if g.tobytes() != w[2]]
    assert not bad, ("sig", bad[:8])


# ---- spends ----
FIELDS = ("asset", "value", "d", "pk_d", "lead", "rseed", "ak", "nsk", "ar", "rcv", "position")
ZEROS = (ZERO,) * 5


def _decodes(b):
    return H.load_library().masp_host_point_uv(b, bytes(64)) == 0


# encodings of points of small order: the identity, (0, -1), and the points with v = 0 (order four), as far as they decode
SMALL_ORDER = [b for b in (H.JUBJUB_IDENTITY, _le(H.FR_MODULUS - 1), ZERO, _le(1 << 255))
               if _decodes(b) and H.jubjub_mul(b, 8) == H.JUBJUB_IDENTITY]
assert len(SMALL_ORDER) >= 3, SMALL_ORDER


def status_of(p):
    """the status the semantics give a spend, from the one-call primitives"""
    s = NR.status_of(dict(p, nk=NR.G_NCR))
    if s:
        return s
    if not _decodes(p["ak"]):
        return 5
    if H.jubjub_mul(p["ak"], 8) == H.JUBJUB_IDENTITY:
        return 6
    for s, f in ((7, "nsk"), (8, "ar"), (9, "rcv")):
        if _int(p[f]) >= RJ:
            return s
    return 0


def reference(p):
    """-> (status, cv, rk, nf, cmu, nk); the outputs are zeros where the status is not 0"""
    s = status_of(p)
    if s:
        return (s,) + ZEROS
    nk = H.jubjub_mul(G_PGK, p["nsk"])
    rk = H.jubjub_add(p["ak"], H.jubjub_mul(G_SPEND, p["ar"]))
    cv = H.value_commitment(p["asset"], p["value"], p["rcv"])[0]
    _, cmu, nf = NR.reference(dict(p, nk=nk))
    return 0, cv, rk, nf, cmu, nk


def good_spend(seed, lead=None):
    rng = random.Random(seed)
    n = NR.good_note(seed, lead)
    n.pop("nk")
    return dict(n, ak=H.jubjub_mul(G_SPEND, _le(rng.randrange(1, RJ))), nsk=_le(rng.randrange(RJ)), ar=_le(rng.randrange(RJ)),
                rcv=_le(rng.randrange(RJ)))


def spoil(p, status, variant=0):
    """the spend with the one field changed that gives it `status`"""
    if status <= 4:
        q = NR.spoil(dict(p, nk=None), status, variant)
        q.pop("nk")
        return q
    if status == 5:
        return dict(p, ak=(NR.OFF_CURVE, NR.NOT_CANONICAL, NR.NEGATIVE_ZERO)[variant % 3])
    if status == 6:
        return dict(p, ak=SMALL_ORDER[variant % len(SMALL_ORDER)])
    return dict(p, **{("nsk", "ar", "rcv")[status - 7]: (_le(RJ), _le((1 << 256) - 1))[variant % 2]})


def status_spends():
    """[(control, spoiled, status)]: every status, every way to it, next to the spend that differs in that one field"""
    out = []
    for s, variants in ((1, 1), (2, 1), (3, 3), (4, 5), (5, 3), (6, len(SMALL_ORDER)), (7, 2), (8, 2), (9, 2)):
        for v in range(variants):
            base = good_spend(900 + 10 * s + v, 1 if s == 4 and v < 2 else None)
            out.append((base, spoil(base, s, v), s))
    return out


def double_spends():
    """[(spoiled, status)]: two checks fail, the first in the order counts"""
    base = good_spend(999, 1)
    sp = lambda a, b: spoil(spoil(base, a), b)
    return [(sp(9, 2), 2), (sp(5, 3), 3), (sp(7, 4), 4), (sp(9, 5), 5), (sp(8, 7), 7), (sp(9, 8), 8), (sp(1, 9), 1), (sp(9, 7), 7)]


def edge_spends():
    """the edge scalars as nsk, ar and rcv on a spend of either lead byte"""
    out = []
    for j, k in enumerate(EDGE_SCALARS):
        base = good_spend(700 + j, 1 + j % 2)
        out += [dict(base, nsk=_le(k)), dict(base, ar=_le(k)), dict(base, rcv=_le(k))]
    return out


def random_batch(n, seed, bad_share=0.1):
    """n spends of both lead bytes, about bad_share of them spoiled across the nine statuses"""
    rng = random.Random(seed)
    out, spoiled = [], 0
    for i in range(n):
        p = good_spend(seed * 100000 + i)
        if rng.random() < bad_share:
            p = spoil(p, 1 + spoiled % 9, rng.randrange(30))
            spoiled += 1
        out.append(p)
    return out


def arrays(spends):
    """the eleven input arrays of either build_spends call, in the C ABI's order"""
    n = len(spends)
    cat = lambda f, w: np.frombuffer(b"".join(p[f] for p in spends), np.uint8).reshape(n, w).copy()
    return (cat("asset", 32), np.array([p["value"] for p in spends], np.uint64), cat("d", 11), cat("pk_d", 32),
            np.array([p["lead"] for p in spends], np.uint8), cat("rseed", 32), cat("ak", 32), cat("nsk", 32), cat("ar", 32), cat("rcv", 32),
            np.array([p["position"] for p in spends], np.uint64))


def as_plans(spends):
    """the spends as note_encryption's ((ak, nsk), Note, PaymentAddress, position, ar, rcv)"""
    from masp_amd import note_encryption as NE
    return [((p["ak"], p["nsk"]), NE.Note(p["asset"], p["value"], p["pk_d"], NE.Rseed(p["lead"], p["rseed"])), NE.PaymentAddress(p["d"], p["pk_d"]),
             p["position"], p["ar"], p["rcv"]) for p in spends]


def check(got, want):
    """got: (status, cvs, rks, nfs, cmus or None, nks or None) arrays; want: [reference(spend)]"""
    assert got[0].tolist() == [w[0] for w in want]
    for k, name in enumerate(("cv", "rk", "nf", "cmu", "nk"), 1):
        if got[k] is None:
            continue
        bad = [i for i, (g, w) in enumerate(zip(got[k], want)) if g.tobytes() != w[k]]
        assert not bad, (name, bad[:8])


_cache = {}


def references(name, make, ref=reference):
    """(items, [ref(item)]) of a named list, computed once"""
    if name not in _cache:
        items = make()
        _cache[name] = (items, [ref(p) for p in items])
    return _cache[name]


def batch(n, seed=43):
    """the first n spends of one random batch of 130 and their references: the sizes of a test share a prefix"""
    spends, want = references("spends%d" % seed, lambda: random_batch(130, seed))
    return spends[:n], want[:n]


def sign_batch(n, seed=47):
    """the first n items of one random batch of 130 and their references"""
    items, want = references("items%d" % seed, lambda: random_items(130, seed), sign_reference)
    return items[:n], want[:n]
