"""The host side of bundle validation (masp_amd/verifier.py), CPU only: the public inputs SaplingVerificationContext packs against the
circuits' own input assignments, the completeness of Jubjub's addition law the device relies on (device/jubjub.hpp), and a big-integer
restatement of the RedJubjub batch equation of masp_hip_redjubjub_verify_batch against per-signature verification."""
import random

from masp_amd import host as H
from masp_amd import redjubjub as RJS
from masp_amd import verifier as V
from masp_amd import workload as W

Q = H.FR_MODULUS
RJ = H.JUBJUB_ORDER
D = (-10240 * pow(10241, -1, Q)) % Q


def test_jubjub_addition_law_is_complete():
    """a = -1 a square and d a non-square in Fr: the unified addition is then complete (the device uses it for P + P, O, small order)."""
    assert pow(Q - 1, (Q - 1) // 2, Q) == 1
    assert pow(D, (Q - 1) // 2, Q) == Q - 1
    assert D == 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1


def test_public_inputs_equal_the_circuits_input_assignments():
    for seed in range(2):
        _, kw = W.description("spend", seed)
        ak, nsk = kw["proof_generation_key"]
        sib, pos = kw["merkle_path"]
        inputs, _, cv, rk, nf = H.spend_assignment(ak, nsk, kw["diversifier"], kw["rcm"], kw["ar"], kw["asset_type"], kw["value"],
                                                   kw["anchor"], sib, pos, kw["rcv"])
        assert V.spend_public_inputs(cv, kw["anchor"], nf, rk) == W.public_inputs(inputs)
        _, kw = W.description("convert", seed)
        sib, pos = kw["merkle_path"]
        inputs, _, cv = H.convert_assignment(kw["allowed_conversion"].generator, kw["value"], kw["anchor"], sib, pos, kw["rcv"])
        assert V.convert_public_inputs(cv, kw["anchor"]) == W.public_inputs(inputs)
        _, kw = W.description("output", seed)
        d, pk = kw["payment_address"]
        inputs, _, cv = H.output_assignment(kw["esk"], d, pk, kw["rcm"], kw["asset_type"], kw["value"], kw["rcv"])
        pub = W.public_inputs(inputs)
        epk = H.point_bytes(pub[2], pub[3])           # the circuit's epk = [esk] g_d, re-encoded
        assert H.jubjub_mul(epk, 1) == epk
        assert V.output_public_inputs(cv, pub[4], epk) == pub


# ---- Jubjub in big integers (affine, the complete twisted Edwards law with a = -1) ----
def _add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % Q
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, Q) % Q, (y1 * y2 + x1 * x2) * pow(1 - t, -1, Q) % Q)


def _mul(p, k):
    r = (0, 1)
    for bit in bin(k)[2:]:
        r = _add(r, r)
        if bit == "1":
            r = _add(r, p)
    return r


def _decode(b):
    try:
        return H.point_uv(b)
    except ValueError:
        return None


def batch_equation(items, zs):
    """masp_hip_redjubjub_verify_batch restated: every R, vk decodes, every S < r_J and
    [8](sum z_i R_i + z_i c_i vk_i - (sum z_i S_i) G_kind) = O, with z_i | 1 as the library takes it."""
    gens = [H.generator_uv(4), H.generator_uv(3)]
    acc, gsum = (0, 1), [0, 0]
    for (vk, sig, sighash, kind), z in zip(items, zs):
        R, P = _decode(sig[:32]), _decode(vk)
        s = int.from_bytes(sig[32:], "little")
        if R is None or P is None or s >= RJ:
            return False
        z |= 1
        c = RJS.h_star(sig[:32], vk + sighash)
        acc = _add(acc, _add(_mul(R, z), _mul(P, z * c % RJ)))
        gsum[kind] = (gsum[kind] + z * s) % RJ
    for g, s in zip(gens, gsum):
        acc = _add(acc, _mul(g, (-s) % RJ))
    return _mul(acc, 8) == (0, 1)


def _signed_items(rng, n):
    items = []
    for _ in range(n):
        kind = rng.randrange(2)
        g = H.point_bytes(*H.generator_uv(4 if kind == 0 else 3))
        sk = rng.randrange(1, RJ)
        vk = RJS.public_key(sk, g)
        sighash = bytes(rng.getrandbits(8) for _ in range(32))
        items.append((vk, RJS.sign(sk, vk + sighash, g, rng=lambda k: bytes(rng.getrandbits(8) for _ in range(k))), sighash, kind))
    return items


def _single(item):
    vk, sig, sighash, kind = item
    return RJS.verify(vk, vk + sighash, sig, H.point_bytes(*H.generator_uv(4 if kind == 0 else 3)))


def _non_canonical(enc):
    """the same point with v + q in the low 255 bits, or None if that does not fit"""
    v = int.from_bytes(enc, "little") & ((1 << 255) - 1)
    if v + Q >= 1 << 255:
        return None
    return ((v + Q) | (int.from_bytes(enc, "little") & (1 << 255))).to_bytes(32, "little")


def test_batch_equation_agrees_with_per_signature_verification():
    rng = random.Random(5)
    items = _signed_items(rng, 3)
    zs = [rng.getrandbits(128) for _ in items]
    assert all(_single(it) for it in items) and batch_equation(items, zs)
    cases = []
    vk, sig, sighash, kind = items[1]
    cases.append((vk, sig, bytes([sighash[0] ^ 1]) + sighash[1:], kind))                                   # wrong message
    s = int.from_bytes(sig[32:], "little")
    cases.append((vk, sig[:32] + (s + RJ).to_bytes(32, "little"), sighash, kind))                           # s >= r_J
    cases.append((vk, sig, sighash, 1 - kind))                                                                # wrong basepoint
    while True:                                                                                               # non-canonical R
        it = _signed_items(rng, 1)[0]
        bad_r = _non_canonical(it[1][:32])
        if bad_r is not None:
            cases.append((it[0], bad_r + it[1][32:], it[2], it[3]))
            break
    for bad in cases:
        batch = [items[0], bad, items[2]]
        assert not _single(bad)
        assert batch_equation(batch, zs) is False
