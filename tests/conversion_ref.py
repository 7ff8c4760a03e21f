"""The allowed-conversion tests' other side and their shared inputs.  `reference` composes AllowedConversion::from and ::cmu
(masp_primitives/src/convert.rs:39-64, 86-118) from one-call primitives that the reference's vectors pin (tests/test_circuits.py): the asset
generator, a scalar multiplication, an addition and the Pedersen hash over the generator's 256 bits.  It goes through neither
masp_host_allowed_conversion nor the batch calls under test.  The cases (the edge list, a random batch) are computed once and shared by the
host, the device-header and the GPU file.  A conversion is a list of (identifier, value) terms, summed as given."""
import random

import numpy as np

from masp_amd import host as H

I128_MIN = -(1 << 127)
U64 = (1 << 64) - 1


def _le(k, n=32):
    return int(k).to_bytes(n, "little")


def has_generator(identifier):
    return H.load_library().masp_host_asset_generator(identifier, bytes(32)) == 0


def status_of(terms):
    """1: a term's identifier has no generator; else 2: a term's value is i128::MIN; whatever the order"""
    if any(not has_generator(i) for i, _ in terms):
        return 1
    if any(v == I128_MIN for _, v in terms):
        return 2
    return 0


def reference(terms, trace=False):
    """-> (status, generator, cmu[, repr(cm)]); the outputs are zeros where the status is not 0"""
    s = status_of(terms)
    if s:
        return (s, bytes(32), bytes(32)) + ((bytes(32),) if trace else ())
    gen = H.JUBJUB_IDENTITY
    for ident, v in terms:
        assert I128_MIN < v < (1 << 127)
        k = abs(v) & U64                                     # `abs as u64`: the low 64 bits
        gen = H.jubjub_add(gen, H.jubjub_mul(H.asset_generator(ident), _le(k)), subtract=v < 0)
    bits = [(gen[i // 8] >> (i % 8)) & 1 for i in range(256)]
    u, v = H.pedersen_hash(-1, bits)
    return (0, gen, _le(u)) + ((H.point_bytes(u, v),) if trace else ())


def _good_assets(n):
    out, k = [], 0
    while len(out) < n:
        try:
            out.append(H.asset_identifier(b"conversion asset %d" % k))
        except ValueError:
            pass
        k += 1
    return out


ASSETS = _good_assets(24)
A, B, C3 = ASSETS[:3]
BAD_ASSET = next(bytes([i]) * 32 for i in range(256) if not has_generator(bytes([i]) * 32))


def _bit255_value():
    """the smallest k for which [k] G_A's encoding has bit 255 set: the last chunk's one real bit"""
    g = H.asset_generator(A)
    return next(k for k in range(1, 200) if H.jubjub_mul(g, _le(k))[31] & 0x80)


def _many(n, seed):
    rng = random.Random(seed)
    return [(ASSETS[j % len(ASSETS)], rng.randrange(-(1 << 70), 1 << 70)) for j in range(n)]


def edge_conversions():
    """the issue's edge list as [(name, terms)]"""
    out = [("empty", []), ("zero", [(A, 0)])]
    for name, v in (("1", 1), ("2^63", 1 << 63), ("2^64-1", U64), ("2^64", 1 << 64), ("2^64+5", (1 << 64) + 5), ("2^127-1", (1 << 127) - 1)):
        out.append(("+" + name, [(A, v)]))
        out.append(("-" + name, [(A, -v)]))                  # (-(2^127 - 1) = -2^127 + 1 among them)
    out.append(("min alone", [(A, I128_MIN)]))
    out.append(("min next to a bad identifier", [(A, I128_MIN), (BAD_ASSET, 3)]))
    out.append(("a bad identifier next to min", [(BAD_ASSET, 3), (A, I128_MIN)]))
    out.append(("cancels", [(A, 5), (A, -5)]))
    three = [(A, 7), (B, -(1 << 65) - 9), (C3, 1 << 40)]
    out.append(("order 1", three))
    out.append(("order 2", three[::-1]))
    out.append(("bit 255", [(A, _bit255_value())]))
    five = [(ASSETS[j], 10 + j) for j in range(5)]
    for name, at in (("bad first", 0), ("bad middle", 2), ("bad last", 4)):
        out.append((name, [(BAD_ASSET, v) if j == at else (i, v) for j, (i, v) in enumerate(five)]))
    for n in (1, 2, 3, 17, 300):
        out.append(("%d terms" % n, _many(n, n)))
    return out


BATCH_SEED = 3   # chosen on the CPU by the reference alone: of random_batch(130, 3), see test_conversion_host.py for the counts it asserts


def random_batch(n, seed=BATCH_SEED):
    """n conversions of 0 to 5 terms: good identifiers and raw random ones (about half of which have no generator), values of every width,
    now and then i128::MIN"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        terms = []
        for _ in range(rng.choice((0, 1, 2, 3, 3, 3, 4, 5))):
            ident = rng.choice(ASSETS) if rng.random() < 0.85 else rng.randbytes(32)
            r = rng.random()
            if r < 0.06:
                v = I128_MIN
            elif r < 0.4:
                v = rng.randrange(-(1 << 20), 1 << 20)
            elif r < 0.7:
                v = rng.randrange(-(1 << 64), 1 << 64)
            else:
                v = rng.randrange(I128_MIN + 1, 1 << 127)
            terms.append((ident, v))
        out.append(terms)
    return out


def arrays(convs):
    """the three arrays of either allowed_conversions call: offsets uint64[n + 1], identifiers uint8[t, 32], values uint8[t, 16]"""
    off = np.zeros(len(convs) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in convs])
    ids = np.frombuffer(b"".join(i for c in convs for i, _ in c), np.uint8).reshape(-1, 32).copy()
    vals = np.frombuffer(b"".join(v.to_bytes(16, "little", signed=True) for c in convs for _, v in c), np.uint8).reshape(-1, 16).copy()
    return off, ids, vals


_cache = {}


def references(name):
    """(conversions, [reference(terms, trace=True)]) of "edges" or "random130", computed once"""
    if name not in _cache:
        convs = [t for _, t in edge_conversions()] if name == "edges" else random_batch(130)
        _cache[name] = (convs, [reference(t, trace=True) for t in convs])
    return _cache[name]


def edge(name):
    """the index of a named edge conversion"""
    return [n for n, _ in edge_conversions()].index(name)


def check(got, want):
    """got: (status, generators or None, cmus) arrays; want: [reference(terms)]"""
    status, gens, cmus = got
    assert status.tolist() == [w[0] for w in want]
    if gens is not None:
        assert [g.tobytes() for g in gens] == [w[1] for w in want]
    assert [c.tobytes() for c in cmus] == [w[2] for w in want]
