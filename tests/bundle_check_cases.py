"""Host-shaped bundles for the tests of BatchValidator.check_bundles and masp_hip_sapling_check_bundles: points that decode, proofs
`Proof::read` accepts, nothing proved (as tests/test_validate_each_bookkeeping.py makes them), and one bundle per refusal reason."""
import functools

from masp_amd import host as H
from masp_amd import verifier as V
from test_validate_each_bookkeeping import StubContext, StubKey, point, sig  # noqa: F401  (re-exported)
from test_validate_each_bookkeeping import proof as _proof

Q, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
SMALL_ORDER = (Q - 1).to_bytes(32, "little")          # (0, -1): order 2
NOT_CANONICAL = Q.to_bytes(32, "little")              # v = r
ASSET = H.asset_identifier(b"bundle check")
ASSET_B = H.asset_identifier(b"another asset")


@functools.lru_cache(maxsize=None)
def proof(tag):
    return _proof(tag % 24)          # (two dozen different proofs do: every one costs three scalar multiplications in the oracle)


def bad_proof(tag):
    p = proof(tag)
    q = bytes([p[0] & 0x7f]) + p[1:]          # A without the compression flag
    assert not H.proof_read(q)
    return q


@functools.lru_cache(maxsize=None)
def asset_without_generator():
    for seed in range(256):
        ident = bytes([seed]) * 32
        try:
            H.asset_generator(ident)
        except ValueError:
            return ident
    raise AssertionError("every seed has a generator")


def bundle(tag, n=3, value_balance=((ASSET, 5), (ASSET_B, -7)), **bad):
    """n spends, n converts and n outputs; bad: spend_cv / spend_rk / spend_proof / convert_cv / convert_proof / output_cv / output_epk /
    output_proof = (index, replacement)"""
    def pick(what, i, good):
        at = bad.get(what)
        return at[1] if at is not None and at[0] == i else good
    base = 1000 * (tag + 1)
    spends = [V.SpendDescription(pick("spend_cv", i, point(base + i)), 5 + i, bytes([tag, i, 0xff, 0xc1]) * 8, pick("spend_rk", i, point(base + 100 + i)),
                                 pick("spend_proof", i, proof(9 * tag + i)), sig((7 * tag + i) % 256)) for i in range(n)]
    converts = [V.ConvertDescription(pick("convert_cv", i, point(base + 200 + i)), (6 + i).to_bytes(32, "little"), pick("convert_proof", i, proof(9 * tag + 3 + i)))
                for i in range(n)]
    outputs = [V.OutputDescription(pick("output_cv", i, point(base + 300 + i)), 7 + i, pick("output_epk", i, point(base + 400 + i)),
                                   pick("output_proof", i, proof(9 * tag + 6 + i))) for i in range(n)]
    return V.Bundle(spends, converts, outputs, list(value_balance), sig((7 * tag + 99) % 256))


# (reason, which field of which kind, replacement): each reason once per kind it applies to, at a first, a middle or a last description
REFUSALS = [
    (1, "spend_cv", NOT_CANONICAL), (1, "convert_cv", NOT_CANONICAL), (1, "output_cv", NOT_CANONICAL),
    (2, "spend_rk", NOT_CANONICAL), (2, "output_epk", NOT_CANONICAL),
    (3, "spend_proof", None), (3, "convert_proof", None), (3, "output_proof", None),
    (4, "spend_cv", SMALL_ORDER), (4, "convert_cv", SMALL_ORDER), (4, "output_cv", SMALL_ORDER),
    (5, "spend_rk", SMALL_ORDER), (5, "output_epk", SMALL_ORDER),
]


@functools.lru_cache(maxsize=None)
def refusal_list():
    """-> (bundles, sighashes, expected check_bundle verdicts, {bundle index: (reason, field, position)}): fine bundles, an empty one, one
    bundle per entry of REFUSALS, and the two value-balance refusals (bundle statuses 2 and 3)"""
    bundles, want, where = [bundle(0)], [True], {}
    for k, (reason, field, repl) in enumerate(REFUSALS):
        at = k % 3                                   # first, middle, last in turn
        tag = len(bundles)
        repl = bad_proof(9 * tag + at) if repl is None else repl
        where[tag] = (reason, field, at)
        bundles.append(bundle(tag, **{field: (at, repl)}))
        want.append(False)
    bundles.append(V.Bundle([], [], [], [], sig(200)))                                                  # empty
    want.append(True)
    bundles.append(bundle(len(bundles), value_balance=[(ASSET, 1), (ASSET_B, -(1 << 127)), (ASSET, 2)]))   # bundle status 2
    want.append(False)
    bundles.append(bundle(len(bundles), value_balance=[(ASSET, 1), (asset_without_generator(), 3)]))        # bundle status 3
    want.append(False)
    bundles.append(bundle(len(bundles), value_balance=[(ASSET, 4), (ASSET, 4), (ASSET, -8)]))               # duplicate identifiers
    want.append(True)
    bundles.append(bundle(len(bundles), n=1, value_balance=[]))
    want.append(True)
    return bundles, [bytes([k + 1]) * 32 for k in range(len(bundles))], want, where


def state(bv):
    return bv._bundles_added, bv._bundles, bv._signatures, bv._proofs
