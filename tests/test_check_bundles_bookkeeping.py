"""BatchValidator.check_bundles (masp_amd/verifier.py) leaves the validator exactly as check_bundle, bundle after bundle, does.  The
context is a stub whose check_bundles is the device code on the CPU (tests/bundle_check_shim.py, `Proof::read` by the host library); the
bundles are shaped on the host alone (tests/bundle_check_cases.py), one per refusal reason among them.  No GPU."""
import bundle_check_cases as K
import bundle_check_shim as S
from masp_amd import verifier as V


class Context(K.StubContext):
    """the per-item signature verifier of the bookkeeping tests, and check_bundles from the shim"""

    def __init__(self, bad_sigs=()):
        super().__init__(bad_sigs)
        self.bundle_calls = []

    def check_bundles(self, counts, spends, converts, outputs, balance):
        self.bundle_calls.append(len(counts))
        return S.check_bundles(counts, spends, converts, outputs, balance)


def _sequential(bundles, sighashes, ctx=None):
    bv = V.BatchValidator(ctx or K.StubContext())
    return bv, [bv.check_bundle(b, s) for b, s in zip(bundles, sighashes)]


def test_one_call_leaves_the_state_of_check_bundle_one_by_one():
    bundles, sighashes, want, _ = K.refusal_list()
    assert len(bundles) >= 12
    ctx = Context()
    bv = V.BatchValidator(ctx)
    got = bv.check_bundles(bundles, sighashes)
    ref, ref_got = _sequential(bundles, sighashes)
    assert ref_got == want                                         # (the list is what it says it is)
    assert got == want and K.state(bv) == K.state(ref)
    assert all(isinstance(x, int) for pis in bv._proofs["spend"][1] for x in pis)
    assert ctx.bundle_calls == [len(bundles)]                      # ONE device call


def test_a_refused_bundle_keeps_what_it_queued_before_and_nothing_after():
    bundles, sighashes, _, where = K.refusal_list()
    bv = V.BatchValidator(Context())
    bv.check_bundles(bundles, sighashes)
    marks = [start for _, start in bv._bundles] + [bv._queue_marks()]
    for k, (reason, field, at) in where.items():
        grown = [e - s for s, e in zip(marks[k], marks[k + 1])]    # signatures, spend, convert, output proofs of bundle k
        kind = field.split("_")[0]
        n = 3
        expect = {"spend": [at, at, 0, 0], "convert": [n, n, at, 0], "output": [n, n, n, at]}[kind]   # no binding signature either
        assert grown == expect, (k, reason, field, at, grown)


def test_a_mixed_sequence_gives_the_sequential_marks():
    bundles, sighashes, want, _ = K.refusal_list()
    bv = V.BatchValidator(Context())
    got = [bv.check_bundle(bundles[0], sighashes[0])] + bv.check_bundles(bundles[1:-1], sighashes[1:-1]) + [bv.check_bundle(bundles[-1], sighashes[-1])]
    ref, _ = _sequential(bundles, sighashes)
    assert got == want and K.state(bv) == K.state(ref)


def test_validate_each_gives_the_same_verdicts_on_both_paths():
    bundles, sighashes, want, _ = K.refusal_list()
    bad_sigs, bad_proofs = [bundles[0].spends[1].spend_auth_sig, bundles[-1].binding_sig], [bundles[-2].outputs[0].zkproof]
    a = V.BatchValidator(Context(bad_sigs))
    a.check_bundles(bundles, sighashes)
    b, _ = _sequential(bundles, sighashes, K.StubContext(bad_sigs))
    each = [v.validate_each(*[K.StubKey(bad_proofs) for _ in range(3)]) for v in (a, b)]
    assert each[0] == each[1] and len(each[0]) == len(bundles)
    assert each[0][0] is False and each[0][-1] is False and each[0][-2] is False       # the three bad items, each against its own bundle
    assert not any(v for v, w in zip(each[0], want) if not w) and any(each[0])
    assert a.validate(*[K.StubKey() for _ in range(3)]) is b.validate(*[K.StubKey() for _ in range(3)]) is False   # a bad signature is queued


def test_no_bundles():
    ctx = Context()
    bv = V.BatchValidator(ctx)
    assert bv.check_bundles([], []) == []
    assert bv._bundles_added is False and ctx.bundle_calls == []
    assert bv.validate(K.StubKey(), K.StubKey(), K.StubKey()) is True


def test_cases_decided_on_the_host():
    """a value outside i128 and fields of the wrong length get check_bundle's verdict and leave check_bundle's state"""
    fine = K.bundle(1)
    too_large = K.bundle(2, value_balance=[(K.ASSET, 1 << 127)])
    too_small = K.bundle(3, value_balance=[(K.ASSET, -(1 << 127) - 1)])
    short_proof = K.bundle(4, spend_proof=(1, K.proof(5)[:191]))
    long_nullifier = K.bundle(5)
    long_nullifier.spends[2].nullifier = bytes(33)
    bundles = [fine, too_large, short_proof, too_small, long_nullifier, K.bundle(6)]
    sighashes = [bytes([k]) * 32 for k in range(len(bundles))]
    ctx = Context()
    bv = V.BatchValidator(ctx)
    got = bv.check_bundles(bundles, sighashes)
    ref, want = _sequential(bundles, sighashes)
    assert got == want == [True, False, False, False, True, True]
    assert K.state(bv) == K.state(ref) and ctx.bundle_calls == [len(bundles)]
