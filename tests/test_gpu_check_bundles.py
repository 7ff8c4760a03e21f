"""masp_hip_sapling_check_bundles and BatchValidator.check_bundles on the GPU: the C ABI item by item against the host references at
the lane and workgroup edges, the validator's state against check_bundle one by one, proved bundles end to end, arguments and limits.
Run with `-m gpu`."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import bundle_check_cases as K
import test_gpu_batch_validator as TB
import verify_cases as VC
from masp_amd import hip as HIP
from masp_amd import host as H
from masp_amd import prover as P
from masp_amd import verifier as V
from test_bundle_check_device_header import _flatten, _mirror_bvk

pytestmark = pytest.mark.gpu
N = VC.PREPARE_N                      # 150 descriptions per kind
EDGES = VC.FORCED_BAD                 # 0, 63, 64, 127, 128, 149


@pytest.fixture(scope="module")
def env():
    lp = P.LocalTxProver.with_synthetic_parameters(seed=11)
    rng = random.Random(12)
    prepared = [TB._prepare_bundle(lp, rng) for _ in range(8)]
    jobs = [j for js, _ in prepared for j in js]
    proofs = lp.prove_prepared(jobs)
    lp._aux_give(jobs)
    bundles = [finish(proofs[5 * i:5 * i + 5]) for i, (_, finish) in enumerate(prepared)]
    gpu_vks = (lp._gpu_vk["spend"], lp._gpu_vk["convert"], lp._ctx.prepare_verifying_key(lp.parameters["output"]))
    yield lp, bundles, gpu_vks
    gpu_vks[2].close()
    lp.close()


@pytest.fixture(scope="module")
def ctx(env):
    return env[0]._ctx


# ---- 3. the C ABI against the references, item by item ----
def _expected_status(cv, key, proof):
    if not V.decodes(cv):
        return 1
    if key is not None and not V.decodes(key):
        return 2
    if not H.proof_read(proof):
        return 3
    if V.is_small_order(cv):
        return 4
    if key is not None and V.is_small_order(key):
        return 5
    return 0


def _expected_bundle(b, statuses):
    """-> (bundle status, bvk) by the Python mirror"""
    if any(statuses):
        return 1, bytes(32)
    for asset, value in b.value_balance:
        if value == -(1 << 127):
            return 2, bytes(32)
        try:
            H.asset_generator(asset)
        except ValueError:
            return 3, bytes(32)
    return 0, _mirror_bvk(b)


def _edge_descriptions():
    """N spends, converts and outputs.  The proofs are verify_cases.prepare_batch()'s (every kind of encoding `Proof::read` refuses, the
    forced ones at EDGES): as they come for the spends, moved on by one for converts and outputs, whose points are bad at EDGES instead; the
    spends' points are bad next to the edges."""
    proofs = VC.prepare_batch()[0]
    negative_zero = ((H.FR_MODULUS - 1) | (1 << 255)).to_bytes(32, "little")
    # (which point, what it becomes) for the k-th forced index: the second point is the rk / epk
    two_points = [(0, K.SMALL_ORDER), (1, K.NOT_CANONICAL), (1, K.SMALL_ORDER), (0, K.SMALL_ORDER), (0, K.NOT_CANONICAL), (1, H.JUBJUB_IDENTITY)]
    one_point = [K.SMALL_ORDER, K.NOT_CANONICAL, K.SMALL_ORDER, negative_zero, H.JUBJUB_IDENTITY, K.SMALL_ORDER]
    near = (1, 62, 65, 126, 129, N - 2)
    spends, converts, outputs = [], [], []
    for i in range(N):
        pts = [K.point(5000 + i), K.point(6000 + i)]
        if i in near:
            which, bad = two_points[near.index(i)]
            pts[which] = bad
        spends.append(V.SpendDescription(pts[0], 11 + i, bytes([i, 0xee]) * 16, pts[1], proofs[i], K.sig(i)))
        pts, ccv = [K.point(7000 + i), K.point(8000 + i)], K.point(9000 + i)
        if i in EDGES:
            which, bad = two_points[EDGES.index(i)]
            pts[which] = bad
            ccv = one_point[EDGES.index(i)]
        cv, epk = pts
        converts.append(V.ConvertDescription(ccv, 12 + i, proofs[(i + 1) % N]))
        outputs.append(V.OutputDescription(cv, 13 + i, epk, proofs[(i + 1) % N]))
    return spends, converts, outputs


def _edge_bundles():
    """an empty bundle, one of 300 descriptions, fifty of one description for each kind, an empty bundle: 750 encodings in all"""
    spends, converts, outputs = _edge_descriptions()
    no_gen = K.asset_without_generator()
    bundles = [V.Bundle([], [], [], [], b"")]
    bundles.append(V.Bundle(spends[:100], converts[:100], outputs[:100], [(K.ASSET, 3)], b""))
    balances = [[], [(K.ASSET, 1)], [(K.ASSET, -(1 << 127))], [(no_gen, 2)], [(K.ASSET, 2), (K.ASSET, 2), (K.ASSET_B, -(1 << 64))], [(no_gen, -(1 << 127))],
                [(K.ASSET, (1 << 127) - 1), (K.ASSET_B, -((1 << 127) - 1))]]
    for i in range(100, N):
        bundles.append(V.Bundle([spends[i]], [], [], balances[i % 7], b""))
    for i in range(100, N):
        bundles.append(V.Bundle([], [converts[i]], [], balances[(i + 3) % 7], b""))
    for i in range(100, N):
        bundles.append(V.Bundle([], [], [outputs[i]], balances[(i + 5) % 7], b""))
    bundles.append(V.Bundle([], [], [], [], b""))
    assert (2 * N + N + 2 * N) % 64 != 0
    return bundles


def _compare_with_references(res, bundles):
    want = {"spend": [_expected_status(d.cv, d.rk, d.zkproof) for b in bundles for d in b.spends],
            "convert": [_expected_status(d.cv, None, d.zkproof) for b in bundles for d in b.converts],
            "output": [_expected_status(d.cv, d.ephemeral_key, d.zkproof) for b in bundles for d in b.outputs]}
    assert res.spend_status.tolist() == want["spend"]
    assert res.convert_status.tolist() == want["convert"]
    assert res.output_status.tolist() == want["output"]
    zero7, zero3, zero5 = [0] * 7, [0] * 3, [0] * 5
    rows = [V._rows_as_ints(a) for a in (res.spend_inputs, res.convert_inputs, res.output_inputs)]
    sp, cv, ou = ([d for b in bundles for d in getattr(b, k)] for k in ("spends", "converts", "outputs"))
    assert rows[0] == [zero7 if st else V.spend_public_inputs(d.cv, d.anchor, d.nullifier, d.rk) for d, st in zip(sp, want["spend"])]
    assert rows[1] == [zero3 if st else V.convert_public_inputs(d.cv, d.anchor) for d, st in zip(cv, want["convert"])]
    assert rows[2] == [zero5 if st else V.output_public_inputs(d.cv, d.cmu, d.ephemeral_key) for d, st in zip(ou, want["output"])]
    at = {"spend": 0, "convert": 0, "output": 0}
    for k, b in enumerate(bundles):
        sts = []
        for kind, items in (("spend", b.spends), ("convert", b.converts), ("output", b.outputs)):
            sts += want[kind][at[kind]:at[kind] + len(items)]
            at[kind] += len(items)
        st, bvk = _expected_bundle(b, sts)
        assert (int(res.bundle_status[k]), res.bvk[k].tobytes()) == (st, bvk), k
    return want


def test_c_abi_item_by_item_at_the_lane_edges(ctx):
    bundles = _edge_bundles()
    res = ctx.check_bundles(*_flatten(bundles))
    want = _compare_with_references(res, bundles)
    assert set(want["spend"]) == set(want["output"]) == {0, 1, 2, 3, 4, 5} and set(want["convert"]) == {0, 1, 3, 4}
    assert all(want["spend"][i] == 3 for i in EDGES) and all(want["convert"][i] in (1, 3, 4) for i in EDGES) and all(want["output"][i] for i in EDGES)
    assert set(res.bundle_status.tolist()) == {0, 1, 2, 3}
    assert res.bundle_status[0] == res.bundle_status[-1] == 0 and res.bvk[0].tobytes() == res.bvk[-1].tobytes() == H.JUBJUB_IDENTITY


def test_a_valid_bundle_longer_than_a_workgroup(ctx):
    """100 spends, 100 converts and 100 outputs that are all accepted: bvk is the sum over 300 descriptions and three terms, by one lane"""
    ok = [p for i, p in enumerate(VC.prepare_batch()[0]) if i not in VC.prepare_batch()[2]]
    sp = [V.SpendDescription(K.point(100 + i), i, bytes([i]) * 32, K.point(300 + i), ok[i % len(ok)], K.sig(i)) for i in range(100)]
    cv = [V.ConvertDescription(K.point(500 + i), i, ok[(i + 1) % len(ok)]) for i in range(100)]
    ou = [V.OutputDescription(K.point(700 + i), i, K.point(900 + i), ok[(i + 2) % len(ok)]) for i in range(100)]
    bundles = [V.Bundle(sp[:1], [], [], [], b""), V.Bundle(sp[1:], cv, ou, [(K.ASSET, 9), (K.ASSET_B, -4), (K.ASSET, -(1 << 100))], b""), V.Bundle([], [], [], [], b"")]
    res = ctx.check_bundles(*_flatten(bundles))
    want = _compare_with_references(res, bundles)
    assert not any(want["spend"] + want["convert"] + want["output"]) and res.bundle_status.tolist() == [0, 0, 0]


# ---- 4. the validator's state, as on the CPU ----
def test_validator_state_equals_check_bundle_one_by_one(ctx):
    bundles, sighashes, want, _ = K.refusal_list()
    bv = V.BatchValidator(ctx)
    got = bv.check_bundles(bundles, sighashes)
    ref = V.BatchValidator(ctx)
    assert [ref.check_bundle(b, s) for b, s in zip(bundles, sighashes)] == want
    assert got == want and K.state(bv) == K.state(ref)
    mixed = V.BatchValidator(ctx)
    got = [mixed.check_bundle(bundles[0], sighashes[0])] + mixed.check_bundles(bundles[1:-1], sighashes[1:-1]) + [mixed.check_bundle(bundles[-1], sighashes[-1])]
    assert got == want and K.state(mixed) == K.state(ref)
    keys = [K.StubKey([bundles[-2].outputs[0].zkproof]) for _ in range(3)]
    assert bv.validate_each(*keys) == ref.validate_each(*keys)          # real signature verdicts (all bad: nothing was signed), stub keys
    empty = V.BatchValidator(ctx)
    assert empty.check_bundles([], []) == [] and empty._bundles_added is False and empty.validate(*keys) is True


# ---- 5. end to end with proved bundles ----
def test_proved_bundles_end_to_end(env):
    lp, bundles, gpu_vks = env
    bv = V.BatchValidator(lp._ctx)
    assert bv.check_bundles([b for b, _, _ in bundles], [s for _, s, _ in bundles]) == [True] * 8
    assert bv.validate(*gpu_vks) is True
    assert bv.validate_each(*gpu_vks) == [True] * 8


def test_one_thing_changed_in_one_bundle(env):
    lp, bundles, gpu_vks = env
    muts, sighash = TB._mutations(bundles)
    good = [(b, s) for b, s, _ in bundles[2:5]]

    def run(name):
        items = good[:1] + [(muts[name][0], sighash)] + good[1:]
        bv = V.BatchValidator(lp._ctx)
        return bv, bv.check_bundles([b for b, _ in items], [s for _, s in items])

    bv, checks = run("flipped spend-auth signature")
    assert checks == [True] * 4 and bv.validate(*gpu_vks) is False and bv.validate_each(*gpu_vks) == [True, False, True, True]
    bv, checks = run("small-order cv")
    assert checks == [True, False, True, True]                            # refused here; its neighbours are unaffected
    assert bv.validate_each(*gpu_vks) == [True, False, True, True]
    bv, checks = run("value balance off by one")
    assert checks == [True] * 4                                           # a valid bvk of another balance: the binding signature fails
    assert bv.validate(*gpu_vks) is False and bv.validate_each(*gpu_vks) == [True, False, True, True]


# ---- 6. arguments and limits ----
def _raw_call(ctx, s):
    return HIP.load_library().masp_hip_sapling_check_bundles(ctx._h, C.byref(s))


def test_zero_bundles(ctx):
    res = ctx.check_bundles([], [b""] * 5, [b""] * 3, [b""] * 4, [b""] * 2)
    assert res.bvk.shape == (0, 32) and res.bundle_status.size == 0
    assert _raw_call(ctx, HIP.BundleCheckStruct()) == 0                    # nothing is read: every pointer is NULL


def test_bad_arguments_write_nothing_and_leave_the_context_usable(ctx):
    bundles = [K.bundle(1), K.bundle(2)]
    flat = list(_flatten(bundles))
    good = ctx.check_bundles(*flat)
    for counts in ([(3, 3, 3, 2), (3, 3, 2, 2)], [(3, 3, 3, 2), (3, 3, 3, 3)], [(4, 3, 3, 2), (3, 3, 3, 2)]):
        s, res, keep = HIP.bundle_check_args(counts, *flat[1:])
        for a in res:
            a.fill(0xaa)
        assert _raw_call(ctx, s) == 1
        assert all((a == 0xaa).all() for a in res)
        with pytest.raises(HIP.MaspHipError) as e:
            ctx.check_bundles(counts, *flat[1:])
        assert e.value.code == 1
    for field in ("counts", "spend_rk", "convert_zkproof", "output_cmu", "balance_value", "spend_status", "output_inputs", "bvk", "bundle_status"):
        s, res, keep = HIP.bundle_check_args(*flat)
        setattr(s, field, None)
        for a in res:
            a.fill(0xaa)
        assert _raw_call(ctx, s) == 1, field
        assert all((a == 0xaa).all() for a in res), field
    again = ctx.check_bundles(*flat)
    assert all((a == b).all() for a, b in zip(good, again)) and good.bundle_status.tolist() == [0, 0]
    assert all(t >= 0 for t in ctx.check_bundles_last_timing()) and ctx.check_bundles_last_timing()[1] > 0


def test_two_identical_calls_return_identical_bytes(ctx):
    flat = _flatten(K.refusal_list()[0])
    a, b = ctx.check_bundles(*flat), ctx.check_bundles(*flat)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_threads_on_one_context_and_no_new_stream(ctx):
    n_streams = ctx.stream_concurrency()[0]
    bundles, sighashes, want, _ = K.refusal_list()
    lists = {"forward": (bundles, sighashes, want), "backward": (bundles[::-1], sighashes[::-1], want[::-1])}
    single = {}
    for name, (bs, ss, _) in lists.items():
        bv = V.BatchValidator(ctx)
        bv.check_bundles(bs, ss)
        single[name] = K.state(bv)
    results = {}

    def run(name, rounds=3):
        bs, ss, w = lists[name]
        out = []
        for _ in range(rounds):
            bv = V.BatchValidator(ctx)
            out.append(bv.check_bundles(bs, ss) == w and K.state(bv) == single[name])
        results[name] = out

    threads = [threading.Thread(target=run, args=(name,)) for name in lists]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == {"forward": [True] * 3, "backward": [True] * 3}
    assert ctx.stream_concurrency()[0] == n_streams
