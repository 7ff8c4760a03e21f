#!/usr/bin/env python3
"""RedJubjub batch verification and bundle validation on one GPU -> one JSON line.

    python tools/validate_bench.py [--sizes 1,64,1024,16384] [--bundles 8[,256,820]] [--distinct 32] [--reps 5] [--host-subset 64] [--out FILE]

redjubjub_verify_batch: wall time of Context.redjubjub_verify_batch at each n (median of --reps after one warm-up call), split into
`device_ms` = Context.jubjub_msm over the same 2n + 2 points and scalars (upload, the two kernels, read-back; the scalars are computed
beforehand in Python) and `host_ms` = the rest (H*, the coefficients mod r_J, packing the arguments).  `host_verify_ms_per_sig`:
masp_amd.redjubjub.verify one signature at a time on a subset.  Bundles: B bundles of two Spends, one Convert and two Outputs built as
tests/test_gpu_batch_validator.py builds them; `check_bundle_ms` per bundle (host) and `validate_ms` for all B (one signature batch and
three Groth16 batches on the GPU).  Next to them, in the same run and on the same bundles: `check_bundles_ms`, the wall time of ONE
BatchValidator.check_bundles call over all B (flattening, the device call, rebuilding the queues), its device call's three parts from HIP
events (`check_bundles_device_ms`: upload, kernels, download), `check_bundle_all_ms` = the B sequential check_bundle calls, and their ratio.
--bundles takes a list (8,256,820); --distinct D builds and proves D different bundles and repeats them up to B (neither path caches
anything, so a repeated bundle costs what a new one does; proving 820 bundles would only lengthen the run).  The line is also written to --out."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from masp_amd import host as H  # noqa: E402
from masp_amd import redjubjub as RJS  # noqa: E402
from masp_amd.hip import Context  # noqa: E402

RJ = H.JUBJUB_ORDER
GENS = [H.point_bytes(*H.generator_uv(4)), H.point_bytes(*H.generator_uv(3))]


def signatures(rng, n):
    items = []
    for i in range(n):
        kind = i % 2
        sk = rng.randrange(1, RJ)
        vk = RJS.public_key(sk, GENS[kind])
        sighash = bytes(rng.getrandbits(8) for _ in range(32))
        items.append((vk, RJS.sign(sk, vk + sighash, GENS[kind], rng=lambda k: bytes(rng.getrandbits(8) for _ in range(k))), sighash, kind))
    return items


def msm_arguments(items, z):
    """the 2n + 2 points and scalars masp_hip_redjubjub_verify_batch hands to the device"""
    pts, sc, acc = [], [], [0, 0]
    for i, (vk, sig, sighash, kind) in enumerate(items):
        zi = int.from_bytes(z[16 * i:16 * i + 16], "little") | 1
        pts.append(sig[:32])
        sc.append(zi)
        acc[kind] = (acc[kind] + zi * int.from_bytes(sig[32:], "little")) % RJ
    for i, (vk, sig, sighash, kind) in enumerate(items):
        zi = int.from_bytes(z[16 * i:16 * i + 16], "little") | 1
        pts.append(vk)
        sc.append(zi * RJS.h_star(sig[:32], vk + sighash) % RJ)
    return pts + GENS, sc + [(-acc[0]) % RJ, (-acc[1]) % RJ]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--bundles", default="8", help="numbers of bundles, comma-separated; 0 = none")
    ap.add_argument("--distinct", type=int, default=32, help="different bundles built and proved; repeated up to each B")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-subset", type=int, default=64)
    a = ap.parse_args()
    rng = random.Random(1)
    sizes = [int(x) for x in a.sizes.split(",")]
    items = signatures(rng, max(sizes))
    ctx = Context(0)
    res = {"metric": "redjubjub_validate", "redjubjub_verify_batch": {}}
    for n in sizes:
        batch = items[:n]
        z = bytes(rng.getrandbits(8) for _ in range(16 * n))
        total, ok = timed(lambda: ctx.redjubjub_verify_batch(batch, randomness=z), a.reps)
        pts, sc = msm_arguments(batch, z)
        dev, enc = timed(lambda: ctx.jubjub_msm(pts, sc), a.reps)
        assert ok is True and H.jubjub_mul(enc, 8) == H.JUBJUB_IDENTITY
        res["redjubjub_verify_batch"][str(n)] = {"total_ms": round(total, 3), "device_ms": round(dev, 3), "host_ms": round(total - dev, 3),
                                                 "us_per_sig": round(1e3 * total / n, 2)}
    sub = items[:a.host_subset]
    t0 = time.perf_counter()
    assert all(RJS.verify(vk, vk + sh, sig, GENS[k]) for vk, sig, sh, k in sub)
    res["host_verify_ms_per_sig"] = round((time.perf_counter() - t0) * 1e3 / len(sub), 3)
    res["host_verify_subset"] = len(sub)
    ctx.close()
    n_bundles = [int(x) for x in a.bundles.split(",") if int(x)]
    if n_bundles:
        from masp_amd import prover as P
        from masp_amd import verifier as V
        from test_gpu_batch_validator import _prepare_bundle
        lp = P.LocalTxProver.with_synthetic_parameters(seed=11)
        prepared = [_prepare_bundle(lp, rng) for _ in range(min(max(n_bundles), a.distinct))]
        jobs = [j for js, _ in prepared for j in js]
        proofs = lp.prove_prepared(jobs)
        lp._aux_give(jobs)
        distinct = [finish(proofs[5 * i:5 * i + 5]) for i, (_, finish) in enumerate(prepared)]
        vks = (lp._gpu_vk["spend"], lp._gpu_vk["convert"], lp._ctx.prepare_verifying_key(lp.parameters["output"]))
        entries = []
        for B in n_bundles:
            bundles = [distinct[i % len(distinct)] for i in range(B)]
            checks, vals, alls, parts = [], [], [], []
            for _ in range(a.reps + 1):
                bv = V.BatchValidator(lp._ctx)
                t0 = time.perf_counter()
                assert all(bv.check_bundle(b, s) for b, s, _ in bundles)
                t1 = time.perf_counter()
                assert bv.validate(*vks) is True
                t2 = time.perf_counter()
                checks.append((t1 - t0) * 1e3)
                vals.append((t2 - t1) * 1e3)
                bw = V.BatchValidator(lp._ctx)
                t0 = time.perf_counter()
                got = bw.check_bundles([b for b, _, _ in bundles], [s for _, s, _ in bundles])
                alls.append((time.perf_counter() - t0) * 1e3)
                parts.append(lp._ctx.check_bundles_last_timing())
                assert all(got) and (bw._signatures, bw._proofs, bw._bundles) == (bv._signatures, bv._proofs, bv._bundles)
            seq, one = statistics.median(checks[1:]), statistics.median(alls[1:])
            entries.append({"B": B, "distinct": len(distinct), "shape": "2 spends, 1 convert, 2 outputs", "check_bundle_ms": round(seq / B, 3),
                            "validate_ms": round(statistics.median(vals[1:]), 3), "check_bundle_all_ms": round(seq, 3),
                            "check_bundles_ms": round(one, 3), "check_bundles_device_ms": [round(statistics.median(p[k] for p in parts[1:]), 3) for k in range(3)],
                            "sequential_over_batched": round(seq / one, 2)})
        res["bundles"] = entries[0] if len(entries) == 1 else entries
        vks[2].close()
        lp.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
