"""Per-item verdicts against the batch calls and against the host, one item at a time:

    python tools/verify_each_bench.py [--sizes 1,64,4096] [--signatures 16384] [--reps 5] [--threads 16] [--out profiles/verify_each_bench.json]

Groth16: n real Spend proofs through GpuVerifyingKey.verify_each, through verify_batch and through the host's one-by-one path
(host.PreparedVerifyingKey.verify on --threads threads); RedJubjub: the same three for signatures.  The three alternate inside one run
(each, batch, host, each, ...), every figure is the median of --reps calls after one warm-up, and verify_each's time is split per
kernel from the HIP events of masp_hip_verify_each_last_timing (median per stage).  Asserted: every verdict is 1, and at the largest
size verify_each is faster than the host's one-by-one path.  The ratio to the batch call is recorded, not judged."""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import masp_amd                                   # noqa: E402
from masp_amd import host as H, workload as W     # noqa: E402
from masp_amd import redjubjub as RJS             # noqa: E402
from masp_amd.synthetic import toxic_waste        # noqa: E402

R, RJ = H.FR_MODULUS, H.JUBJUB_ORDER
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


def alternate(fns, reps):
    """fns: name -> callable; one warm-up round, then `reps` rounds in which the callables take turns -> name -> (median ms, last result)"""
    times, last = {k: [] for k in fns}, {}
    for rnd in range(reps + 1):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            last[name] = fn()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), last[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--signatures", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_each_bench.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    threads = max(1, min(a.threads, H.effective_cpus()))
    rng = random.Random(1)
    ctx = masp_amd.Context(0, batch_cap=128)
    cs = H.circuit("spend")[0]
    params = ctx.generate_parameters(cs, toxic_waste(3))
    ctx.load_circuit(0, params, cs)
    insts = W.instances("spend", min(256, max(sizes)))
    proofs, pub = [], []
    while len(proofs) < max(sizes):
        proofs += ctx.prove_batch([(0, i, x, rng.randrange(R), rng.randrange(R)) for i, x in insts])
        pub += [W.public_inputs(i) for i, _ in insts]
    hvk, gvk = H.PreparedVerifyingKey(params), ctx.prepare_verifying_key(params)
    res = {"metric": "verify_each", "reps": a.reps, "host_threads": threads, "groth16_spend": {}, "redjubjub": {}}
    with ThreadPoolExecutor(threads) as ex:
        for n in sizes:
            p, x = proofs[:n], pub[:n]
            split = []

            def each():
                out = gvk.verify_each(p, x)
                split.append(gvk.verify_each_last_timing())
                return out

            got = alternate({"each": each, "batch": lambda: gvk.verify_batch(p, x),
                             "host": lambda: list(ex.map(lambda k: hvk.verify(p[k], x[k]), range(n)))}, a.reps)
            assert got["each"][1] == [1] * n and got["batch"][1] is True and all(got["host"][1])
            stages = {k: round(statistics.median(s[k] for s in split[1:]), 3) for k in split[0]}
            e, b, h = (got[k][0] for k in ("each", "batch", "host"))
            res["groth16_spend"][str(n)] = {"verify_each_ms": round(e, 3), "verify_batch_ms": round(b, 3), "host_one_by_one_ms": round(h, 3),
                                            "each_over_batch": round(e / b, 2), "host_over_each": round(h / e, 2),
                                            "each_us_per_proof": round(1e3 * e / n, 2), "device_ms": stages}
            print("groth16 n = %5d   verify_each %9.2f ms   verify_batch %8.2f ms   host x%d %10.2f ms   %s" % (n, e, b, threads, h, stages), flush=True)
        n = max(sizes)
        assert res["groth16_spend"][str(n)]["host_over_each"] > 1, "verify_each is not faster than the host's one-by-one path at n = %d" % n
        if a.signatures:
            items = signatures(rng, a.signatures)
            single = lambda it: RJS.verify(it[0], it[0] + it[2], it[1], GENS[it[3]])
            got = alternate({"each": lambda: ctx.redjubjub_verify_each(items), "batch": lambda: ctx.redjubjub_verify_batch(items),
                             "host": lambda: list(ex.map(single, items))}, a.reps)
            assert all(got["each"][1]) and got["batch"][1] is True and all(got["host"][1])
            e, b, h = (got[k][0] for k in ("each", "batch", "host"))
            res["redjubjub"][str(a.signatures)] = {"verify_each_ms": round(e, 3), "verify_batch_ms": round(b, 3), "host_one_by_one_ms": round(h, 3),
                                                   "each_over_batch": round(e / b, 2), "host_over_each": round(h / e, 2),
                                                   "each_us_per_signature": round(1e3 * e / a.signatures, 2)}
            print("redjubjub n = %d   verify_each %.2f ms (H* on the host included)   verify_batch %.2f ms   host x%d %.2f ms"
                  % (a.signatures, e, b, threads, h), flush=True)
    gvk.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"metric": "verify_each", "out": os.path.relpath(a.out, ROOT)}))


if __name__ == "__main__":
    main()
