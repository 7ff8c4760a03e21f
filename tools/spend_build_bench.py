#!/usr/bin/env python3
"""Measures the building of spend descriptions without their proofs and the signing of them: the GPU calls
(masp_hip_sapling_build_spends: from arrays in host memory to status, cv, rk, nf, cmu and nk in host memory;
masp_hip_redjubjub_sign_batch: to status, vk and the signatures) next to the host calls (masp_host_sapling_build_spends,
masp_host_redjubjub_sign_batch) over the same items on 16 host threads (capped by the CPUs this process may use), and next to
redjubjub.sign, the Python signer, one signature after the other.

  python tools/spend_build_bench.py [--out profiles/spend_build_bench.json] [--quick] [--reps N] [--threads N] [--sizes a,b,...]

Per size (4 096 and 2^20 random valid items: both lead bytes, both kinds of signature): one warm-up call of either side, then `--reps` (at
least five) timed calls of each, alternating, so that the medians are of the same minutes of the same machine (host clock around a call
that ends synchronised).  The host's calls stop early once they have taken `--host-seconds` in all at a size: its "reps" says how many
were timed, the warm-up call among them where it was the only one.  upload_ms / kernel_ms / download_ms come from HIP events on the call's
stream (masp_hip_build_spends_last_timing, masp_hip_redjubjub_sign_last_timing), summed over the call's chunks; kernel_share is the
kernels' part of the three, which says whether a call is bound by its kernels or by its copies.  The two results are compared by bytes
once per size.  What counts is items_per_second of the GPU call against the host's, in one run; no speed-up is fixed in advance, and
nothing here is a test."""
import argparse
import datetime
import json
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import masp_amd  # noqa: E402
from masp_amd import host as H  # noqa: E402
from masp_amd import redjubjub as RJS  # noqa: E402

POOL = 512      # distinct (diversifier, pk_d, ak) triples; everything else is random per item


def scalars(nrng, n):      # below 2^251 < r_J
    s = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x07
    return s


def random_spends(n, seed):
    """n valid spend plans as the eleven arrays, in the C ABI's order"""
    import random
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    g, gs = H.point_bytes(*H.generator_uv(1)), H.point_bytes(*H.generator_uv(4))
    ds, pks, aks = [], [], []
    while len(ds) < min(n, POOL):
        d = rng.randbytes(11)
        try:
            H.diversifier_base(d)
        except H.HostError:
            continue
        ds.append(d)
        pks.append(H.jubjub_mul(g, rng.randrange(1, H.JUBJUB_ORDER)))
        aks.append(H.jubjub_mul(gs, rng.randrange(1, H.JUBJUB_ORDER)))
    pick = nrng.integers(0, len(ds), n)
    take = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, w)[pick].copy()
    leads = nrng.integers(1, 3, n, dtype=np.uint8)
    rseeds = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
    rseeds[leads == 1, 31] &= 0x07
    ident = np.tile(np.frombuffer(H.asset_identifier(b"benchmark"), np.uint8), (n, 1))
    return (ident, nrng.integers(0, 1 << 63, n, dtype=np.uint64), take(ds, 11), take(pks, 32), leads, rseeds, take(aks, 32), scalars(nrng, n),
            scalars(nrng, n), scalars(nrng, n), nrng.integers(0, 1 << 32, n, dtype=np.uint64))


def random_items(n, seed):
    """n valid signing items as the five arrays, in the C ABI's order"""
    nrng = np.random.default_rng(seed)
    return (scalars(nrng, n), scalars(nrng, n), nrng.integers(0, 256, (n, 32), dtype=np.uint8), nrng.integers(0, 2, n, dtype=np.uint8),
            nrng.integers(0, 256, (n, 80), dtype=np.uint8))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def summary(t, n, split=None):
    med = statistics.median(t)
    out = {"seconds_median": med, "seconds_min": min(t), "seconds_max": max(t), "items_per_second": n / med}
    if split:
        i = t.index(med) if med in t else 0
        out.update(upload_ms=split[i][0], kernel_ms=split[i][1], download_ms=split[i][2], kernel_share=split[i][1] / max(sum(split[i]), 1e-9))
    return out


def measure(name, gpu, gpu_timing, host, arrays, n, reps, threads, host_seconds):
    first, want = timed(host)     # warm-up
    assert not want[0].any(), "every item is valid"
    got = gpu()
    assert all((x == y).all() for x, y in zip(got, want)), "both sides give the same bytes"
    tg, th, split = [], [], []
    for _ in range(reps):
        tg.append(timed(gpu)[0])
        split.append(gpu_timing())
        if first + sum(th) < host_seconds:
            th.append(timed(host)[0])
    th = th or [first]
    r = {"call": name, "items": n, "reps": reps, "gpu": summary(tg, n, split), "host": dict(summary(th, n), threads=threads, reps=len(th))}
    r["gpu_over_host"] = r["host"]["seconds_median"] / r["gpu"]["seconds_median"]
    return r


def python_signer(n, seed):
    """redjubjub.sign, one signature after the other: n spend authorisation signatures with their rk"""
    sks, alphas, sighashes, _, _ = random_items(n, seed)
    g = H.point_bytes(*H.generator_uv(4))

    def run():
        for sk, al, m in zip(sks, alphas, sighashes):
            rsk = (int.from_bytes(sk.tobytes(), "little") + int.from_bytes(al.tobytes(), "little")) % H.JUBJUB_ORDER
            rk = RJS.public_key(rsk, g)
            RJS.sign(rsk, rk + m.tobytes(), g)
    t = timed(run)[0]
    return {"call": "redjubjub.sign", "items": n, "seconds": t, "items_per_second": n / t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spend_build_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--host-seconds", type=float, default=30.0, help="the host's timed calls at a size stop once they took this long in all")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    ap.add_argument("--sizes", default=None, help="comma-separated item counts instead of the two")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("spend_build_bench: no GPU (the host paths alone are masp_host_sapling_build_spends and masp_host_redjubjub_sign_batch)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    ctx = masp_amd.Context(0)
    doc = {"tool": "tools/spend_build_bench.py" + (" --quick" if a.quick else ""), "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": []}
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes else [64, 1024] if a.quick else [4096, 1 << 20]
    if a.sizes:
        doc["tool"] += " --sizes " + a.sizes
    for n in sizes:
        spends, items = random_spends(n, 3000 + n), random_items(n, 4000 + n)
        for r in (measure("build_spends", lambda: ctx.build_spends(*spends), ctx.build_spends_last_timing,
                          lambda: H.build_spends(*spends, threads=threads), spends, n, reps, threads, a.host_seconds),
                  measure("redjubjub_sign_batch", lambda: ctx.redjubjub_sign_batch(*items), ctx.redjubjub_sign_last_timing,
                          lambda: H.redjubjub_sign_batch(*items, threads=threads), items, n, reps, threads, a.host_seconds)):
            doc["shapes"].append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    doc["python_signer"] = python_signer(32 if a.quick else 256, 5000)
    print(json.dumps(doc["python_signer"]), flush=True)
    for r in doc["shapes"]:
        print("%22s %8d items: GPU %10.0f /s (kernels %.0f %% of the events' time), host on %d threads %10.0f /s, GPU over host %.2f"
              % (r["call"], r["items"], r["gpu"]["items_per_second"], 100 * r["gpu"]["kernel_share"], threads, r["host"]["items_per_second"],
                 r["gpu_over_host"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
