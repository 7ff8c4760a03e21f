#!/usr/bin/env python3
"""Measures the building of output descriptions without their proofs: the GPU call (masp_hip_sapling_build_outputs, from arrays in host
memory to status, cv, cmu, epk and the two ciphertexts in host memory) next to the host call (masp_host_sapling_build_outputs) over the
same outputs on 16 host threads (capped by the CPUs this process may use).

  python tools/output_build_bench.py [--out profiles/output_build_bench.json] [--quick] [--reps N] [--threads N] [--sizes a,b,...]
                                     [--chunks a,b,...]

Per size (256, 4 096, 65 536 and 2^20 random valid outputs: both lead bytes, random memos, one ovk in eight absent): one warm-up call of
either side, then `--reps` (at least five) timed calls of each, alternating, so that the medians are of the same minutes of the same
machine (host clock around a call that ends synchronised).  The host's calls stop early once they have taken `--host-seconds` in all at a
size (2^20 outputs are minutes a call on 16 threads): its "reps" says how many were timed, the warm-up call among them where it was the
only one.  upload_ms / kernel_ms / download_ms come from HIP events on the call's stream
(masp_hip_build_outputs_last_timing), summed over the call's chunks.  The two results are compared by bytes once per size.  `--chunks`: an
A/B of chunk sizes (masp_hip_build_outputs_configure) at the largest size, recorded under "chunk_ab".  What counts is outputs_per_second of
the GPU call against the host's, in one run; no speed-up is fixed in advance, and nothing here is a test."""
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

POOL = 512      # distinct (diversifier, pk_d) pairs; everything else is random per output


def random_outputs(n, seed):
    """n valid output plans as the twelve arrays, in the C ABI's order"""
    import random
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    g = H.point_bytes(*H.generator_uv(1))
    ds, pks = [], []
    while len(ds) < min(n, POOL):
        d = rng.randbytes(11)
        try:
            H.diversifier_base(d)
        except H.HostError:
            continue
        ds.append(d)
        pks.append(H.jubjub_mul(g, rng.randrange(1, H.JUBJUB_ORDER)))
    pick = nrng.integers(0, len(ds), n)
    take = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, w)[pick].copy()

    def scalars():      # below 2^251 < r_J
        s = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
        s[:, 31] &= 0x07
        return s

    leads = nrng.integers(1, 3, n, dtype=np.uint8)
    rseeds = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
    rseeds[leads == 1, 31] &= 0x07
    ident = np.tile(np.frombuffer(H.asset_identifier(b"benchmark"), np.uint8), (n, 1))
    flags = (nrng.integers(0, 8, n) != 0).astype(np.uint8)
    return (ident, nrng.integers(0, 1 << 63, n, dtype=np.uint64), take(ds, 11), take(pks, 32), leads, rseeds, scalars(), scalars(),
            nrng.integers(0, 256, (n, 512), dtype=np.uint8), nrng.integers(0, 256, (n, 32), dtype=np.uint8), flags,
            nrng.integers(0, 256, (n, 96), dtype=np.uint8))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def gpu_side(ctx, arrays, n, reps, chunk=0):
    """-> ({seconds_median, ..., upload_ms, kernel_ms, download_ms}, the call's result) with `chunk` outputs per chunk (0: the default)"""
    ctx.build_outputs_configure(chunk)
    try:
        result = ctx.build_outputs(*arrays)     # warm-up
        t, split = [], []
        for _ in range(reps):
            t.append(timed(lambda: ctx.build_outputs(*arrays))[0])
            split.append(ctx.build_outputs_last_timing())
    finally:
        ctx.build_outputs_configure(0)
    return summary(t, n, split), result


def summary(t, n, split=None):
    med = statistics.median(t)
    out = {"seconds_median": med, "seconds_min": min(t), "seconds_max": max(t), "outputs_per_second": n / med}
    if split:
        i = t.index(med) if med in t else 0
        out.update(upload_ms=split[i][0], kernel_ms=split[i][1], download_ms=split[i][2])
    return out


def measure(ctx, n, reps, threads, host_seconds):
    arrays = random_outputs(n, 2000 + n)
    host = lambda: H.build_outputs(*arrays, threads=threads)
    first, want = timed(host)     # warm-up
    assert not want[0].any(), "every output is valid"
    got = ctx.build_outputs(*arrays)
    assert all((x == y).all() for x, y in zip(got, want)), "both sides give the same bytes"
    tg, th, split = [], [], []
    for _ in range(reps):
        tg.append(timed(lambda: ctx.build_outputs(*arrays))[0])
        split.append(ctx.build_outputs_last_timing())
        if first + sum(th) < host_seconds:
            th.append(timed(host)[0])
    th = th or [first]
    r = {"outputs": n, "reps": reps, "gpu": summary(tg, n, split), "host": dict(summary(th, n), threads=threads, reps=len(th))}
    r["gpu_over_host"] = r["host"]["seconds_median"] / r["gpu"]["seconds_median"]
    return r, arrays, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_build_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--host-seconds", type=float, default=60.0, help="the host's timed calls at a size stop once they took this long in all")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    ap.add_argument("--sizes", default=None, help="comma-separated output counts instead of the four")
    ap.add_argument("--chunks", default=None, help="comma-separated chunk sizes for an A/B at the largest size (0: the default)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("output_build_bench: no GPU (the host path alone is masp_host_sapling_build_outputs)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    ctx = masp_amd.Context(0)
    doc = {"tool": "tools/output_build_bench.py" + (" --quick" if a.quick else ""), "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": []}
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes else [64, 1024] if a.quick else [256, 4096, 65536, 1 << 20]
    if a.sizes:
        doc["tool"] += " --sizes " + a.sizes
    arrays = want = None
    for n in sizes:
        r, arrays, want = measure(ctx, n, reps, threads, a.host_seconds)
        doc["shapes"].append(r)
        print(json.dumps(r), flush=True)
    if a.chunks:
        doc["tool"] += " --chunks " + a.chunks
        doc["chunk_ab"] = {"outputs": sizes[-1], "reps": reps, "chunks": []}
        for chunk in (int(x) for x in a.chunks.split(",")):
            side, got = gpu_side(ctx, arrays, sizes[-1], reps, chunk)
            assert all((x == y).all() for x, y in zip(got, want)), "the bytes do not depend on the chunk size"
            doc["chunk_ab"]["chunks"].append(dict(side, chunk_outputs=chunk))
            print(json.dumps(doc["chunk_ab"]["chunks"][-1]), flush=True)
    ctx.close()
    for r in doc["shapes"]:
        print("%8d outputs: GPU %10.0f outputs/s, host on %d threads %10.0f outputs/s, GPU over host %.2f"
              % (r["outputs"], r["gpu"]["outputs_per_second"], threads, r["host"]["outputs_per_second"], r["gpu_over_host"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
