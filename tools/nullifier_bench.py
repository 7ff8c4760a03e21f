#!/usr/bin/env python3
"""Measures the note nullifiers: the GPU call (masp_hip_sapling_note_nullifiers, from arrays in host memory to status, cmu and nf in host
memory) with one and with eight lanes per note, next to the host call (masp_host_sapling_note_nullifiers) over the same notes on 16 host
threads (capped by the CPUs this process may use).

  python tools/nullifier_bench.py [--out profiles/nullifier_bench.json] [--quick] [--reps N] [--threads N] [--sizes a,b,...]

Per size (256, 4 096, 65 536 and 2^20 random valid notes): one warm-up call of each of the three, then `--reps` (at least five) timed
calls of each, alternating, so that the medians are of the same minutes of the same machine (host clock around a call that ends
synchronised).  upload_ms / kernel_ms / download_ms come from HIP events on the call's stream (masp_hip_note_nullifiers_last_timing).
The three results are compared by bytes once per size.  `crossover`: the smallest measured size from which one lane per note is not
slower than eight (None: eight lanes are faster at every size).  gpu_not_below_host is the expectation from 65 536 notes up, with the lane
width the call chooses by itself; it is printed and recorded, and it is not a test."""
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

POOL = 512      # distinct (diversifier, pk_d, nk) triples; the values, rseeds and positions are random per note


def random_notes(n, seed):
    """n valid notes as the eight arrays: half lead byte 1 with a canonical rcm, half lead byte 2"""
    import random
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    g = H.point_bytes(*H.generator_uv(1))
    ds, pks, nks = [], [], []
    while len(ds) < min(n, POOL):
        d = rng.randbytes(11)
        try:
            H.diversifier_base(d)
        except H.HostError:
            continue
        ds.append(d)
        pks.append(H.jubjub_mul(g, rng.randrange(1, H.JUBJUB_ORDER)))
        nks.append(H.jubjub_mul(g, rng.randrange(1, H.JUBJUB_ORDER)))
    pick = nrng.integers(0, len(ds), n)
    take = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, w)[pick].copy()
    leads = nrng.integers(1, 3, n, dtype=np.uint8)
    rseeds = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
    rseeds[leads == 1, 31] &= 0x07      # below 2^251 < r_J
    ident = np.tile(np.frombuffer(H.asset_identifier(b"benchmark"), np.uint8), (n, 1))
    return (ident, nrng.integers(0, 1 << 63, n, dtype=np.uint64), take(ds, 11), take(pks, 32), leads, rseeds, take(nks, 32),
            nrng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + 1)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def measure(ctx, n, reps, threads):
    arrays = random_notes(n, 1000 + n)

    def gpu(lanes):
        ctx.note_nullifiers_configure(lanes)
        try:
            return ctx.note_nullifiers(*arrays)
        finally:
            ctx.note_nullifiers_configure(0)

    host = lambda: H.note_nullifiers(*arrays, threads=threads)
    results = [timed(lambda: gpu(1))[1], timed(lambda: gpu(8))[1], timed(lambda: gpu(0))[1], timed(host)[1]]     # warm-up
    assert not results[0][0].any(), "every note is valid"
    for r in results[1:]:
        assert all((x == y).all() for x, y in zip(r, results[0])), "all sides give the same bytes"
    t = {1: [], 8: [], 0: [], "host": []}
    split = {1: [], 8: [], 0: []}
    for _ in range(reps):
        for lanes in (1, 8, 0):
            t[lanes].append(timed(lambda: gpu(lanes))[0])
            split[lanes].append(ctx.note_nullifiers_last_timing())
        t["host"].append(timed(host)[0])

    def side(key):
        med = statistics.median(t[key])
        out = {"seconds_median": med, "seconds_min": min(t[key]), "seconds_max": max(t[key]), "notes_per_second": n / med}
        if key != "host":
            i = t[key].index(med) if med in t[key] else 0
            out.update(upload_ms=split[key][i][0], kernel_ms=split[key][i][1], download_ms=split[key][i][2])
        return out

    r = {"notes": n, "reps": reps, "gpu_lanes_1": side(1), "gpu_lanes_8": side(8), "gpu_default": side(0),
         "host": dict(side("host"), threads=threads)}
    r["lanes_8_over_lanes_1"] = r["gpu_lanes_1"]["seconds_median"] / r["gpu_lanes_8"]["seconds_median"]
    r["kernels_lanes_8_over_lanes_1"] = r["gpu_lanes_1"]["kernel_ms"] / r["gpu_lanes_8"]["kernel_ms"]
    r["gpu_over_host"] = r["host"]["seconds_median"] / r["gpu_default"]["seconds_median"]
    r["gpu_not_below_host"] = r["gpu_default"]["seconds_median"] <= r["host"]["seconds_median"]
    r["expected_not_below_host"] = n >= 65536
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nullifier_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    ap.add_argument("--sizes", default=None, help="comma-separated note counts instead of the four (to bracket the crossover)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("nullifier_bench: no GPU (the host path alone is masp_host_sapling_note_nullifiers)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    ctx = masp_amd.Context(0)
    doc = {"tool": "tools/nullifier_bench.py" + (" --quick" if a.quick else ""), "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": []}
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes else [64, 1024] if a.quick else [256, 4096, 65536, 1 << 20]
    if a.sizes:
        doc["tool"] += " --sizes " + a.sizes
    for n in sizes:
        r = measure(ctx, n, reps, threads)
        doc["shapes"].append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    # by the kernels' own time (HIP events): the copies are the same for both widths and only blur the comparison at small sizes
    wide_wins = [r["notes"] for r in doc["shapes"] if r["kernels_lanes_8_over_lanes_1"] > 1.0]
    narrow = [r["notes"] for r in doc["shapes"] if r["kernels_lanes_8_over_lanes_1"] <= 1.0]
    doc["lanes_8_faster_at"] = wide_wins
    doc["crossover"] = min((n for n in narrow if all(w < n for w in wide_wins)), default=None)
    doc["gpu_not_below_host_where_expected"] = all(r["gpu_not_below_host"] for r in doc["shapes"] if r["expected_not_below_host"])
    print("eight lanes per note faster at: %s; one lane not slower from: %s" % (wide_wins, doc["crossover"]))
    print("expectation (from 65 536 notes up the GPU call is not slower than the host call on %d threads): %s"
          % (threads, "met" if doc["gpu_not_below_host_where_expected"] else "NOT met"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
