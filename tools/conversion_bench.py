#!/usr/bin/env python3
"""Measures the allowed conversions in batches: the GPU call (masp_hip_sapling_allowed_conversions, from arrays in host memory to status,
generator and cmu in host memory) with one and with eight lanes per conversion, next to the host twin (masp_host_allowed_conversions) over
the same conversions on 16 host threads (capped by the CPUs this process may use) and next to host.AllowedConversion one by one, the only
path there was (on at most 4 096 conversions).

  python tools/conversion_bench.py [--out profiles/conversion_bench.json] [--quick] [--reps N] [--threads N] [--sizes a,b,...]

Per size (256, 4 096, 65 536 and 2^20 conversions of three terms each, the shape of the reference's masp_proofs/benches/convert.rs:32-44:
(asset i, -(i + 1)), (asset i + 1, i + 1), (reward, i + 1)): one warm-up call of each side, then `--reps` (at least five) timed calls of
each, taking turns, so that the medians are of the same minutes of the same machine (host clock around a call that ends synchronised).
upload_ms / kernel_ms / download_ms come from HIP events on the call's stream (masp_hip_allowed_conversions_last_timing).  The sides'
results are compared by bytes once per size.  `sweep`: between the two measured sizes where one lane per conversion overtakes eight, the
powers of two in between, GPU only; `crossover`: the smallest size, measured or swept, from which one lane is not slower than eight by
the kernels' own time (None: eight lanes are faster at every size).  No speed-up is fixed in advance: the ratios are printed and recorded."""
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

POOL = 1024        # distinct "asset k" identifiers; a conversion takes two neighbours and the reward's
ONE_BY_ONE = 4096  # host.AllowedConversion one by one on at most this many


def conversions(n, seed):
    """n conversions of three terms as (offsets, identifiers, values) and the same as a list of sums for the one-by-one path"""
    rng = np.random.default_rng(seed)
    pool = [H.asset_identifier(b"asset %d" % k) for k in range(POOL + 1)]
    reward = H.asset_identifier(b"reward")
    table = np.frombuffer(b"".join(pool + [reward]), np.uint8).reshape(-1, 32)
    i = rng.integers(0, 1 << 31, n)
    ids = np.empty((n, 3, 32), np.uint8)
    ids[:, 0], ids[:, 1], ids[:, 2] = table[i % POOL], table[i % POOL + 1], table[POOL + 1]
    vals = np.zeros((n, 3, 2), np.int64)                    # an i128 as two little-endian words: the values fit the low one
    vals[:, 0, 0], vals[:, 1, 0], vals[:, 2, 0] = -(i + 1), i + 1, i + 1
    vals[:, 0, 1] = -1                                      # (the sign's extension)
    off = np.arange(n + 1, dtype=np.uint64) * 3
    sums = [[(pool[k % POOL], -(int(k) + 1)), (pool[k % POOL + 1], int(k) + 1), (reward, int(k) + 1)] for k in i[:ONE_BY_ONE]]
    return (off, ids.reshape(-1, 32), vals.view(np.uint8).reshape(-1, 16)), sums


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def gpu_call(ctx, arrays, lanes):
    ctx.allowed_conversions_configure(lanes)
    try:
        return ctx.allowed_conversions(*arrays)
    finally:
        ctx.allowed_conversions_configure(0)


def side(n, times, split=None):
    med = statistics.median(times)
    out = {"seconds_median": med, "seconds_min": min(times), "seconds_max": max(times), "conversions_per_second": n / med}
    if split is not None:
        i = times.index(med) if med in times else 0
        out.update(upload_ms=split[i][0], kernel_ms=split[i][1], download_ms=split[i][2])
    return out


def measure(ctx, n, reps, threads, gpu_only=False):
    arrays, sums = conversions(n, 1000 + n)
    first = gpu_call(ctx, arrays, 1)                                                # warm-up
    assert not first[0].any(), "every conversion is valid"
    for lanes in (8, 0):
        assert all((x == y).all() for x, y in zip(gpu_call(ctx, arrays, lanes), first)), "both widths give the same bytes"
    host = lambda: H.allowed_conversions(*arrays, threads=threads)
    one_by_one = lambda: [(c.generator, c.cmu()) for c in map(H.AllowedConversion, sums)]
    if not gpu_only:
        assert all((x == y).all() for x, y in zip(host(), first)), "the host twin gives the same bytes"
        assert one_by_one() == [(g.tobytes(), c.tobytes()) for g, c in zip(first[1][:len(sums)], first[2][:len(sums)])]
    t = {1: [], 8: [], 0: [], "host": [], "one": []}
    split = {1: [], 8: [], 0: []}
    for _ in range(reps):
        for lanes in (1, 8, 0):
            t[lanes].append(timed(lambda: gpu_call(ctx, arrays, lanes))[0])
            split[lanes].append(ctx.allowed_conversions_last_timing())
        if not gpu_only:
            t["host"].append(timed(host)[0])
            t["one"].append(timed(one_by_one)[0])
    r = {"conversions": n, "terms": 3 * n, "reps": reps, "gpu_lanes_1": side(n, t[1], split[1]), "gpu_lanes_8": side(n, t[8], split[8]),
         "gpu_default": side(n, t[0], split[0])}
    r["kernels_lanes_8_over_lanes_1"] = r["gpu_lanes_1"]["kernel_ms"] / r["gpu_lanes_8"]["kernel_ms"]
    if not gpu_only:
        r["host"] = dict(side(n, t["host"]), threads=threads)
        r["one_by_one"] = dict(side(len(sums), t["one"]), conversions=len(sums))
        r["gpu_over_host"] = r["host"]["seconds_median"] / r["gpu_default"]["seconds_median"]
        r["gpu_over_one_by_one"] = r["gpu_default"]["conversions_per_second"] / r["one_by_one"]["conversions_per_second"]
        r["host_microseconds_per_conversion_one_thread_one_by_one"] = 1e6 * r["one_by_one"]["seconds_median"] / len(sums)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conversion_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    ap.add_argument("--sizes", default=None, help="comma-separated conversion counts instead of the four")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("conversion_bench: no GPU (the host path alone is masp_host_allowed_conversions)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    ctx = masp_amd.Context(0)
    doc = {"tool": "tools/conversion_bench.py" + (" --quick" if a.quick else ""), "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": [], "sweep": []}
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes else [64, 1024] if a.quick else [256, 4096, 65536, 1 << 20]
    if a.sizes:
        doc["tool"] += " --sizes " + a.sizes
    for n in sizes:
        r = measure(ctx, n, reps, threads)
        doc["shapes"].append(r)
        print(json.dumps(r), flush=True)
    # by the kernels' own time (HIP events): the copies are the same for both widths and only blur the comparison at small sizes
    wide = lambda r: r["kernels_lanes_8_over_lanes_1"] > 1.0
    for lo, hi in zip(doc["shapes"], doc["shapes"][1:]):
        if wide(lo) and not wide(hi):
            n = 2 * lo["conversions"]
            while n < hi["conversions"]:
                r = measure(ctx, n, reps, threads, gpu_only=True)
                doc["sweep"].append(r)
                print(json.dumps(r), flush=True)
                n *= 2
    ctx.close()
    every = sorted(doc["shapes"] + doc["sweep"], key=lambda r: r["conversions"])
    wide_wins = [r["conversions"] for r in every if wide(r)]
    doc["lanes_8_faster_at"] = wide_wins
    doc["crossover"] = min((r["conversions"] for r in every if not wide(r) and all(w < r["conversions"] for w in wide_wins)), default=None)
    print("eight lanes per conversion faster at: %s; one lane not slower from: %s" % (wide_wins, doc["crossover"]))
    for r in doc["shapes"]:
        print("%8d conversions: the GPU call %.1f x the host twin on %d threads, %.1f x one by one (%.0f us a conversion on one thread)"
              % (r["conversions"], r["gpu_over_host"], threads, r["gpu_over_one_by_one"], r["host_microseconds_per_conversion_one_thread_one_by_one"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
