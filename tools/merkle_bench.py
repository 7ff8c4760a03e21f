#!/usr/bin/env python3
"""Measures the frozen commitment tree: the GPU call (masp_hip_merkle_tree_complete, from leaves in host memory to the root and 64 paths
in host memory, and once more with the whole node vector downloaded) next to the host path (masp_host_merkle_tree_complete) over the same
leaves on the CPUs this process may use.

  python tools/merkle_bench.py [--out profiles/merkle_bench.json] [--quick] [--reps N] [--threads N]
  python tools/merkle_bench.py --append [--out profiles/merkle_append_bench.json] [--quick] [--reps N]

Per size (2^10, 2^16, 2^20 random leaves) and per form (paths only / with the node vector): one warm-up call of each side, then `--reps`
(at least five) timed calls of each, alternating, so that the two medians are of the same minutes of the same machine (host clock around a
call that ends synchronised).  upload_ms / kernel_ms / download_ms come from HIP events on the tree's stream (masp_hip_merkle_last_timing).
Both sides' bytes are compared once per size.  gpu_not_below_host is the expectation at 2^16 and 2^20 leaves; at 2^10 the 32 dependent
levels of one hash each are all there is, and both numbers are recorded without one.

--append measures the incremental tree instead: a block of 2^16 leaves onto a CommitmentTree of 2^20 + 3 leaves with 1 024
IncrementalWitnesses, through advance(..., ctx) (masp_hip_merkle_tree_append), through advance(ctx=None) (the host twin) and, on a block of
2^10 leaves scaled to 2^16, through one-by-one append to the tree and to every witness, the reference's way.  Every timed call starts from
the same state, re-read from its bytes outside the clock, and the three end states are compared by bytes on the 2^10 block."""
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

N_PATHS = 64


def random_leaves(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] %= 0x73            # below the modulus, whose top byte is 0x73
    return a


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def measure(ctx, logn, reps, threads, with_nodes):
    n = 1 << logn
    leaves = random_leaves(n, 100 + logn)
    pos = sorted(np.random.default_rng(logn).choice(n, N_PATHS, replace=False).tolist())
    gpu = lambda: ctx.merkle_tree_complete(leaves, 0, pos, want_nodes=with_nodes)
    host = lambda: H.merkle_tree_complete(leaves, 0, pos, want_nodes=with_nodes, threads=threads)
    _, a = timed(gpu)                     # warm-up: code objects, buffers, the table
    _, b = timed(host)                    # tables
    assert a[1] == b[1] and (a[2] == b[2]).all() and (not with_nodes or (a[0] == b[0]).all()), "both sides give the same bytes"
    g, h, split = [], [], []
    for _ in range(reps):
        g.append(timed(gpu)[0])
        split.append(ctx.merkle_last_timing())
        h.append(timed(host)[0])
    gmed, hmed = statistics.median(g), statistics.median(h)
    i = g.index(gmed) if gmed in g else 0
    hashes = n - 1 + (32 - logn)
    return {"leaves": n, "paths": N_PATHS, "node_vector_downloaded": with_nodes, "hashes": hashes, "reps": reps,
            "gpu": {"seconds_median": gmed, "seconds_min": min(g), "seconds_max": max(g), "hashes_per_second": hashes / gmed,
                    "upload_ms": split[i][0], "kernel_ms": split[i][1], "download_ms": split[i][2]},
            "host": {"threads": threads, "seconds_median": hmed, "seconds_min": min(h), "seconds_max": max(h), "hashes_per_second": hashes / hmed},
            "gpu_over_host": hmed / gmed, "gpu_not_below_host": gmed <= hmed, "expected_not_below_host": logn >= 16}


def measure_append(ctx, reps, quick):
    from masp_amd import CommitmentTree, IncrementalWitness, advance
    size, block, small, n_wit = ((1 << 12) + 3, 1 << 10, 1 << 6, 64) if quick else ((1 << 20) + 3, 1 << 16, 1 << 10, 1024)
    leaves, nodes = random_leaves(size, 200), random_leaves(block, 201)
    tree = CommitmentTree.empty()
    track = sorted(np.random.default_rng(202).choice(size, n_wit, replace=False).tolist())
    witnesses = advance(tree, [], leaves, track, ctx)
    tree_ser, wit_ser = tree.write(), [w.write() for w in witnesses]

    def state():
        return CommitmentTree.read(tree_ser), [IncrementalWitness.read(x) for x in wit_ser]

    def run(c, count):
        t, ws = state()
        dt, _ = timed(lambda: advance(t, ws, nodes[:count], (), c))
        return dt, [t.write()] + [w.write() for w in ws]

    def one_by_one(count):
        t, ws = state()
        t0 = time.perf_counter()
        for x in nodes[:count]:
            x = x.tobytes()
            t.append(x)
            for w in ws:
                w.append(x)
        return time.perf_counter() - t0, [t.write()] + [w.write() for w in ws]

    t_one, end_one = one_by_one(small)
    assert run(ctx, small)[1] == end_one and run(None, small)[1] == end_one, "the three paths end in the same bytes"
    run(ctx, block)                           # warm-up
    g, h, split = [], [], []
    for _ in range(reps):
        g.append(run(ctx, block)[0])
        split.append(ctx.merkle_last_timing())
        h.append(run(None, block)[0])
    gmed, hmed = statistics.median(g), statistics.median(h)
    i = g.index(gmed) if gmed in g else 0
    return {"tree_leaves": size, "block": block, "witnesses": n_wit, "reps": reps,
            "gpu_advance": {"seconds_median": gmed, "seconds_min": min(g), "seconds_max": max(g), "upload_ms": split[i][0],
                            "kernel_ms": split[i][1], "download_ms": split[i][2]},
            "host_advance": {"threads": H.effective_cpus(), "seconds_median": hmed, "seconds_min": min(h), "seconds_max": max(h)},
            "one_by_one": {"block": small, "seconds": t_one, "seconds_scaled_to_block": t_one * block / small, "runs": 1},
            "gpu_over_host": hmed / gmed, "gpu_over_one_by_one_scaled": t_one * block / small / gmed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--append", action="store_true", help="the incremental tree: advance by a block, not the frozen tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("merkle_bench: no GPU (the host path alone is masp_host_merkle_tree_complete)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    a.out = a.out or os.path.join(ROOT, "profiles", "merkle_append_bench.json" if a.append else "merkle_bench.json")
    ctx = masp_amd.Context(0)
    doc = {"tool": "tools/merkle_bench.py" + (" --append" if a.append else "") + (" --quick" if a.quick else ""),
           "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": []}
    if a.append:
        doc["append"] = measure_append(ctx, reps, a.quick)
        del doc["shapes"]
        print(json.dumps(doc["append"]), flush=True)
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", a.out)
        return
    for logn in ((8, 12) if a.quick else (10, 16, 20)):
        for with_nodes in (False, True):
            r = measure(ctx, logn, reps, threads, with_nodes)
            doc["shapes"].append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    doc["gpu_not_below_host_where_expected"] = all(r["gpu_not_below_host"] for r in doc["shapes"] if r["expected_not_below_host"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
