#!/usr/bin/env python3
"""Measures batch trial decryption of Sapling notes: trials per second of the GPU call (masp_hip_sapling_trial_decrypt, from host
memory to the sorted hit list, plus the host's finishing of the hits) next to the host batch path on the CPUs this process may use.

  python tools/note_scan_bench.py [--out profiles/note_scan_bench.json] [--quick] [--only N_OUT,N_IVK]
  python tools/note_scan_bench.py --compact [--out profiles/note_scan_compact_bench.json] [--quick]

Per configuration: one warm-up call, then `--reps` timed calls (host clock around a call that ends synchronised); the median is
reported, with the spread.  upload_ms / kernel_ms come from HIP events on the scan's streams (masp_hip_note_scan_last_timing),
finish_ms is the host's second half (masp_host_sapling_finish_note_decryption over the hits).  Every epk decodes (4 096 distinct
points, tiled: a trial's cost does not depend on the point), the ciphertexts are random bytes, and 64 notes are planted per call so
that the hit path runs.  The A/B section times the two digit recodings and the two inversions alternately in one process.
--only runs one configuration once after its warm-up, for a profiler's kernel trace.

--compact measures the compact (ZIP 307) scan (masp_hip_sapling_compact_trial_decrypt: the whole check on the device, nothing to finish on
the host) on the same shapes and inputs, of which it takes enc[:, :84], and the FULL scan in the same run: the two calls alternate, so
that their medians are of the same minutes of the same machine.  Per shape: trials/s of both, upload ms and the kernel ms of stage 1 and
stage 2 (masp_hip_note_scan_compact_last_timing), candidates per call, and whether the compact median is at least the full one's less the
full scan's own spread (its max - min of the run).  The host side is masp_host_sapling_try_compact_note_decryption_batch."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import masp_amd  # noqa: E402
from masp_amd import host as H  # noqa: E402
from masp_amd import note_encryption as NE  # noqa: E402

RJ = H.JUBJUB_ORDER
ASSET = H.asset_identifier(b"note scan bench")


def recipient(ivk, rng):
    while True:
        d = rng.randbytes(11)
        try:
            gd = H.diversifier_base(d)
        except H.HostError:
            continue
        return NE.PaymentAddress(d, H.jubjub_mul(gd, ivk.to_bytes(32, "little")))


def make_inputs(n_out, ivks_int, seed, n_planted=64):
    rng = random.Random(seed)
    nprng = np.random.default_rng(seed)
    base = H.diversifier_base(recipient(1, rng).diversifier)
    pool = np.frombuffer(b"".join(H.jubjub_mul(base, rng.randrange(1, RJ).to_bytes(32, "little")) for _ in range(4096)), np.uint8).reshape(-1, 32)
    epks = np.ascontiguousarray(np.tile(pool, ((n_out + 4095) // 4096, 1))[:n_out])
    cmus = nprng.integers(0, 256, (n_out, 32), dtype=np.uint8)
    encs = nprng.integers(0, 256, (n_out, 612), dtype=np.uint8)
    places = rng.sample(range(n_out), min(n_planted, n_out))
    for j, o in enumerate(places):
        ivk = ivks_int[j % len(ivks_int)]
        to = recipient(ivk, rng)
        note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(2, rng.randbytes(32)))
        out = NE.sapling_note_encrypt(note, to)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
    return epks, cmus, encs, sorted(places)


def gpu_call(ctx, ivks, epks, cmus, encs):
    """one whole scan: the ABI call, then the host's finishing of its hits -> (call s, finish s, upload ms, kernel ms, notes found)"""
    t0 = time.perf_counter()
    _, ho, hi, hk = ctx.sapling_trial_decrypt(ivks, epks, encs, hit_capacity=4096)
    t1 = time.perf_counter()
    found = 0
    for o, k, key in zip(ho.tolist(), hi.tolist(), hk):
        if H.sapling_finish_note_decryption(key.tobytes(), ivks[32 * k:32 * k + 32], epks[o].tobytes(), cmus[o].tobytes(), encs[o].tobytes(), 2):
            found += 1
    t2 = time.perf_counter()
    up, kern = ctx.note_scan_last_timing()
    return t1 - t0, t2 - t1, up, kern, found


def measure(ctx, n_out, n_ivk, reps, seed):
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = b"".join(k.to_bytes(32, "little") for k in ivks_int)
    epks, cmus, encs, places = make_inputs(n_out, ivks_int, seed)
    gpu_call(ctx, ivks, epks, cmus, encs)    # warm-up: code objects, buffers
    runs = [gpu_call(ctx, ivks, epks, cmus, encs) for _ in range(reps)]
    assert all(r[4] == len(places) for r in runs), (runs, len(places))
    total = [r[0] + r[1] for r in runs]
    med = statistics.median(total)
    i = total.index(med) if med in total else 0
    trials = n_out * n_ivk
    return {"outputs": n_out, "ivks": n_ivk, "trials": trials, "reps": reps, "seconds_median": med, "seconds_min": min(total), "seconds_max": max(total),
            "trials_per_second": trials / med, "call_ms": runs[i][0] * 1e3, "finish_ms": runs[i][1] * 1e3, "upload_ms": runs[i][2],
            "kernel_ms": runs[i][3], "notes_found": runs[i][4], "input_megabytes": n_out * 644 / 1e6}


def compact_call(ctx, ivks, epks, cmus, enc84):
    """one whole compact scan: the hits are final -> (call s, upload ms, stage 1 ms, stage 2 ms, notes found, candidates)"""
    t0 = time.perf_counter()
    _, ho, hi, hp, hk, cand = ctx.sapling_compact_trial_decrypt(ivks, epks, cmus, enc84, 2, hit_capacity=4096)
    t1 = time.perf_counter()
    up, k1, k2 = ctx.note_scan_compact_last_timing()
    return t1 - t0, up, k1, k2, len(set(ho.tolist())), cand


def measure_compact(ctx, n_out, n_ivk, reps, seed):
    """the compact and the full scan of the same inputs, alternating"""
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = b"".join(k.to_bytes(32, "little") for k in ivks_int)
    epks, cmus, encs, places = make_inputs(n_out, ivks_int, seed)
    enc84 = np.ascontiguousarray(encs[:, :84])
    compact_call(ctx, ivks, epks, cmus, enc84)    # warm-up: code objects, buffers, the Pedersen table
    gpu_call(ctx, ivks, epks, cmus, encs)
    cr, fr = [], []
    for _ in range(reps):
        cr.append(compact_call(ctx, ivks, epks, cmus, enc84))
        fr.append(gpu_call(ctx, ivks, epks, cmus, encs))
    assert all(r[4] == len(places) for r in cr) and all(r[4] == len(places) for r in fr), (cr, fr, len(places))
    ct, ft = [r[0] for r in cr], [r[0] + r[1] for r in fr]
    cmed, fmed = statistics.median(ct), statistics.median(ft)
    i = ct.index(cmed) if cmed in ct else 0
    trials = n_out * n_ivk
    return {"outputs": n_out, "ivks": n_ivk, "trials": trials, "reps": reps,
            "compact": {"seconds_median": cmed, "seconds_min": min(ct), "seconds_max": max(ct), "trials_per_second": trials / cmed,
                        "upload_ms": cr[i][1], "stage1_ms": cr[i][2], "stage2_ms": cr[i][3], "kernel_ms": cr[i][2] + cr[i][3],
                        "candidates": cr[i][5], "notes_found": cr[i][4], "input_megabytes": n_out * 148 / 1e6},
            "full": {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft), "trials_per_second": trials / fmed,
                     "upload_ms": fr[0][2], "kernel_ms": fr[0][3], "input_megabytes": n_out * 644 / 1e6},
            "compact_over_full": fmed / cmed,
            "compact_not_below_full_within_its_spread": cmed <= fmed + (max(ft) - min(ft))}


def host_measure_compact(n_out, n_ivk, threads, seed):
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ivks_int), np.uint8)
    epks, cmus, encs, places = make_inputs(n_out, ivks_int, seed)
    enc84 = np.ascontiguousarray(encs[:, :84])
    H.sapling_try_compact_note_decryption_batch(ivks, epks[:256], cmus[:256], enc84[:256], threads=threads)   # tables, threads
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        hit, _, _, cand = H.sapling_try_compact_note_decryption_batch(ivks, epks, cmus, enc84, threads=threads)
        secs.append(time.perf_counter() - t0)
    assert [i for i, k in enumerate(hit.tolist()) if k >= 0] == places
    med = statistics.median(secs)
    return {"outputs": n_out, "ivks": n_ivk, "trials": n_out * n_ivk, "threads": threads, "seconds_median": med, "seconds_min": min(secs),
            "seconds_max": max(secs), "trials_per_second": n_out * n_ivk / med, "candidates": cand}


def main_compact(a, ctx, torch):
    configs = [(4096, 1), (4096, 4)] if a.quick else [(65536, 1), (65536, 4), (65536, 16), (1 << 20, 1)]
    threads = H.effective_cpus()
    doc = {"tool": "tools/note_scan_bench.py --compact", "device": torch.cuda.get_device_name(0), "host_threads": threads, "gpu": [], "host": []}
    for n_out, n_ivk in configs:
        r = measure_compact(ctx, n_out, n_ivk, a.reps, 7)
        doc["gpu"].append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    for n_out, n_ivk in ([(1024, 1)] if a.quick else [(32768, 1), (8192, 4)]):
        r = host_measure_compact(n_out, n_ivk, threads, 9)
        doc["host"].append(r)
        print(json.dumps(r), flush=True)
    doc["gpu_over_host"] = doc["gpu"][-1 if a.quick else 1]["compact"]["trials_per_second"] / doc["host"][-1]["trials_per_second"]
    out = a.out or os.path.join(ROOT, "profiles", "note_scan_compact_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


def ab(ctx, n_out, n_ivk, rounds, seed):
    """kernel_ms of the four settings, alternating, `rounds` times each"""
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = b"".join(k.to_bytes(32, "little") for k in ivks_int)
    epks, cmus, encs, _ = make_inputs(n_out, ivks_int, seed)
    settings = [(0, 0), (1, 0), (0, 1), (1, 1)]
    ms = {s: [] for s in settings}
    try:
        for r in range(rounds + 1):
            for s in settings:
                ctx.note_scan_configure(*s)
                k = gpu_call(ctx, ivks, epks, cmus, encs)[3]
                if r:                       # round 0 warms up
                    ms[s].append(k)
    finally:
        ctx.note_scan_configure(1, 0)      # the defaults
    return [{"signed_digits": s[0], "inversion": ("divsteps", "binary_gcd")[s[1]], "kernel_ms": ms[s], "kernel_ms_median": statistics.median(ms[s])}
            for s in settings]


def host_measure(n_out, n_ivk, threads, seed):
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, RJ) for _ in range(n_ivk)]
    ivks = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ivks_int), np.uint8)
    epks, cmus, encs, places = make_inputs(n_out, ivks_int, seed)
    H.sapling_try_note_decryption_batch(ivks, epks[:256], cmus[:256], encs[:256], threads=threads)   # tables, threads
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        hit, _, _ = H.sapling_try_note_decryption_batch(ivks, epks, cmus, encs, threads=threads)
        secs.append(time.perf_counter() - t0)
    assert [i for i, k in enumerate(hit.tolist()) if k >= 0] == places
    med = statistics.median(secs)
    return {"outputs": n_out, "ivks": n_ivk, "trials": n_out * n_ivk, "threads": threads, "seconds_median": med, "seconds_min": min(secs),
            "seconds_max": max(secs), "trials_per_second": n_out * n_ivk / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/note_scan_bench.json, with --compact profiles/note_scan_compact_bench.json")
    ap.add_argument("--compact", action="store_true", help="the compact (ZIP 307) scan next to the full one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    ap.add_argument("--only", default=None, help="N_OUT,N_IVK: that configuration alone, one call after the warm-up (for a kernel trace)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("note_scan_bench: no GPU (there is no CPU fallback for the scan)")
    ctx = masp_amd.Context(0)
    if a.compact:
        main_compact(a, ctx, torch)
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "note_scan_bench.json")
    if a.only:
        n_out, n_ivk = (int(x) for x in a.only.split(","))
        print(json.dumps(measure(ctx, n_out, n_ivk, 1, 7)))
        ctx.close()
        return
    configs = [(4096, 1), (4096, 4)] if a.quick else [(65536, 1), (65536, 4), (65536, 16), (1 << 20, 1)]
    threads = H.effective_cpus()
    doc = {"tool": "tools/note_scan_bench.py", "device": torch.cuda.get_device_name(0), "host_threads": threads, "gpu": [], "host": [], "ab": []}
    for n_out, n_ivk in configs:
        r = measure(ctx, n_out, n_ivk, a.reps, 7)
        doc["gpu"].append(r)
        print(json.dumps(r), flush=True)
    doc["ab"] = ab(ctx, 4096 if a.quick else 65536, 4, 2 if a.quick else 4, 8)
    print(json.dumps(doc["ab"]), flush=True)
    ctx.close()
    for n_out, n_ivk in ([(1024, 1)] if a.quick else [(32768, 1), (8192, 4)]):
        r = host_measure(n_out, n_ivk, threads, 9)
        doc["host"].append(r)
        print(json.dumps(r), flush=True)
    doc["gpu_over_host"] = doc["gpu"][-1 if a.quick else 1]["trials_per_second"] / doc["host"][-1]["trials_per_second"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
