#!/usr/bin/env python3
"""Measures batch output recovery with outgoing viewing keys: trials per second of the GPU call (masp_hip_sapling_output_recovery_scan,
from host memory to the sorted hit list, plus the host's finishing of the hits into notes) next to the host batch path
(masp_host_sapling_try_output_recovery_batch) over the same data on the CPUs this process may use.

  python tools/out_recovery_bench.py [--out profiles/out_recovery_bench.json] [--quick] [--reps N] [--threads N]

Per shape (outputs x ovks): one warm-up call of each side, then `--reps` (at least five) timed calls of each, alternating, so that the
two medians are of the same minutes of the same machine (host clock around a call that ends synchronised).  upload_ms / kernel_ms
come from HIP events on the scan's streams (masp_hip_out_recovery_last_timing), finish_ms is the host's second half
(masp_host_sapling_try_output_recovery_with_ock over the hits).  The outputs are random bytes (a trial's cost does not depend on them)
and 64 sent notes are planted per call so that the hit path runs.  gpu_not_below_host is the acceptance of the shape."""
import argparse
import datetime
import json
import os
import platform
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
ASSET = H.asset_identifier(b"output recovery bench")


def sent_output(ovk, rng):
    """an honest OutputDescription sent under ovk to a random address"""
    while True:
        d = rng.randbytes(11)
        try:
            gd = H.diversifier_base(d)
        except H.HostError:
            continue
        break
    to = NE.PaymentAddress(d, H.jubjub_mul(gd, rng.randrange(1, RJ).to_bytes(32, "little")))
    note = NE.Note(ASSET, rng.randrange(1 << 64), to.pk_d, NE.Rseed(2, rng.randbytes(32)))
    out = NE.sapling_note_encrypt(note, to)
    cv = H.value_commitment(ASSET, note.value, rng.randrange(RJ).to_bytes(32, "little"))[0]
    esk = NE.note_derive_esk(note)
    return NE.OutputDescription(cv, out.cmu, out.epk, out.enc_ciphertext, NE.encrypt_outgoing_plaintext(ovk, cv, out.cmu, out.epk, to.pk_d, esk))


def make_inputs(n_out, ovks, seed, n_planted=64):
    rng = random.Random(seed)
    nprng = np.random.default_rng(seed)
    cvs, epks, cmus = (nprng.integers(0, 256, (n_out, 32), dtype=np.uint8) for _ in range(3))
    couts = nprng.integers(0, 256, (n_out, 80), dtype=np.uint8)
    encs = np.zeros((n_out, 612), np.uint8)      # read for the hits alone
    places = sorted(rng.sample(range(n_out), min(n_planted, n_out)))
    for j, o in enumerate(places):
        out = sent_output(ovks[j % len(ovks)], rng)
        cvs[o], cmus[o], epks[o], encs[o], couts[o] = (np.frombuffer(x, np.uint8) for x in out)
    return cvs, epks, cmus, encs, couts, places


def gpu_call(ctx, ovks, cvs, epks, cmus, encs, couts):
    """one whole scan: the ABI call, then the host's finishing of its hits -> (call s, finish s, upload ms, kernel ms, outputs recovered)"""
    t0 = time.perf_counter()
    ho, hk, ocks = ctx.sapling_output_recovery_scan(ovks, cvs, epks, cmus, couts, hit_capacity=4096)
    t1 = time.perf_counter()
    found = set()
    for o, ock in zip(ho.tolist(), ocks):
        if o not in found and H.sapling_try_output_recovery_with_ock(ock.tobytes(), epks[o].tobytes(), cmus[o].tobytes(), encs[o].tobytes(),
                                                                     couts[o].tobytes(), 2):
            found.add(o)
    t2 = time.perf_counter()
    up, kern = ctx.out_recovery_last_timing()
    return t1 - t0, t2 - t1, up, kern, sorted(found)


def host_call(ovks, cvs, epks, cmus, encs, couts, threads):
    t0 = time.perf_counter()
    hit, _, _ = H.sapling_try_output_recovery_batch(ovks, cvs, epks, cmus, encs, couts, lead_byte=2, threads=threads)
    return time.perf_counter() - t0, [i for i, k in enumerate(hit.tolist()) if k >= 0]


def measure(ctx, n_out, n_ovk, reps, threads, seed):
    rng = random.Random(seed)
    ovk_list = [rng.randbytes(32) for _ in range(n_ovk)]
    ovks = np.frombuffer(b"".join(ovk_list), np.uint8).reshape(n_ovk, 32)
    cvs, epks, cmus, encs, couts, places = make_inputs(n_out, ovk_list, seed)
    gpu_call(ctx, ovks, cvs, epks, cmus, encs, couts)                  # warm-up: code objects, buffers
    host_call(ovks, cvs[:256], epks[:256], cmus[:256], encs[:256], couts[:256], threads)   # tables, threads
    g, h = [], []
    for _ in range(reps):
        g.append(gpu_call(ctx, ovks, cvs, epks, cmus, encs, couts))
        h.append(host_call(ovks, cvs, epks, cmus, encs, couts, threads))
    assert all(r[4] == places for r in g) and all(r[1] == places for r in h), "both sides recover the planted notes and nothing else"
    gt, ht = [r[0] + r[1] for r in g], [r[0] for r in h]
    gmed, hmed = statistics.median(gt), statistics.median(ht)
    i = gt.index(gmed) if gmed in gt else 0
    trials = n_out * n_ovk
    return {"outputs": n_out, "ovks": n_ovk, "trials": trials, "reps": reps, "notes_planted": len(places), "input_megabytes": n_out * 176 / 1e6,
            "gpu": {"seconds_median": gmed, "seconds_min": min(gt), "seconds_max": max(gt), "trials_per_second": trials / gmed,
                    "call_ms": g[i][0] * 1e3, "finish_ms": g[i][1] * 1e3, "upload_ms": g[i][2], "kernel_ms": g[i][3]},
            "host": {"threads": threads, "seconds_median": hmed, "seconds_min": min(ht), "seconds_max": max(ht), "trials_per_second": trials / hmed},
            "gpu_over_host": hmed / gmed, "gpu_not_below_host": gmed <= hmed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "out_recovery_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the comparison (capped by the CPUs this process may use)")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal, not a measurement")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("out_recovery_bench: no GPU (there is no CPU fallback for the scan)")
    reps = max(5, a.reps)
    threads = max(1, min(a.threads, H.effective_cpus()))
    ctx = masp_amd.Context(0)
    configs = [(4096, 1), (4096, 4)] if a.quick else [(65536, 1), (65536, 4), (65536, 16), (1 << 20, 1)]
    doc = {"tool": "tools/out_recovery_bench.py" + (" --quick" if a.quick else ""), "date": datetime.date.today().isoformat(),
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "host_threads": threads, "shapes": []}
    for n_out, n_ovk in configs:
        r = measure(ctx, n_out, n_ovk, reps, threads, 7)
        doc["shapes"].append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    doc["gpu_not_below_host_at_every_shape"] = all(r["gpu_not_below_host"] for r in doc["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
