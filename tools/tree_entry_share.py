"""The share of a query's witness scalars, among those the R1CS does not prove boolean, that are neither 0 nor 1 — what
masp_hip_ctx_set_tree_entry_share (include/masp_hip.h) stands for — measured on the CPU over `workload.instances` of the three MASP
circuits.  No GPU: the synthesizer (libmasp_host) and the two host-only entry points of libmasp_hip.

    python tools/tree_entry_share.py [--seeds 64] [--first-seed 0]

Prints one line per circuit and query (l: the aux assignment, inside the merged h + l MSM; a; b), and the largest share of all.  The
default of the library (MASP_TREE_ENTRY_SHARE, masp_amd/csrc/internal.h) is that share with a quarter on top: MEASUREMENTS.md."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from masp_amd import hip, host as H, workload   # noqa: E402


def densities(cs):
    """-> (a_var, b_var) as masp_hip_circuit_load derives them: every input and the aux variables of A's columns; the variables of B's"""
    nv = cs.n_inputs + cs.n_aux
    in_a, in_b = np.zeros(nv, bool), np.zeros(nv, bool)
    in_a[cs.mats[0][1]] = True
    in_b[cs.mats[1][1]] = True
    in_a[:cs.n_inputs] = True
    return np.flatnonzero(in_a), np.flatnonzero(in_b)


def nontrivial(values):
    """u8[n, 32] little-endian -> bool[n]: neither 0 nor 1"""
    return (values[:, 0] > 1) | values[:, 1:].any(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--first-seed", type=int, default=0)
    args = ap.parse_args()
    worst = 0.0
    for kind in ("spend", "output", "convert"):
        cs = H.circuit(kind)[0]
        proven = hip.r1cs_boolean_variables(cs).astype(bool)
        a_var, b_var = densities(cs)
        aux = np.arange(cs.n_inputs, cs.n_inputs + cs.n_aux)
        queries = {"l": aux, "a": a_var, "b": b_var}
        top = {q: (0, 0.0) for q in queries}
        for inputs, aux_vals in workload.instances(kind, args.seeds, first_seed=args.first_seed):
            nt = nontrivial(np.concatenate([inputs, aux_vals]))
            assert not (nt & proven).any(), "a variable proven boolean holds another value"
            for q, var in queries.items():
                rest = var[~proven[var]]
                full = int(nt[rest].sum())
                top[q] = max(top[q], (full, full / max(len(rest), 1)))
        for q, var in queries.items():
            rest = int((~proven[var]).sum())
            print("%-8s %s: %6d scalars, %6d proven boolean, %6d not; of those at most %6d neither 0 nor 1 = %.2f %%  (%d seeds)"
                  % (kind, q, len(var), len(var) - rest, rest, top[q][0], 100 * top[q][1], args.seeds))
            worst = max(worst, top[q][1])
    print("largest share %.2f %%; with a quarter on top %.2f %%" % (100 * worst, 125 * worst))


if __name__ == "__main__":
    main()
