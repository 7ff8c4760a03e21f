#!/usr/bin/env python3
"""Extracts the DATA of the reference's test_sapling_tree (masp_primitives/src/merkle_tree.rs:1091-1415; the loop that consumes it is
:1468-1533) into tests/golden/merkle_tree_vectors.json: five arrays of hex strings and no code.  Run where /root/reference exists; the
JSON file is committed and is what tests/test_incremental_tree_host.py reads.

  commitments   16 leaves of a depth-4 tree                         (zcash: merkle_commitments_sapling.json, byte-reversed)
  roots         16 roots, after each append                         (merkle_roots_sapling.json)
  tree_ser      16 CommitmentTree::write outputs                    (merkle_serialization_sapling.json)
  paths         120 MerklePath serialisations at depth 4            (merkle_path_sapling.json)
  witness_ser   136 IncrementalWitness::write outputs               (merkle_witness_serialization_sapling.json)

Order of paths and witness_ser: round i = 0..15 appends commitments[i] to the tree and to the i + 1 witnesses made so far (witness j was
made from the tree of j leaves, before round j's append), witness by witness; witness 0 (of the empty tree) has no path."""
import json
import os
import re

REF = "/root/reference/masp_primitives/src/merkle_tree.rs"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "merkle_tree_vectors.json")
COUNTS = {"commitments": 16, "roots": 16, "tree_ser": 16, "paths": 120, "witness_ser": 136}


def main():
    s = open(REF).read()
    s = s[s.index("fn test_sapling_tree()"):]
    s = s[:s.index("fn assert_root_eq")]
    out = {}
    for name, count in COUNTS.items():
        m = re.search(r"let %s = \[(.*?)\];" % name, s, re.S)
        out[name] = re.findall(r'"([0-9a-f]*)"', m.group(1))
        assert len(out[name]) == count, (name, len(out[name]))
    out["depth"] = 4
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
