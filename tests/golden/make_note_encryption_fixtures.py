#!/usr/bin/env python3
"""Extracts the reference's note-encryption known-answer DATA (no code) into tests/golden/note_encryption_vectors.json.
Usage: make_note_encryption_fixtures.py <reference checkout>; the JSON file is committed and is what the tests read.

Source: masp_primitives/src/test_vectors/note_encryption.rs, the 10 vectors checked at sapling/note_encryption.rs:1308-1480.
Every byte array becomes a hex string, `v` stays an integer.  The vectors use lead byte 1 (rcm in the plaintext) and the asset
identifier b"testtesttesttesttesttesttesttest" (note_encryption.rs:1323-1327), recorded here as `asset_identifier`.
"""
import json
import os
import re
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
FIELDS = {"ovk": 32, "ivk": 32, "default_d": 11, "default_pk_d": 32, "rcm": 32, "memo": 512, "cv": 32, "cmu": 32, "esk": 32, "epk": 32,
          "shared_secret": 32, "k_enc": 32, "p_enc": 596, "c_enc": 612, "ock": 32, "op": 64, "c_out": 80}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    s = open(os.path.join(sys.argv[1], "masp_primitives/src/test_vectors/note_encryption.rs")).read()
    blocks = s.split("TestVector {")[2:]   # [0] the head of the file, [1] the struct's own declaration
    out = []
    for b in blocks:
        tv = {}
        for name, size in FIELDS.items():
            m = re.search(r"\b%s: \[(.*?)\]," % name, b, re.S)
            data = bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", m.group(1)))
            assert len(data) == size, (name, len(data))
            tv[name] = data.hex()
        tv["v"] = int(re.search(r"\bv: (\d+),", b).group(1))
        out.append(tv)
    assert len(out) == 10, len(out)
    doc = {"source": "masp_primitives/src/test_vectors/note_encryption.rs", "lead_byte": 1,
           "asset_identifier": b"testtesttesttesttesttesttesttest".hex(), "vectors": out}
    with open(os.path.join(OUT, "note_encryption_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
