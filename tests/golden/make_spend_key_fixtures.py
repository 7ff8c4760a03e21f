#!/usr/bin/env python3
"""Extracts the reference's ZIP 32 spending-key known-answer DATA (no code) into tests/golden/zip32_key_vectors.json.
Usage: make_spend_key_fixtures.py <reference checkout>; the JSON file is committed and is what the tests read.

Source: masp_primitives/src/zip32/sapling.rs, the test vectors of its `test_vectors` test (from zcash-test-vectors' sapling_zip32.py).
Of the five vectors the three that carry an `ask` (the hardened path's) are kept, and of each the four arrays that pin the two fixed-base
multiplications behind a spend: ask, nsk, ak = [ask] G_spend, nk = [nsk] G_pgk.  Every byte array becomes a hex string.
"""
import json
import os
import re
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("ask", "nsk", "ak", "nk")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    s = open(os.path.join(sys.argv[1], "masp_primitives/src/zip32/sapling.rs")).read()
    blocks = s.split("TestVector {")[2:]   # [0] the head of the file, [1] the struct's own declaration
    out = []
    for b in blocks:
        if not re.search(r"\bask: Some\(\[", b):
            continue
        tv = {}
        for name in FIELDS:
            m = re.search(r"\b%s: (?:Some\()?\[(.*?)\]" % name, b, re.S)
            data = bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", m.group(1)))
            assert len(data) == 32, (name, len(data))
            tv[name] = data.hex()
        out.append(tv)
    assert len(out) == 3, len(out)
    doc = {"source": "masp_primitives/src/zip32/sapling.rs", "vectors": out}
    with open(os.path.join(OUT, "zip32_key_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
