"""The stream table of a device context (masp_hip_ctx::streams): the context creates every stream it uses and destroys each distinct
handle once; a slot only borrows its row.  Slots 0 and 1 have side streams of their own, from slot 2 on a slot's row holds slot 1's, and
with lone_proof_graph every slot has its own.  For shapes the other tests do not cover, contexts are created and destroyed one after the
other in one process: each counts the streams the rule gives and proves a lone proof with the oracle's bytes.  Run with `-m gpu`."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

SCRIPT = r"""
import random, sys
sys.path[:0] = [%r, %r]
import masp_amd
import oracle_lib as O
import toy_r1cs
from pyref import R
cs, inputs, aux, _ = toy_r1cs.make(67, 4, 80, 700, bool_share=0.6)
pbuf = O.generate_parameters(cs, toy_r1cs.toxic(67))
P = O.Params(pbuf)
rng = random.Random(69)
for slots in (1, 3, 5):
    for graph in (0, 1):
        ctx = masp_amd.Context(0, slots=slots, lone_proof_graph=graph)
        try:
            n = ctx.stream_concurrency()[0]
            want = 3 + slots + 4 * (slots if graph else min(slots, 2))
            assert n == want, (slots, graph, n, want)
            ctx.load_circuit(2, pbuf, cs)
            r, s = rng.randrange(R), rng.randrange(R)
            assert ctx.prove_batch([(2, inputs, aux, r, s)]) == [O.create_proof(P, cs, inputs, aux, r, s)], (slots, graph)
            print("slots", slots, "graph", graph, "streams", n, flush=True)
        finally:
            ctx.close()
""" % (ROOT, TESTS)


def test_contexts_of_every_shape_own_the_streams_the_rule_gives():
    out = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert len(out.stdout.splitlines()) == 6, out.stdout
