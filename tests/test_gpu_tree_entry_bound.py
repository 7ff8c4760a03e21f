"""The bucket tree sized for what a witness can contain (masp_hip_ctx_set_tree_entry_share): proofs whose digit lists have more
entries than the tree's views were cut for are found on the device and go through the XYZZ accumulation — the same bytes, counted
in bucket_tree_fallback_proofs, for G1 (h + l, a, b_g1) and G2 (b_g2), one such proof among proofs under the bound, sub-batches
that do not divide the batch.  On the long-row toy circuit MIXED (tests/long_rows.py) with assignments made for the purpose: the
prover turns any assignment into the bytes the oracle turns it into.  Run with `-m gpu` on an MI355X."""
import random

import numpy as np
import pytest

import long_rows
import oracle_lib as O
import toy_r1cs
from pyref import R
from test_tree_entry_bound import densities, entries, ints

pytestmark = pytest.mark.gpu

NAME = "MIXED"
LEVELS = 4            # asked for, so that every batch MSM of the toy circuit goes through the tree whatever its run lengths
MSMS = 4              # h + l, a, b_g1, b_g2


def _le(x):
    return np.frombuffer((x % R).to_bytes(32, "little"), np.uint8)


class Rig:
    def __init__(self):
        import masp_amd
        self.cs, self.inputs, _, _ = long_rows.named(NAME)
        self.toxic = toy_r1cs.toxic(900)
        # share 100 (the default: nothing in this circuit is proven boolean, so the bound is the worst case); share 1 in the whole
        # batch and in sub-batches of four
        self.ctx = {"wide": masp_amd.Context(0, bucket_tree_levels=LEVELS), "tight": masp_amd.Context(0, bucket_tree_levels=LEVELS),
                    "tight4": masp_amd.Context(0, bucket_tree_levels=LEVELS, bucket_tree_sub_batch=4)}
        self.params = self.ctx["wide"].generate_parameters(self.cs, self.toxic)
        self.oparams = O.Params(self.params)
        for name, c in self.ctx.items():
            c.set_boolean_block_bits(-1)            # no subset rows: a digit list has exactly the entries Python counts
            if name != "wide":
                c.set_tree_entry_share(1)
                assert c.tree_entry_share == 1
            c.load_circuit(0, self.params, self.cs)
        rng = random.Random(901)
        n_aux = self.cs.n_aux
        # dense: every aux value full width.  sparse: zeros and ones but for two
        self.dense = [np.stack([_le(rng.randrange(2, R)) for _ in range(n_aux)]) for _ in range(9)]
        self.sparse = []
        for _ in range(9):
            v = [rng.randint(0, 1) for _ in range(n_aux)]
            for at in rng.sample(range(n_aux), 2):
                v[at] = rng.randrange(2, R)
            self.sparse.append(np.stack([_le(x) for x in v]))
        self.rs = [(rng.randrange(R), rng.randrange(R)) for _ in range(9)]
        self._want = {}

    def want(self, kind, k):
        if (kind, k) not in self._want:
            aux = (self.dense if kind == "dense" else self.sparse)[k]
            self._want[kind, k] = O.create_proof(self.oparams, self.cs, self.inputs, aux, *self.rs[k])
        return self._want[kind, k]

    def run(self, which, kinds):
        """proves job k with the dense or the sparse assignment k -> (all proofs equal the oracle's, proofs counted as fallen back)"""
        ctx = self.ctx[which]
        before = ctx.current_options()["bucket_tree_fallback_proofs"]
        jobs = [(0, self.inputs, (self.dense if kind == "dense" else self.sparse)[k]) + self.rs[k] for k, kind in enumerate(kinds)]
        got = ctx.prove_batch(jobs)
        bad = [k for k, kind in enumerate(kinds) if got[k] != self.want(kind, k)]
        return bad, ctx.current_options()["bucket_tree_fallback_proofs"] - before

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def test_the_assignments_lie_on_the_two_sides_of_the_bound(rig):
    """With Python integers: a sparse assignment has no more entries than the bound of any of the four MSMs (then its padded digit list
    fits the views: the bound leaves room for 2^pad_log - 1 padding entries per bucket), a dense one more than the bound and all the
    padding it allows — whatever the coset evaluations in front of the aux values in the merged MSM come to."""
    cs = rig.cs
    a_var, b_var = densities(cs)
    tight, wide = rig.ctx["tight"].circuit_tree_entry_bounds(0), rig.ctx["wide"].circuit_tree_entry_bounds(0)
    inputs = ints(rig.inputs)
    assert set(tight) == {"hl", "a", "b_g1", "b_g2"}
    for kind, auxs in (("dense", rig.dense), ("sparse", rig.sparse)):
        for aux in auxs:
            vals = inputs + ints(aux)
            for q, var in (("hl", None), ("a", a_var), ("b_g1", b_var), ("b_g2", b_var)):
                bound, c = tight[q]
                W, nb = (256 + c - 1) // c, 1 << (c - 1)
                if var is None:
                    # the merged set: the coset evaluations (or quotient coefficients) and the used inputs in front of the aux values, at W
                    # entries each at most; the aux values counted.  bound = W (fixed + k) + n_aux - k, k = ceil(n_aux / 100)
                    m, k = 1 << cs.logm, (cs.n_aux + 99) // 100
                    fixed, rem = divmod(bound - (cs.n_aux - k), W)
                    fixed -= k
                    assert rem == 0 and m - 1 <= fixed <= m + cs.n_inputs, (bound, W, fixed, rem)
                    lo, hi = entries(vals[cs.n_inputs:], c), entries(vals[cs.n_inputs:], c) + fixed * W
                else:
                    lo = hi = entries([vals[v] for v in var], c)
                    ones = int(0 in var)                                                  # share 100: only ONE is proven boolean
                    assert wide[q] == ((len(var) - ones) * W + ones, c)
                if kind == "sparse":
                    assert hi <= bound, (q, hi, bound)
                else:
                    assert lo > bound + 3 * nb, (q, lo, bound)


@pytest.mark.parametrize("which", ["wide", "tight", "tight4"])
def test_assignments_within_the_bound_go_through_the_tree(rig, which):
    bad, fell = rig.run(which, ["sparse"] * 9)
    assert not bad and fell == 0, (bad, fell)


def test_full_width_assignments_within_the_worst_case_bound(rig):
    bad, fell = rig.run("wide", ["dense"] * 9)
    assert not bad and fell == 0, (bad, fell)


@pytest.mark.parametrize("which", ["tight", "tight4"])
def test_every_proof_over_the_bound(rig, which):
    bad, fell = rig.run(which, ["dense"] * 9)
    assert not bad and fell == MSMS * 9, (bad, fell)


@pytest.mark.parametrize("at", [0, 3, 4, 8])
@pytest.mark.parametrize("which", ["tight", "tight4"])
def test_one_proof_over_the_bound_among_proofs_under_it(rig, which, at):
    """(sub-batches of four: the proof is the first of one, the last of one, the first of the next, alone in the last)"""
    kinds = ["sparse"] * 9
    kinds[at] = "dense"
    bad, fell = rig.run(which, kinds)
    assert not bad and fell == MSMS, (bad, fell)


def test_three_proofs_take_the_lone_path_without_a_tree(rig):
    bad, fell = rig.run("tight", ["dense", "sparse", "dense"])
    assert not bad and fell == 0, (bad, fell)


def test_the_sub_batch_in_use(rig):
    """explicit: the cap; automatic: the whole batch of nine went through in one"""
    assert rig.ctx["tight4"].current_options()["bucket_tree_sub_batch"] == 4
    rig.run("tight", ["sparse"] * 9)
    assert rig.ctx["tight"].current_options()["bucket_tree_sub_batch"] == 9
