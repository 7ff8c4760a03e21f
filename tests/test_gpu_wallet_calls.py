"""The six wallet-side calls of a device context next to each other (the full and the compact note scan, output recovery, the frozen tree,
the appended block, the nullifiers): they share one mutex, the two verifier streams and the Pedersen table, and each has a timing record
of its own.  What each call computes is its own file's business; here every comparison is of a call with itself, byte for byte."""
import math
import random
import threading

import numpy as np
import pytest

import compact_notes as CN
import masp_amd
import merkle_ref as R
import nullifier_ref as NR
import out_recovery_cases as K
from masp_amd import host as H
from masp_amd.merkle_tree import MT_TOP_PARENTS

pytestmark = pytest.mark.gpu

OUT_FIELDS = (("cv", 32), ("epk", 32), ("cmu", 32), ("out_ciphertext", 80))


def note_rows(n_out, places, seed):
    """2 ivks x n_out outputs of noise with a note (lead byte 2) planted at each of `places` -> (ivks, epks, cmus, encs)"""
    rng = random.Random(seed)
    ivks_int = [rng.randrange(1, CN.RJ) for _ in range(2)]
    epks, cmus, encs = CN.noise(n_out, seed)
    for j, o in enumerate(places):
        out, _, _ = CN.planted(ivks_int[j % 2], seed * 1000 + j)
        epks[o], cmus[o], encs[o] = (np.frombuffer(x, np.uint8) for x in out)
    return b"".join(k.to_bytes(32, "little") for k in ivks_int), epks, cmus, encs


def sent_rows(n_out, places, seed):
    """2 ovks x n_out outputs of noise with a sent note planted at each of `places` -> (ovks, cvs, epks, cmus, out_ciphertexts)"""
    rng = random.Random(seed)
    ovks = [rng.randbytes(32) for _ in range(2)]
    g = np.random.default_rng(seed)
    rows = {f: g.integers(0, 256, (n_out, w), dtype=np.uint8) for f, w in OUT_FIELDS}
    for j, o in enumerate(places):
        output = K.Sent(ovks[j % 2], CN.ASSET, seed * 1000 + j).output
        for f, _ in OUT_FIELDS:
            rows[f][o] = np.frombuffer(getattr(output, f), np.uint8)
    return (b"".join(ovks),) + tuple(rows[f] for f, _ in OUT_FIELDS)


def arr(nodes):
    return np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 32)


def as_bytes(result):
    """a call's result as a tuple of byte strings (and what is not an array as it is)"""
    if isinstance(result, np.ndarray):
        result = (result,)
    return tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in result)


def wallet_calls(ctx, n_out, places, n_leaves):
    """[(name, index of its timing getter, the call)] over inputs built once; the getters in the order of GETTERS"""
    ivks, epks, cmus, encs = note_rows(n_out, places, 71)
    enc84 = np.ascontiguousarray(encs[:, :84])
    sent = sent_rows(n_out, places, 72)
    leaves = arr(R.random_nodes(n_leaves, 7300 + n_leaves))
    frontier = arr([random.Random(74).randrange(R.Q).to_bytes(32, "little")] + [b"\xff" * 32] * 31)      # start = 1 reads entry 0 alone
    block = arr(R.random_nodes(2, 75))
    notes = NR.arrays([NR.good_note(76), NR.good_note(77)])
    return [
        ("full scan", 0, lambda: ctx.sapling_trial_decrypt(ivks, epks, encs)),
        ("compact scan", 1, lambda: ctx.sapling_compact_trial_decrypt(ivks, epks, cmus, enc84, 2)),
        ("output recovery", 2, lambda: ctx.sapling_output_recovery_scan(*sent)),
        ("frozen tree", 3, lambda: ctx.merkle_tree_complete(leaves, 0, [n_leaves - 1])),
        ("appended block", 3, lambda: ctx.merkle_tree_append(1, frontier, block)),
        ("nullifiers", 4, lambda: ctx.note_nullifiers(*notes)),
    ]


GETTERS = (("note_scan_last_timing", 2, (1,)), ("note_scan_compact_last_timing", 3, (1, 2)), ("out_recovery_last_timing", 2, (1,)),
           ("merkle_last_timing", 3, (1,)), ("note_nullifiers_last_timing", 3, (1,)))      # (name, length, its kernel entries)
HIT_OUTPUT = (1, 1, 0)      # where hit_output stands in the results of the three scans


def test_each_timing_getter_reads_its_own_call():
    """2 keys x 3 outputs with one planted note, a tree of 3 leaves with one path, a block of 2 leaves at 1, 2 notes: the smallest inputs
    that launch every kernel of each call.  A getter answers zeros until its call has run, then that call's times, and no other call
    changes them."""
    ctx = masp_amd.Context(0)
    try:
        read = lambda g: tuple(getattr(ctx, GETTERS[g][0])())
        for g, (_, length, _) in enumerate(GETTERS):
            assert read(g) == (0.0,) * length
        seen = {}
        for name, own, call in wallet_calls(ctx, 3, [1], 3):
            result = call()
            if own < 3:
                assert len(result[HIT_OUTPUT[own]]) == 1, name      # the planted pair is a hit: every kernel of the call had work
            ms = read(own)
            print(name, ms)
            assert len(ms) == GETTERS[own][1] and all(math.isfinite(t) and t >= 0 for t in ms), (name, ms)
            assert all(ms[k] > 0 for k in GETTERS[own][2]), (name, ms)
            seen[own] = ms
            for g, (_, length, _) in enumerate(GETTERS):
                assert read(g) == seen.get(g, (0.0,) * length), (name, GETTERS[g][0])
        assert len(seen) == 5
    finally:
        ctx.close()


def test_wallet_calls_of_every_kind_from_four_threads():
    """2 keys x 300 outputs (a chunk of two workgroups, the second ragged) and 131 leaves (k_mt_level, then k_mt_top); four threads make
    the six calls in four different orders, three rounds each, on one context: every result is the bytes of the same call made alone."""
    assert 131 > 2 * MT_TOP_PARENTS
    ctx = masp_amd.Context(0)
    try:
        places = [0, 255, 256, 299]
        calls = wallet_calls(ctx, 300, places, 131)
        alone = [as_bytes(call()) for _, _, call in calls]
        want_hits = np.asarray(places, np.uint32).tobytes()
        assert [alone[k][HIT_OUTPUT[k]] for k in range(3)] == [want_hits] * 3      # the planted pairs, and no other
        assert [len(a[0]) for a in alone[3:5]] == [32 * H.merkle_node_count(131), 32 * H.merkle_append_node_count(1, 2)]
        assert alone[5][0] == bytes(2)                                     # both notes are valid
        orders = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [3, 0, 5, 1, 4, 2], [1, 3, 2, 5, 0, 4]]
        wrong = [[] for _ in orders]

        def work(t):
            try:
                for rnd in range(3):
                    for k in orders[t]:
                        if as_bytes(calls[k][2]()) != alone[k]:
                            wrong[t].append((rnd, calls[k][0]))
            except Exception as e:      # (a failure in a thread is not the test's unless it is carried over)
                wrong[t].append(repr(e))

        threads = [threading.Thread(target=work, args=(t,)) for t in range(len(orders))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert wrong == [[] for _ in orders]
    finally:
        ctx.close()
