"""masp_amd/csrc/device/conversion.hpp compiled for the host (tests/native/conversion_dev.hip): the terms, the lane shares and their
folds, the 88-chunk hash, with the generator point and cm traced, against conversion_ref.  CPU only; bytes."""
import numpy as np
import pytest

import conversion_ref as R
import conversion_shim as S
from masp_amd import host as H


def _check_trace(want, tr):
    for w, t in zip(want, tr):
        assert t[:32].tobytes() == w[1] and t[32:].tobytes() == w[3]


@pytest.mark.parametrize("lanes", [1, 8])
def test_edges(lanes):
    convs, want = R.references("edges")
    status, gens, cmus, tr = S.steps_host(*R.arrays(convs), lanes=lanes, trace=True)
    R.check((status, gens, cmus), want)
    _check_trace(want, tr)
    assert tr[R.edge("bit 255")][31] & 0x80 and not tr[R.edge("min alone")].any()


@pytest.mark.parametrize("lanes", [1, 8])
def test_random_batch(lanes):
    convs, want = R.references("random130")
    arrays = R.arrays(convs)
    status, gens, cmus, tr = S.steps_host(*arrays, lanes=lanes, trace=True)
    R.check((status, gens, cmus), want)
    _check_trace(want, tr)
    for x, y in zip((status, gens, cmus), H.allowed_conversions(*arrays, threads=2)):
        assert np.array_equal(x, y)


def test_other_lane_shares_sum_to_the_same_bytes():
    convs, want = R.references("edges")
    for lanes in (2, 3, 10):
        R.check(S.steps_host(*R.arrays(convs), lanes=lanes), want)


def test_the_hash_ends_at_88_chunks():
    """the 280-chunk note commitment over the generator padded with zeros is ANOTHER point: every zero chunk adds its window's base"""
    convs, want = R.references("edges")
    i = R.edge("+1")
    gen = want[i][1]
    padded = [(gen[k // 8] >> (k % 8)) & 1 for k in range(256)] + [0] * (832 - 256)
    assert H.point_uv(want[i][3])[0] != H.pedersen_hash(-1, padded)[0]
