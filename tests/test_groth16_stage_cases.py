"""The inputs of tests/test_gpu_groth16_stages.py are what they claim to be: every check here goes through tests/pyref.py alone, so it
runs without a GPU and the GPU test never asserts a property its own inputs do not have."""
import pytest

import groth16_stage_cases as K
from pyref import F1, F2, G1, G2, P, R, ec_add, ec_mul, g2_comp


def test_edge_points_are_on_their_curves():
    for p in (G1, K.T3, K.NEG_T3, K.ORD11, K.g1_3r(5), K.g1_mul(7), None):
        assert K.on_curve(F1, p), p
    for q in (G2, K.G2_OUTSIDE, K.ORD13, K.G2_C1_ZERO, K.neg(F2, K.G2_C1_ZERO), K.g2_mul(7), None):
        assert K.on_curve(F2, q), q
    assert not K.on_curve(F1, (1, 1)) and not K.on_curve(F2, ((1, 0), (1, 0)))   # (the predicate can say no)


def test_small_orders():
    assert K.T3[0] == 0
    assert ec_mul(F1, K.T3, 3) is None and ec_add(F1, K.T3, K.T3) == K.NEG_T3
    assert K.ORD11 is not None and ec_mul(F1, K.ORD11, 11) is None
    assert K.ORD13 is not None and ec_mul(F2, K.ORD13, 13) is None
    assert ec_mul(F1, G1, R) is None and ec_mul(F2, G2, R) is None


def test_points_outside_the_subgroups():
    p = K.g1_3r(12345)
    assert ec_mul(F1, p, R) is not None and ec_mul(F1, p, 3 * R) is None            # order 3 r exactly: r is prime and [r] p = [r] T3 != O
    assert ec_mul(F1, K.T3, R) is not None and ec_mul(F1, K.ORD11, R) is not None
    for q in (K.G2_OUTSIDE, K.ORD13, K.G2_C1_ZERO):
        assert ec_mul(F2, q, R) is not None


def test_c1_zero_point_reaches_the_other_sign_rule():
    q = K.G2_C1_ZERO
    assert q[1][1] == 0 and q[1][0] != 0
    plus, minus = g2_comp(q), g2_comp(K.neg(F2, q))
    assert plus[1:] == minus[1:] and (plus[0] ^ minus[0]) == 0x20                    # same x, the sign flags differ
    assert (plus[0] & 0x20 != 0) == (q[1][0] > (P - 1) // 2)                          # ... and come from y.c0


def test_square_roots():
    for a in (4, 9, 2 ** 200 + 1):
        s = K.fp_sqrt(a * a % P)
        assert s in (a % P, P - a % P)
    for a in ((3, 5), (0, 7), (11, 0), (2 ** 300, 1)):
        sq = F2.mul(a, a)
        s = K.fp2_sqrt(sq)
        assert s is not None and F2.mul(s, s) == sq


def test_scalars_are_in_range():
    for r, s in K.RS_EDGES:
        assert 0 <= r < R and 0 <= s < R
    assert ((R - 1) * (R - 1)) % R == 1
    r, s = K.RS_EDGES[7]
    assert r.to_bytes(32, "little").count(0) == 31 and r.to_bytes(32, "little")[0] != 0
    assert s.to_bytes(32, "little").count(0) == 31 and s.to_bytes(32, "little")[31] != 0
    r, s = K.RS_EDGES[9]
    assert r.to_bytes(32, "little").count(0) == 31 and r.to_bytes(32, "little")[15] != 0
    r, s = K.RS_EDGES[10]
    assert r.to_bytes(32, "little") == b"\xff" * 31 + b"\x00"
    r, s = K.RS_EDGES[11]
    assert all((b == 0) == (i % 2 == 0) for i, b in enumerate(r.to_bytes(32, "little")))
    assert all((b == 0) == (i % 2 == 1) for i, b in enumerate(s.to_bytes(32, "little")))


def test_split_model_satisfies_the_bounds_the_gpu_test_asserts():
    ks = K.split_scalars()
    assert len(ks) == len(K.SPLIT_EDGES) + 200 and ks[:len(K.SPLIT_EDGES)] == K.SPLIT_EDGES
    for k in ks:
        assert 0 <= k < 2 ** 255
        q, rem = K.split_model(k)
        assert q * K.U_SQR + rem == k and 0 <= rem < K.U_SQR and 0 <= q < 2 ** 128, hex(k)
    assert K.split_model(K.U_SQR - 1) == (0, K.U_SQR - 1) and K.split_model(K.U_SQR) == (1, 0) and K.split_model(2 * K.U_SQR) == (2, 0)


def test_endomorphism_identity_the_split_relies_on():
    """[u^2] P = (beta x, -y) on the subgroup for one of the two cube roots of unity: what k_groth16_var_mul's second table is"""
    p = K.g1_mul(0x1234567)
    m = ec_mul(F1, p, K.U_SQR)
    assert m[1] == P - p[1] and pow(m[0] * pow(p[0], -1, P) % P, 3, P) == 1 and m[0] != p[0]


@pytest.mark.parametrize("name", ["g1", "t3", "ord11", "inf", "ord13"])
def test_table_model_against_ec_mul(name):
    F, p = {"g1": (F1, K.g1_mul(99)), "t3": (F1, K.T3), "ord11": (F1, K.ORD11), "inf": (F1, None), "ord13": (F2, K.ORD13)}[name]
    tab = K.table_model(F, p)
    assert len(tab) == 32 and all(len(row) == 255 for row in tab)
    for w, d in [(0, 1), (0, 2), (0, 255), (1, 1), (7, 33), (31, 255)]:
        assert tab[w][d - 1] == ec_mul(F, p, d << (8 * w)), (w, d)
    if name in ("t3", "ord11", "ord13"):
        order = {"t3": 3, "ord11": 11, "ord13": 13}[name]
        assert [e is None for e in tab[0][:2 * order]] == [(d % order) == 0 for d in range(1, 2 * order + 1)]
    if name == "inf":
        assert all(e is None for row in tab for e in row)


def test_table_sample_holds_the_windows_and_digits_it_says():
    s = K.table_sample(1)
    assert len(s) == 2 * 255 + 32 * 3 + 40
    assert {(w, d) for w in (0, 31) for d in range(1, 256)} <= set(s)
    assert {(w, d) for w in range(32) for d in (1, 2, 255)} <= set(s)
    assert all(0 <= w < 32 and 1 <= d <= 255 for w, d in s)
