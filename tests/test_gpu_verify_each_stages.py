"""The kernels of the per-item verifiers, each on its own.  k_final_exp and k_verify_acc (masp_amd/csrc/device/pairing.hpp) are launched
through the test-side unit tests/native/verify_each_dev.hip with the product's tables: the final exponentiation against the host's
final_exp bytes, the public-input combination against big-integer sums.  k_jj_verify_each sits in k_redjubjub.hip's own translation
unit, so it is reached through its entry point masp_hip_redjubjub_verify_each — H* on the host, then that kernel alone — and compared
with masp_amd.redjubjub.verify.  Run with `-m gpu`."""
import random

import pytest

import oracle_lib as O
import test_final_exp_program as TF
import test_gpu_redjubjub_batch as TR
import verify_each_shim as VE
from pyref import P, R, g1_unc
from verify_ref import FP12_ONE, fp12_mul

pytestmark = pytest.mark.gpu
G1_IDENTITY = bytes([0x40]) + bytes(95)


# ---- k_final_exp ----
def test_final_exp_kernel_equals_the_host_final_exp():
    m = TF.miller_values()
    cancel = fp12_mul(m[0], m[2])                                   # ML(P, Q) ML(-P, Q)
    rng = random.Random(91)
    vals = [m[0], m[1], FP12_ONE, cancel, (0,) * 12] + [tuple(rng.randrange(P) for _ in range(12)) for _ in range(65)]
    got, verdict = VE.final_exp_gpu(vals)                           # 70 wavefronts: more than one block
    want = [VE.final_exp_host(v) for v in vals]
    assert got == want
    assert want[2] == FP12_ONE and want[3] == FP12_ONE and want[0] != FP12_ONE and want[4] == (0,) * 12
    assert verdict == [1 if w == FP12_ONE else 0 for w in want]
    assert verdict[:5] == [0, 0, 1, 1, 0]                           # zero: "invalid", and nothing was inverted


# ---- k_verify_acc ----
TOP_IN_RANGE = 7 * 16 ** 63          # the largest digit the top window of a value below r can hold (r = 0x73ed...)
EDGE_INPUTS = [0, 1, R - 1, 15 * 16 ** 62, TOP_IN_RANGE, 15]
assert TOP_IN_RANGE < R < 8 * 16 ** 63


def _neg(p96):
    if p96[0] & 0x40:
        return p96
    x, y = int.from_bytes(p96[:48], "big"), int.from_bytes(p96[48:], "big")
    return g1_unc((x, (P - y) % P))


def _multiples(ks):
    """[k] G for every k, as 96-byte strings (the oracle's fixed-base multiplication)"""
    import numpy as np
    arr = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32)
    return [row.tobytes() for row in O.g1_mul_gen_many(arr)]


def _check_acc(ks, rows):
    """IC_j = [ks[j]] G; rows: the inputs per proof.  acc_i = [ks[0] + sum_j x_ij ks[j]] G by big integers, then one oracle multiple."""
    ic = _multiples(ks)
    got, pre = VE.acc_gpu(ic, rows)
    in_range = [all(x < R for x in row) for row in rows]
    assert pre == [0 if ok else 3 for ok in in_range]
    sums = [(ks[0] + sum(x * k for x, k in zip(row, ks[1:]))) % R for row in rows]
    want = _multiples([s if s else 1 for s in sums])
    for i, row in enumerate(rows):
        if not in_range[i] or sums[i] == 0:
            assert got[i] == G1_IDENTITY, i
        else:
            assert got[i] == _neg(want[i]), (i, row)


@pytest.mark.parametrize("n_public,n", [(1, 1), (3, 64), (7, 65), (1, 65)])
def test_acc_kernel_equals_big_integer_sums(n_public, n):
    rng = random.Random(100 * n_public + n)
    ks = [rng.randrange(1, R) for _ in range(n_public + 1)]
    rows = [[e] * n_public for e in EDGE_INPUTS] + [[R] + [1] * (n_public - 1), [3] * (n_public - 1) + [2 ** 256 - 1]]
    rows += [[rng.choice(EDGE_INPUTS + [rng.randrange(R)]) for _ in range(n_public)] for _ in range(3)]
    while len(rows) < n:
        rows.append([rng.randrange(R) for _ in range(n_public)])
    rng.shuffle(rows)
    _check_acc(ks, rows[:n] if n > 1 else [rows[0]])


def test_acc_kernel_single_proof_edges():
    for x in EDGE_INPUTS + [R, 2 ** 256 - 1]:
        _check_acc([12345, 678], [[x]])


def test_acc_kernel_additions_are_exact_for_equal_and_opposite_points():
    # IC_1 = G.  P + P: IC_0 = [3 16^5] G is the table entry the input 3 16^5 selects.  P - P: IC_0 = [k] G and the input r - k, whose
    # running sum reaches -IC_0... and a sum that passes through the identity and leaves it again.
    _check_acc([3 * 16 ** 5, 1], [[3 * 16 ** 5], [R - 3 * 16 ** 5], [0]])
    _check_acc([R - 5, 1], [[5], [5 + 16 ** 9], [4]])
    # a status word from the decoder refuses the proof before anything is added
    ic = _multiples([7, 9])
    got, pre = VE.acc_gpu(ic, [[1], [R], [2]], status=[0, 8, 2])
    assert pre == [0, 2, 2] and got[1] == got[2] == G1_IDENTITY and got[0] != G1_IDENTITY


def test_acc_identity_in_the_key():
    """an IC point at infinity (a key can hold one) contributes nothing"""
    g = _multiples([11, 13])
    got, pre = VE.acc_gpu([g[0], G1_IDENTITY, g[1]], [[5, 2], [R - 1, 0]])
    want = _multiples([11 + 2 * 13, 11])
    assert pre == [0, 0] and got == [_neg(w) for w in want]


# ---- k_jj_verify_each ----
@pytest.fixture(scope="module")
def ctx():
    from masp_amd.hip import Context
    c = Context(0)
    yield c
    c.close()


def _small_order_cases(rng):
    """a vk of small order (any S with R = [S] G verifies: [c] vk dies under the cofactor, or not), R of small order with a matching S"""
    out = []
    for order in (2, 8):
        t = TR._torsion(order)
        for kind in (0, 1):
            sighash = bytes(rng.getrandbits(8) for _ in range(32))
            s = rng.randrange(1, TR.RJ)
            out.append((t, TR.H.jubjub_mul(TR.GENS[kind], s) + s.to_bytes(32, "little"), sighash, kind))     # vk = T, R = [S] G
            sk = rng.randrange(1, TR.RJ)
            vk = TR.H.jubjub_mul(TR.GENS[kind], sk)
            c = TR.RJS.h_star(t, vk + sighash)
            out.append((vk, t + (c * sk % TR.RJ).to_bytes(32, "little"), sighash, kind))                      # R = T, S = c sk
            out.append((vk, t + (c * sk % TR.RJ + 1).to_bytes(32, "little"), sighash, kind))                  # ... and S off by one
    return out


@pytest.mark.parametrize("n", [1, 64, 65])
def test_signature_kernel_equals_redjubjub_verify(ctx, n):
    rng = random.Random(200 + n)
    items = [TR._item(rng, kind=i % 2)[0] for i in range(max(n, 8))]
    vk, sig, sighash, kind = items[2]
    special = list(TR._corruptions(rng, items[3]).values())                                    # wrong sighash / kind, S >= r_J, non-canonical R, vk
    special.append((vk, sig, bytes([sighash[5] ^ 0x10]) + sighash[1:], kind))                  # a flipped message bit
    special.append((vk, sig[:32] + TR.RJ.to_bytes(32, "little"), sighash, kind))               # S = r_J exactly
    special += _small_order_cases(rng)
    for t in (2, 4, 8):                                                                         # cofactor cases both must accept
        tor = TR._torsion(t)
        sk = rng.randrange(1, TR.RJ)
        v = TR.H.jubjub_mul(TR.GENS[1], sk)
        special.append((v, TR._sign(rng, sk, v, sighash, 1, torsion=tor), sighash, 1))
    if n == 1:
        batches = [[it] for it in items[:2] + special]
    else:
        batch = list(items[:n])
        for k, it in zip(rng.sample(range(1, n - 1), len(special)), special):
            batch[k] = it
        batch[0], batch[n - 1] = special[0], special[1]                                        # a bad item first and last
        batches = [batch]
    seen = set()
    for batch in batches:
        want = [TR._single(it) for it in batch]
        assert ctx.redjubjub_verify_each(batch) == want
        seen.update(want)
    assert seen == {True, False}
    assert ctx.redjubjub_verify_each([]) == []
