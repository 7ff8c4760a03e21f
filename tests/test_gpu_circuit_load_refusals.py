"""What masp_hip_circuit_load refuses, what it leaves behind when it does, and the parameter files at the edges of what
masp_hip_generate_parameters writes.  One small circuit whose queries are all longer than 128 points (two waves of k_msm_import and a
remainder), its oracle CRS, one context; one point of the file is replaced at a time by an encoding from tests/setup_model.py's
bad_encodings.  The oracle's reader (oracle_params_parse, bellman's `Parameters::read(_, false)` restated) decides what must be refused;
the codes are MASP_HIP_E_PARAMS_FORMAT (2), and MASP_HIP_E_UNEXPECTED_IDENTITY (6) for a delta at infinity, which the reader accepts and
the prover refuses.  Bytes against bytes: no tolerance.  Run with `-m gpu`."""
import functools
import random

import numpy as np
import pytest

import oracle_lib as O
import setup_model as M
import toy_r1cs
from pyref import R

pytestmark = pytest.mark.gpu

SEED = 5
SLOT = 0
E_PARAMS_FORMAT, E_UNEXPECTED_IDENTITY = 2, 6


@functools.lru_cache(maxsize=None)
def circuit():
    cs, inputs, aux, _ = toy_r1cs.make(SEED, 3, 20, 200)
    buf = O.generate_parameters(cs, toy_r1cs.toxic(SEED)).tobytes()
    sec = M.section_offsets(buf)
    assert all(sec[name][2] > 128 for name in ("h", "l", "a", "b_g1", "b_g2")), sec
    return cs, inputs, aux, buf, sec


@pytest.fixture(scope="module")
def ctx():
    import masp_amd
    c = masp_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def good_proof(ctx):
    """the good circuit in the slot, and what it proves"""
    cs, inputs, aux, buf, _ = circuit()
    ctx.load_circuit(SLOT, np.frombuffer(buf, np.uint8), cs)
    proof = ctx.prove(SLOT, inputs, aux, 1111, 2222)
    assert proof == O.create_proof(O.Params(np.frombuffer(buf, np.uint8)), cs, inputs, aux, 1111, 2222)
    return proof


def _decode(curve, enc):
    from groth16_shim import g1_point, g2_point
    return (g1_point if curve == "g1" else g2_point)(enc)


def _oracle_accepts(buf):
    try:
        O.Params(np.frombuffer(buf, np.uint8))
        return True
    except ValueError:
        return False


def _load_corrupted(ctx, good_proof, offset, width, expect_delta=False):
    """every bad encoding at `offset`, one at a time -> the number of loads that were refused.  After each refusal the slot still proves
    what it proved (checked after the first refusal of this call and after the last); after an accepted load the good file goes back in."""
    import masp_amd
    cs, inputs, aux, buf, _ = circuit()
    curve = "g1" if width == 96 else "g2"
    refused = 0
    cases = M.bad_encodings(curve, _decode(curve, buf[offset:offset + width]))
    for name, enc, _status in cases:
        bad = buf[:offset] + enc + buf[offset + width:]
        assert len(bad) == len(buf)
        accepts = _oracle_accepts(bad)
        delta_inf = expect_delta and name == "infinity"
        if accepts and not delta_inf:
            ctx.load_circuit(SLOT, np.frombuffer(bad, np.uint8), cs)          # legal: alpha, beta, gamma or an ic point at infinity
            ctx.load_circuit(SLOT, np.frombuffer(buf, np.uint8), cs)
            continue
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.load_circuit(SLOT, np.frombuffer(bad, np.uint8), cs)
        assert e.value.code == (E_UNEXPECTED_IDENTITY if delta_inf else E_PARAMS_FORMAT), (name, offset)
        refused += 1
        if refused == 1:
            assert ctx.prove(SLOT, inputs, aux, 1111, 2222) == good_proof, "a refused load changed the slot's circuit"
    assert ctx.prove(SLOT, inputs, aux, 1111, 2222) == good_proof, "a refused load changed the slot's circuit"
    return refused, len(cases)


@pytest.mark.parametrize("pos", ["first", 63, 64, "last"])
@pytest.mark.parametrize("name", ["h", "l", "a", "b_g1", "b_g2"])
def test_bad_point_in_a_query(ctx, good_proof, name, pos):
    """an infinity, a flagged or a non-canonical point anywhere in a query vector: refused, and the slot keeps its circuit"""
    off, width, n = circuit()[4][name]
    k = {"first": 0, "last": n - 1}.get(pos, pos)
    refused, cases = _load_corrupted(ctx, good_proof, off + width * k, width)
    assert refused == cases                                   # bellman refuses the identity inside a query too


@pytest.mark.parametrize("k", [0, 1, 2])
def test_bad_point_in_ic(ctx, good_proof, k):
    """ic is the verifier's: the prover builds nothing from it, and yet an undecodable one is refused (infinity stays legal)"""
    off, width, n = circuit()[4]["ic"]
    assert n == 3
    refused, cases = _load_corrupted(ctx, good_proof, off + width * k, width)
    assert refused == cases - 1


@pytest.mark.parametrize("member", [m[0] for m in M.VK_MEMBERS])
def test_bad_verifying_key_member(ctx, good_proof, member):
    off, width = {m[0]: m[1:] for m in M.VK_MEMBERS}[member]
    is_delta = member.startswith("delta")
    refused, cases = _load_corrupted(ctx, good_proof, off, width, expect_delta=is_delta)
    assert refused == (cases if is_delta else cases - 1)      # alpha, beta, gamma at infinity are merely degenerate


# ---- degenerate but legal toxic waste, end to end ----
@functools.lru_cache(maxsize=None)
def circuit_all_in_c():
    """a circuit whose every aux variable occurs in C: with alpha = beta = 0 an l point is [C_j(tau) / delta] G, and a variable that C
    never names would put the identity into l — a file the reader refuses (test_both_zero_with_a_variable_outside_c).  With n_free = 0
    toy_r1cs.make allocates aux variables only in its product rows, and each of those puts its fresh variable into C (alone, or as
    k z' next to an older variable); the boolean rows, whose C is empty, come with n_free alone.  The assertion below checks that."""
    cs, inputs, aux, _ = toy_r1cs.make(6, 3, 0, 150)
    assert set(range(cs.n_inputs, cs.n_inputs + cs.n_aux)) <= set(cs.mats[2][1].tolist())
    return cs, inputs, aux


def _degenerate_toxic(seed, alpha, beta):
    tw = toy_r1cs.toxic(seed)
    tw[1], tw[2] = tw[1] * alpha, tw[2] * beta
    return tw


@pytest.mark.parametrize("alpha,beta", [(0, 1), (1, 0), (0, 0)])
def test_alpha_beta_zero_end_to_end(ctx, alpha, beta):
    """alpha_g1, beta_g1 / beta_g2 or all three at infinity: written as the oracle writes them, loaded, and proved with"""
    cs, inputs, aux = circuit_all_in_c()
    tw = _degenerate_toxic(6, alpha, beta)
    params = ctx.generate_parameters(cs, tw)
    want = O.generate_parameters(cs, tw)
    assert params.tobytes() == want.tobytes()
    assert (params[0] == 0x40) == (alpha == 0) and (params[96] == 0x40) == (beta == 0) and (params[192] == 0x40) == (beta == 0)
    P = O.Params(want)
    ctx.load_circuit(SLOT + 1, params, cs)
    rng = random.Random(alpha + 2 * beta)
    for r, s in ((0, 0), (rng.randrange(R), rng.randrange(R))):
        assert ctx.prove(SLOT + 1, inputs, aux, r, s) == O.create_proof(P, cs, inputs, aux, r, s), (r, s)


def test_both_zero_with_a_variable_outside_c(ctx, good_proof):
    """the main circuit has boolean constraints with an empty C row: with alpha = beta = 0 its l holds the identity.  generate_parameters
    writes what the oracle writes, and the reader's verdict on that file is the loader's."""
    import masp_amd
    cs, inputs, aux, _buf, _ = circuit()
    tw = _degenerate_toxic(SEED, 0, 0)
    params = ctx.generate_parameters(cs, tw)
    assert params.tobytes() == O.generate_parameters(cs, tw).tobytes()
    assert not _oracle_accepts(params.tobytes())
    with pytest.raises(masp_amd.MaspHipError) as e:
        ctx.load_circuit(SLOT, params, cs)
    assert e.value.code == E_PARAMS_FORMAT
    assert ctx.prove(SLOT, inputs, aux, 1111, 2222) == good_proof


# ---- shapes generate_parameters has not seen ----
def _toxic(tau):
    return [tau % R] + toy_r1cs.toxic(41)[1:]


def _three_way(ctx, cs, tw):
    got = ctx.generate_parameters(cs, tw).tobytes()
    assert got == O.generate_parameters(cs, tw).tobytes()
    assert got == M.generate_parameters(cs, tw)
    return M.section_offsets(got)


def test_generate_without_aux(ctx):
    cs = M.r1cs_from_rows(2, 0, [([(0, 3), (1, 1)], [(1, 1)], [(0, 5)]), ([(1, R - 1)], [(0, 1)], [(1, R - 1)])])
    for tau in (2, M.omega(2) + 1, 0):
        sec = _three_way(ctx, cs, _toxic(tau))
        assert sec["l"][2] == 0 and sec["h"][2] == 3 and sec["ic"][2] == 2


def test_generate_one_constraint(ctx):
    """one constraint and ONE as the only input: a domain of two points, one h point"""
    cs = M.r1cs_from_rows(1, 1, [([(0, 1)], [(1, 1)], [(1, 1)])])
    for tau in (2, R - 2, 0):
        sec = _three_way(ctx, cs, _toxic(tau))
        assert sec["h"][2] == 1 and sec["ic"][2] == 1 and sec["l"][2] == 1


def test_generate_filters_identities(ctx):
    """a variable absent from A, one absent from B, one whose A column cancels at this tau: filtered out of a / b, kept in l"""
    for tau in (2, random.Random(77).randrange(2, R)):
        cs, (n_a, n_b) = M.sparse_system(tau)
        sec = _three_way(ctx, cs, _toxic(tau))
        assert (sec["a"][2], sec["b_g1"][2], sec["b_g2"][2]) == (n_a, n_b, n_b)
        assert sec["l"][2] == 4 and sec["ic"][2] == 3 and sec["h"][2] == 7


# ---- tau on the domain ----
def test_generate_refuses_tau_on_the_domain(ctx):
    """tau^m = 1: Z(tau) = 0, every h point the identity (tests/test_setup_model.py pins what the definition gives there).  Refused before
    any launch, and the context goes on working."""
    import masp_amd
    cs = toy_r1cs.make(9, 2, 4, 9)[0]
    logm = cs.logm
    w = M.omega(logm)
    for tau in (1, R - 1, w, pow(w, (1 << logm) - 1, R), pow(w, 3, R)):
        with pytest.raises(masp_amd.MaspHipError) as e:
            ctx.generate_parameters(cs, _toxic(tau))
        assert e.value.code == E_UNEXPECTED_IDENTITY, tau
    # a root of unity of a larger domain is off this one
    tw = _toxic(M.omega(logm + 1))
    assert ctx.generate_parameters(cs, tw).tobytes() == O.generate_parameters(cs, tw).tobytes()
