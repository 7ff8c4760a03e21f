"""Groth16 parameter generation by definition (wire format A.5): pure Python over tests/pyref.py, independent of the C++
oracle, of tests/pyclosed.py and of every HIP kernel.

The three of them evaluate the Lagrange basis at tau by the closed formula l_k(tau) = (Z(tau) / m) w^k / (tau - w^k).  Here it is what
bellperson computes: the inverse transform of the powers of tau over the domain {w^k}, row k <-> w^k,

    l_k(tau) = (1 / m) sum_i tau^i w^(-i k)          (l_k is the polynomial of degree < m with l_k(w^j) = [j == k]),

which needs no inverse of tau - w^k and so has a value on the domain too: l_k(w^j) = [j == k], Z = 0.
Scalar multiplication is a sum over the set bits of the scalar of a table of doublings of the generator: no window, no Montgomery form."""
from pyref import F1, F2, G1, G2, R, ec_add, g1_unc, g2_unc

ROOT_OF_UNITY_2_32 = pow(7, (R - 1) >> 32, R)     # 7 generates Fr^*, 2-adicity 32


def log2_ceil(n):
    """bellperson's domain: the smallest m = 2^k >= n, and k >= 1 in this project (masp_amd/r1cs.py: logm)"""
    return max(1, (n - 1).bit_length())


def omega(logm):
    return pow(ROOT_OF_UNITY_2_32, 1 << (32 - logm), R)


def lagrange_at(tau, logm):
    """[l_k(tau) for k < m]: the inverse DFT of (1, tau, ..., tau^(m-1)) over {w^k}"""
    m = 1 << logm
    winv = pow(omega(logm), -1, R)
    wp = [1] * m                      # w^(-j)
    for j in range(1, m):
        wp[j] = wp[j - 1] * winv % R
    tp = [1] * m                      # tau^i, with 0^0 = 1
    for i in range(1, m):
        tp[i] = tp[i - 1] * tau % R
    minv = pow(m, -1, R)
    return [minv * sum(tp[i] * wp[i * k % m] for i in range(m)) % R for k in range(m)]


def coefs(coef_u8):
    return [int.from_bytes(coef_u8[t].tobytes(), "little") for t in range(coef_u8.shape[0])]


def qap_at_tau(cs, tau):
    """-> (lag[m], [A_v(tau)], [B_v(tau)], [C_v(tau)]) per variable, inputs first: sums over the constraint rows, and for A the n_inputs
    extra rows Input(i) * 0 = 0 behind them"""
    nc, n_in, nv = cs.n_constraints, cs.n_inputs, cs.n_inputs + cs.n_aux
    lag = lagrange_at(tau, log2_ceil(nc + n_in))
    out = []
    for rp, col, coef in cs.mats:
        acc, cf, rp, col = [0] * nv, coefs(coef), rp.tolist(), col.tolist()
        for row in range(nc):
            for t in range(rp[row], rp[row + 1]):
                acc[col[t]] = (acc[col[t]] + cf[t] * lag[row]) % R
        out.append(acc)
    for i in range(n_in):
        out[0][i] = (out[0][i] + lag[nc + i]) % R
    return lag, out[0], out[1], out[2]


_doublings = {}


def mul_gen(F, gen, k):
    """[k] gen as the sum of 2^i gen over the set bits of k"""
    tab = _doublings.get(gen)
    if tab is None:
        tab = [gen]
        for _ in range(255):
            tab.append(ec_add(F, tab[-1], tab[-1]))
        _doublings[gen] = tab
    acc, i = None, 0
    k %= R
    while k:
        if k & 1:
            acc = ec_add(F, acc, tab[i])
        k >>= 1
        i += 1
    return acc


def g1_mul(k): return mul_gen(F1, G1, k)
def g2_mul(k): return mul_gen(F2, G2, k)


def parameter_scalars(cs, toxic):
    """the discrete logarithms of everything in the file: dict of vk (alpha, beta, gamma, delta), ic, h, l, a, b (a and b with the
    identities filtered out, inputs first)"""
    tau, alpha, beta, gamma, delta = [t % R for t in toxic]
    n_in, nv = cs.n_inputs, cs.n_inputs + cs.n_aux
    m = 1 << log2_ceil(cs.n_constraints + n_in)
    _lag, at, bt, ct = qap_at_tau(cs, tau)
    ginv, dinv = pow(gamma, -1, R), pow(delta, -1, R)
    z = (pow(tau, m, R) - 1) % R
    lc = [(beta * at[v] + alpha * bt[v] + ct[v]) % R for v in range(nv)]
    h, cur = [], z * dinv % R
    for _ in range(m - 1):
        h.append(cur)
        cur = cur * tau % R
    return {"vk": (alpha, beta, gamma, delta), "ic": [x * ginv % R for x in lc[:n_in]], "h": h, "l": [x * dinv % R for x in lc[n_in:]],
            "a": [x for x in at if x], "b": [x for x in bt if x]}


def _u32be(n): return int(n).to_bytes(4, "big")


def generate_parameters(cs, toxic):
    """-> the bellman Parameters bytes"""
    s = parameter_scalars(cs, toxic)
    alpha, beta, gamma, delta = s["vk"]
    out = [g1_unc(g1_mul(alpha)), g1_unc(g1_mul(beta)), g2_unc(g2_mul(beta)), g2_unc(g2_mul(gamma)), g1_unc(g1_mul(delta)),
           g2_unc(g2_mul(delta))]
    for name in ("ic", "h", "l", "a", "b"):
        out.append(_u32be(len(s[name])))
        out += [g1_unc(g1_mul(k)) for k in s[name]]
    out.append(_u32be(len(s["b"])))
    out += [g2_unc(g2_mul(k)) for k in s["b"]]
    return b"".join(out)


# ---- the file's sections, by offset (tests that corrupt or compare one point at a time) ----
VK_MEMBERS = (("alpha_g1", 0, 96), ("beta_g1", 96, 96), ("beta_g2", 192, 192), ("gamma_g2", 384, 192), ("delta_g1", 576, 96),
              ("delta_g2", 672, 192))
SECTIONS = (("ic", 96), ("h", 96), ("l", 96), ("a", 96), ("b_g1", 96), ("b_g2", 192))


def section_offsets(buf):
    """Parameters bytes -> {name: (offset of the first point, point width, number of points)}"""
    buf = bytes(buf)
    out, p = {}, 864
    for name, width in SECTIONS:
        n = int.from_bytes(buf[p:p + 4], "big")
        out[name] = (p + 4, width, n)
        p += 4 + n * width
    assert p == len(buf), (p, len(buf))
    return out


# ---- hand-built constraint systems ----
def r1cs_from_rows(n_inputs, n_aux, rows):
    """rows: [(A, B, C)], each a list of (variable, coefficient) with the variables ascending -> masp_amd.r1cs.R1cs"""
    import numpy as np
    from oracle_lib import R1cs
    mats = []
    for mi in range(3):
        rp, col, coef = [0], [], []
        for row in rows:
            for v, c in row[mi]:
                assert 0 <= v < n_inputs + n_aux
                col.append(v)
                coef.append(np.frombuffer((c % R).to_bytes(32, "little"), dtype=np.uint8))
            rp.append(len(col))
        mats.append((np.array(rp, np.uint32), np.array(col, np.uint32), np.stack(coef) if coef else np.zeros((0, 32), np.uint8)))
    return R1cs(n_inputs, n_aux, len(rows), mats)


def sparse_system(tau):
    """3 inputs (ONE, x1, x2), 4 aux (y0 .. y3), 5 constraints, m = 8.  y1 never appears in A, y2 never in B, x2 in neither (its A is
    the extra row alone), and y3 appears in A on rows 1 and 3 with coefficients chosen for this tau so that A_y3(tau) = 0: it is dense
    in A and yet filtered out of the a query.  -> (R1cs, the filtered lengths (len a, len b))"""
    lag = lagrange_at(tau % R, 3)
    assert lag[1] and lag[3], "tau is on the domain"
    c3 = (-5 * lag[1]) * pow(lag[3], -1, R) % R           # 5 l_1 + c3 l_3 = 0
    ONE, X1, X2, Y0, Y1, Y2, Y3 = range(7)
    rows = [([(ONE, 1), (Y0, R - 1)], [(Y0, 1)], []),
            ([(X1, 2), (Y3, 5)], [(ONE, 3), (Y1, 1)], [(Y2, 1)]),
            ([(Y0, 7), (Y2, R - 2)], [(Y1, R - 3)], [(X2, 1), (Y3, 4)]),
            ([(Y2, 1), (Y3, c3)], [(Y0, 9), (Y3, 1)], [(Y1, 1)]),
            ([(ONE, R - 1)], [(X1, 1)], [(ONE, 1), (X1, 1)])]
    # a: ONE, x1, x2 (extra rows), y0, y2 — not y1 (absent), not y3 (cancels);  b: ONE, x1, y0, y1, y3 — not x2, y2 (absent)
    return r1cs_from_rows(3, 4, rows), (5, 5)


# ---- encodings a reader of uncompressed points must classify (status values of masp_amd/csrc/device/io.hpp, tests/verify_ref.py) ----
def bad_encodings(curve, point):
    """[(name, bytes, status)] made from one good affine point: the encodings that bellman's `Parameters::read` refuses or treats
    specially.  Status by the reader's definition: bit 0x80 set is PT_BAD_FLAGS, else bit 0x40 set is PT_INFINITY, else a
    coordinate that is no reduced residue is PT_NOT_CANONICAL — which is also what the sort flag 0x20 amounts to in this form, where it
    is bit 381 of the first coordinate (p has 381 bits)."""
    from pyref import P
    from verify_ref import PT_BAD_FLAGS, PT_INFINITY, PT_NOT_CANONICAL
    width, good = (96, g1_unc(point)) if curve == "g1" else (192, g2_unc(point))
    names = ("x", "y") if curve == "g1" else ("x.c1", "x.c0", "y.c1", "y.c0")
    out = [("infinity", b"\x40" + bytes(width - 1), PT_INFINITY),
           ("flag 0x80", bytes([good[0] | 0x80]) + good[1:], PT_BAD_FLAGS),
           ("flag 0x20", bytes([good[0] | 0x20]) + good[1:], PT_NOT_CANONICAL)]
    for k, name in enumerate(names):
        c = int.from_bytes(good[48 * k:48 * k + 48], "big")
        for what, v in (("p", P), ("p + itself", P + c)):
            enc = good[:48 * k] + v.to_bytes(48, "big") + good[48 * k + 48:]
            assert not enc[0] & 0xc0
            out.append(("%s = %s" % (name, what), enc, PT_NOT_CANONICAL))
    return out
