"""The evaluation-form quotient's three-kernel schedule (masp_amd/csrc/device/ntt.hpp: k_ntt_dif_top, k_ntt_mid, k_ntt_dit_top_ab) over
any prime field with enough two-adicity, twice: PLAINLY — a stage is a loop over every index pair of the whole vector — which is what the
GPU tests compare a kernel's output with, and AS THE KERNELS INDEX IT — workgroup by workgroup and lane by lane, with their tile
membership, their twiddle index per stage and the bit-reversed scale index — which tests/test_quotient_schedule_model.py compares with the
plain form and with direct interpolation and evaluation.

Stage s pairs the elements whose indices differ in bit s; its twiddle is tw[j << (logm - s - 1)] with j the index's bits below s and
tw[k] = w^k, k < m / 2.  Decimation in time (DIT): s upwards, (u + v w, u - v w).  Decimation in frequency (DIF): s downwards,
(u + v, (u - v) w), natural order in, bit-reversed order out."""


class Field:
    """p prime, root: an element of order 2^two_adicity, gen: the coset shift (not in the subgroup of order 2^two_adicity)"""

    def __init__(self, p, root, two_adicity, gen):
        self.p, self.root, self.two_adicity, self.gen = p, root, two_adicity, gen
        self._tables = {}

    def omega(self, logm):
        return pow(self.root, 1 << (self.two_adicity - logm), self.p)

    def tables(self, logm):
        """(tw_fwd, tw_inv, scale_rev, e_scale): NttDomain's tables, plain integers"""
        if logm not in self._tables:
            p, m, w = self.p, 1 << logm, self.omega(logm)
            w_inv, m_inv = pow(w, -1, p), pow(1 << logm, -1, p)
            powers = lambda b, n: [pow(b, k, p) for k in range(n)]
            scale_rev = [pow(self.gen, rev(i, logm), p) * m_inv % p for i in range(m)]
            self._tables[logm] = (powers(w, m // 2), powers(w_inv, m // 2), scale_rev, pow(pow(self.gen, m, p) - 1, -1, p))
        return self._tables[logm]


SMALL = Field(65537, 3, 16, 3)           # 3 generates the whole multiplicative group of order 2^16


def rev(k, bits):
    return int(format(k, "0%db" % bits)[::-1], 2) if bits else 0


# ---- plainly -------------------------------------------------------------------------------------------------------------------------
def stage(x, p, tw, logm, s, dif):
    """one stage over the whole vector, in place"""
    for i in range(1 << logm):
        if i >> s & 1:
            continue
        k = i | 1 << s
        w = tw[(i & ((1 << s) - 1)) << (logm - s - 1)]
        u, v = x[i], x[k]
        if dif:
            x[i], x[k] = (u + v) % p, (u - v) * w % p
        else:
            v = v * w % p
            x[i], x[k] = (u + v) % p, (u - v) % p


def dif_top(F, a, nrows, logm, lt):
    """what k_ntt_dif_top leaves of one vector: a[:nrows], zero above, through DIF stages logm - 1 ... lt"""
    x = [v % F.p for v in a[:nrows]] + [0] * ((1 << logm) - nrows)
    tw_inv = F.tables(logm)[1]
    for s in range(logm - 1, lt - 1, -1):
        stage(x, F.p, tw_inv, logm, s, True)
    return x


def mid(F, x, logm, lt):
    """k_ntt_mid on one vector"""
    x = list(x)
    tw_fwd, tw_inv, scale_rev, _ = F.tables(logm)
    for s in range(lt - 1, -1, -1):
        stage(x, F.p, tw_inv, logm, s, True)
    x = [v * c % F.p for v, c in zip(x, scale_rev)]
    for s in range(lt):
        stage(x, F.p, tw_fwd, logm, s, False)
    return x


def dit_top_ab(F, a, b, logm, lt):
    """k_ntt_dit_top_ab on one pair of vectors"""
    a, b = list(a), list(b)
    tw_fwd, _, _, e_scale = F.tables(logm)
    for s in range(lt, logm):
        stage(a, F.p, tw_fwd, logm, s, False)
        stage(b, F.p, tw_fwd, logm, s, False)
    return [u * v * e_scale % F.p for u, v in zip(a, b)]


def direct(F, a, b, nrows, logm):
    """a b / (g^m - 1) on the coset g H of the polynomials that interpolate a[:nrows] and b[:nrows] (zero above) on H: O(m^2)"""
    p, m, w = F.p, 1 << logm, F.omega(logm)
    m_inv, w_inv = pow(m, -1, p), pow(w, -1, p)
    e_scale = pow(pow(F.gen, m, p) - 1, -1, p)

    def on_coset(ev):
        ev = [v % p for v in ev[:nrows]] + [0] * (m - nrows)
        wi = [pow(w_inv, k, p) for k in range(m)]
        coef = [sum(ev[k] * wi[j * k % m] for k in range(m)) * m_inv % p for j in range(m)]
        pts = [F.gen * pow(w, k, p) % p for k in range(m)]
        out = []
        for x in pts:
            acc = 0
            for c in reversed(coef):
                acc = (acc * x + c) % p
            out.append(acc)
        return out

    return [u * v * e_scale % p for u, v in zip(on_coset(a), on_coset(b))]


# ---- as the kernels index it ---------------------------------------------------------------------------------------------------------
def _top_stages(tile, p, tw, logm, lt, col0, dif):
    """ntt_top_stages: tile[(h << cols_log) | cl] is element (h << lt) | (col0 + cl); tile / 4 lanes, a quad each in a paired round"""
    nst = logm - lt
    cols_log = lt - nst
    cols, lanes = 1 << cols_log, (1 << lt) // 4

    def pair(q):
        s = lt + q
        for t in range(lanes):
            cl, r = t & (cols - 1), t >> cols_log
            hj, hg = r & ((1 << q) - 1), r >> q
            L0, d = ((hg << (q + 2) | hj) << cols_log) | cl, cols << q
            lo = col0 + cl
            j1, j2a, j2b = hj << lt | lo, hj << lt | lo, (hj | 1 << q) << lt | lo
            w1, w2a, w2b = tw[j1 << (logm - s - 1)], tw[j2a << (logm - s - 2)], tw[j2b << (logm - s - 2)]
            x0, x1, x2, x3 = tile[L0], tile[L0 + d], tile[L0 + 2 * d], tile[L0 + 3 * d]
            if dif:
                y0, y2, y1, y3 = (x0 + x2) % p, (x0 - x2) * w2a % p, (x1 + x3) % p, (x1 - x3) * w2b % p
                tile[L0], tile[L0 + d], tile[L0 + 2 * d], tile[L0 + 3 * d] = (y0 + y1) % p, (y0 - y1) * w1 % p, (y2 + y3) % p, (y2 - y3) * w1 % p
            else:
                u = x1 * w1 % p
                y0, y1 = (x0 + u) % p, (x0 - u) % p
                u = x3 * w1 % p
                y2, y3 = (x2 + u) % p, (x2 - u) % p
                u = y2 * w2a % p
                tile[L0], tile[L0 + 2 * d] = (y0 + u) % p, (y0 - u) % p
                u = y3 * w2b % p
                tile[L0 + d], tile[L0 + 3 * d] = (y1 + u) % p, (y1 - u) % p

    def single(q):
        s = lt + q
        for b in range((1 << lt) // 2):
            cl, hb = b & (cols - 1), b >> cols_log
            hj, hg = hb & ((1 << q) - 1), hb >> q
            L0 = ((hg << (q + 1) | hj) << cols_log) | cl
            L1 = L0 + (cols << q)
            w = tw[(hj << lt | (col0 + cl)) << (logm - s - 1)]
            u, v = tile[L0], tile[L1]
            if dif:
                tile[L0], tile[L1] = (u + v) % p, (u - v) * w % p
            else:
                v = v * w % p
                tile[L0], tile[L1] = (u + v) % p, (u - v) % p

    if dif:
        q = nst
        while q >= 2:
            pair(q - 2)
            q -= 2
        if q:
            single(0)
    else:
        q = 0
        while q + 1 < nst:
            pair(q)
            q += 2
        if q < nst:
            single(q)


def _tile_index(L, logm, lt, col0):
    cols_log = 2 * lt - logm
    return (L >> cols_log) << lt | (col0 + (L & ((1 << cols_log) - 1)))


def kernel_dif_top(F, src, nrows, logm, lt):
    """one vector, workgroup by workgroup; src may be longer than nrows (what lies behind a row is never read)"""
    assert lt < logm <= 2 * lt
    tw_inv = F.tables(logm)[1]
    y = [None] * (1 << logm)
    for block in range(1 << (logm - lt)):
        col0 = block << (2 * lt - logm)
        idx = [_tile_index(L, logm, lt, col0) for L in range(1 << lt)]
        tile = [src[i] % F.p if i < nrows else 0 for i in idx]
        _top_stages(tile, F.p, tw_inv, logm, lt, col0, True)
        for L, i in enumerate(idx):
            assert y[i] is None
            y[i] = tile[L]
    return y


def kernel_mid(F, x, logm, lt):
    assert lt % 2 == 0 and lt >= 4
    p = F.p
    tw_fwd, tw_inv, scale_rev, _ = F.tables(logm)
    y = list(x)
    lanes = (1 << lt) // 4
    for block in range(1 << (logm - lt)):
        base = block << lt
        tile = y[base:base + (1 << lt)]
        for q in range(lt - 2, 1, -2):
            for t in range(lanes):
                hj, hg, d = t & ((1 << q) - 1), t >> q, 1 << q
                L0 = hg << (q + 2) | hj
                w1, w2a, w2b = tw_inv[hj << (logm - q - 1)], tw_inv[hj << (logm - q - 2)], tw_inv[(hj | d) << (logm - q - 2)]
                x0, x1, x2, x3 = tile[L0], tile[L0 + d], tile[L0 + 2 * d], tile[L0 + 3 * d]
                y0, y2, y1, y3 = (x0 + x2) % p, (x0 - x2) * w2a % p, (x1 + x3) % p, (x1 - x3) * w2b % p
                tile[L0], tile[L0 + d], tile[L0 + 2 * d], tile[L0 + 3 * d] = (y0 + y1) % p, (y0 - y1) * w1 % p, (y2 + y3) % p, (y2 - y3) * w1 % p
        for t in range(lanes):
            L0 = t << 2
            sc = scale_rev[base + L0:base + L0 + 4]
            x0, x1, x2, x3 = tile[L0:L0 + 4]
            y0, y2, y1, y3 = (x0 + x2) % p, (x0 - x2) % p, (x1 + x3) % p, (x1 - x3) * tw_inv[1 << (logm - 2)] % p
            x0, x1, x2, x3 = (y0 + y1) * sc[0] % p, (y0 - y1) * sc[1] % p, (y2 + y3) * sc[2] % p, (y2 - y3) * sc[3] % p
            y0, y1, y2, y3 = (x0 + x1) % p, (x0 - x1) % p, (x2 + x3) % p, (x2 - x3) * tw_fwd[1 << (logm - 2)] % p
            tile[L0], tile[L0 + 2], tile[L0 + 1], tile[L0 + 3] = (y0 + y2) % p, (y0 - y2) % p, (y1 + y3) % p, (y1 - y3) % p
        for q in range(2, lt - 1, 2):
            for t in range(lanes):
                hj, hg, d = t & ((1 << q) - 1), t >> q, 1 << q
                L0 = hg << (q + 2) | hj
                w1, w2a, w2b = tw_fwd[hj << (logm - q - 1)], tw_fwd[hj << (logm - q - 2)], tw_fwd[(hj | d) << (logm - q - 2)]
                x0, x1, x2, x3 = tile[L0], tile[L0 + d], tile[L0 + 2 * d], tile[L0 + 3 * d]
                u = x1 * w1 % p
                y0, y1 = (x0 + u) % p, (x0 - u) % p
                u = x3 * w1 % p
                y2, y3 = (x2 + u) % p, (x2 - u) % p
                u = y2 * w2a % p
                tile[L0], tile[L0 + 2 * d] = (y0 + u) % p, (y0 - u) % p
                u = y3 * w2b % p
                tile[L0 + d], tile[L0 + 3 * d] = (y1 + u) % p, (y1 - u) % p
        y[base:base + (1 << lt)] = tile
    return y


def kernel_dit_top_ab(F, a, b, logm, lt):
    assert lt < logm <= 2 * lt
    tw_fwd, _, _, e_scale = F.tables(logm)
    y = [None] * (1 << logm)
    for block in range(1 << (logm - lt)):
        col0 = block << (2 * lt - logm)
        idx = [_tile_index(L, logm, lt, col0) for L in range(1 << lt)]
        tiles = []
        for x in (a, b):
            tile = [x[i] for i in idx]
            _top_stages(tile, F.p, tw_fwd, logm, lt, col0, False)
            tiles.append(tile)
        for L, i in enumerate(idx):
            assert y[i] is None
            y[i] = tiles[0][L] * tiles[1][L] * e_scale % F.p
    return y
