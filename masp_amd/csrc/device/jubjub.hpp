// Jubjub on the device: the twisted Edwards curve  -u^2 + v^2 = 1 + d u^2 v^2,  d = -10240/10241, over the BLS12-381 scalar field
// (Fe<FrCfg>, Montgomery form), in extended coordinates (U : V : Z : T) with T = U V / Z.  The device form of host/jubjub.h's JPoint
// (same formulas, same encoding rules) for the RedJubjub batch verifier (k_redjubjub.hip).
//
// Group law: the unified addition add-2008-hwcd-3 for a = -1 with k = 2d.  The affine law behind it is complete on Jubjub because
// a = -1 is a square and d a non-square in Fr (tests/test_verifier_host.py checks both), so one formula serves P + Q, P + P, the
// identity and the small-order points alike.  Doublings use the dedicated a = -1 doubling (dbl-2008-hwcd), which agrees with it.
#pragma once
#include "field.hpp"

namespace masp {

struct JubjubCfg {
    static constexpr uint32_t D[8] = {0xb974f6b0u, 0x2a522455u, 0x0d9acab3u, 0xfc6cc9efu, 0xc27628d1u, 0x7a08fb94u, 0xfe0e262eu, 0x57f8f6a8u};    // d, Montgomery form
    static constexpr uint32_t D2[8] = {0x72e9ed5fu, 0x54a448acu, 0x1b373967u, 0xa51befdbu, 0x7b4a799eu, 0xc0d81f21u, 0xd27ecf14u, 0x3c0445feu};   // 2d, Montgomery form
    // Tonelli-Shanks: r - 1 = 2^32 t with t odd; (t - 1) / 2 as a plain integer (FrCfg::ROOT_OF_UNITY = 7^t has order 2^32)
    static constexpr uint32_t SQRT_EXP[8] = {0x7fffffffu, 0x7fff2dffu, 0xa9ded201u, 0x04d0ec02u, 0x199cec04u, 0x94cebea4u, 0x39f6d3a9u, 0x00000000u};
    static constexpr int TWO_ADICITY = 32;
};

// r_J, the order of Jubjub's prime-order subgroup, as a modulus of field.hpp (Fe<RjCfg>: k_redjubjub.hip's host-side scalar arithmetic)
struct RjCfg {
    static constexpr int N = 8;
    static constexpr uint32_t MOD[8] = {0xd6f72cb7u, 0xd0970e5eu, 0xccc81082u, 0xa6682093u, 0x01343b00u, 0x06673b01u, 0x6533afa9u, 0x0e7db4eau};
    static constexpr uint32_t R2[8] = {0x95e57731u, 0x67719aa4u, 0x9ce3fc26u, 0x51b0cef0u, 0xc026e9a5u, 0x69dab7fau, 0x8d127688u, 0x04f6547bu};   // 2^512 mod r_J
    static constexpr uint32_t INV = 0xef788ef9u;   // -r_J^-1 mod 2^32
};

// a < r_J as eight little-endian words (jubjub::Fr::from_repr accepts exactly these)
MASP_HD bool rj_is_canonical(const uint32_t a[8]) {
    bool lt = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        if (!decided && a[i] != RjCfg::MOD[i]) {
            lt = a[i] < RjCfg::MOD[i];
            decided = true;
        }
    }
    return lt;
}

struct JExt {
    Fr U, V, Z, T;
};

// decoding results (JPoint::from_bytes refuses the same three cases)
enum : int { JJ_OK = 0, JJ_NOT_CANONICAL = 1, JJ_NOT_ON_CURVE = 2, JJ_NEGATIVE_ZERO = 3 };

MASP_HD Fr fr_lit(const uint32_t* limbs) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = limbs[i];
    return r;
}

MASP_HD JExt jj_identity() {
    const Fr one = fe_one<FrCfg>(), zero = fe_zero<FrCfg>();
    return {zero, one, one, zero};
}

// p + q (complete: see the head of this file).  9 products.
MASP_HD JExt jj_add(const JExt& p, const JExt& q) {
    const Fr A = fe_mul(fe_sub(p.V, p.U), fe_sub(q.V, q.U));
    const Fr B = fe_mul(fe_add(p.V, p.U), fe_add(q.V, q.U));
    const Fr C = fe_mul(fe_mul(p.T, fr_lit(JubjubCfg::D2)), q.T);
    const Fr D = fe_dbl(fe_mul(p.Z, q.Z));
    const Fr E = fe_sub(B, A), F = fe_sub(D, C), G = fe_add(D, C), H = fe_add(B, A);
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

// an affine point as (v - u, v + u, 2 d u v): the second operand of a mixed addition
struct JNiels {
    Fr vmu, vpu, t2d;
};

// p + q (negated if `negate`), q affine in Niels form: 7 products.  (`negate` is wave-uniform in the note scan's ladder.)
MASP_HD JExt jj_add_niels(const JExt& p, const JNiels& q, bool negate) {
    const Fr A = fe_mul(fe_sub(p.V, p.U), negate ? q.vpu : q.vmu);
    const Fr B = fe_mul(fe_add(p.V, p.U), negate ? q.vmu : q.vpu);
    Fr C = fe_mul(p.T, q.t2d);
    if (negate) C = fe_neg(C);
    const Fr D = fe_dbl(p.Z);
    const Fr E = fe_sub(B, A), F = fe_sub(D, C), G = fe_add(D, C), H = fe_add(B, A);
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

// 2p for a = -1: 4 squarings + 4 products (= jj_add(p, p))
MASP_HD JExt jj_dbl(const JExt& p) {
    const Fr A = fe_sqr(p.U), B = fe_sqr(p.V), C = fe_dbl(fe_sqr(p.Z));
    const Fr E = fe_sub(fe_sub(fe_sqr(fe_add(p.U, p.V)), A), B), G = fe_sub(B, A), F = fe_sub(G, C), H = fe_neg(fe_add(A, B));
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

MASP_HD JExt jj_mul_by_cofactor(const JExt& p) { return jj_dbl(jj_dbl(jj_dbl(p))); }

MASP_HD bool jj_is_identity(const JExt& p) { return fe_is_zero(p.U) && fe_eq(p.V, p.Z); }

// [k] p, k = a 256-bit little-endian integer in eight words (any value: k >= r_J is fine).  Left-to-right double-and-add with the
// scalar held in registers and shifted out at the top (a runtime-indexed array would live in scratch, and so would a window table);
// doublings start at the lane's top set bit, so a wave of 128-bit scalars does 128 of them.
MASP_HD JExt jj_mul(const JExt& p, const uint32_t* k_in) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = k_in[i];
    JExt r = jj_identity();
    bool started = false;
    for (int i = 0; i < 256; ++i) {
        const bool bit = k[7] >> 31;
#pragma unroll
        for (int w = 7; w > 0; --w) k[w] = (k[w] << 1) | (k[w - 1] >> 31);
        k[0] <<= 1;
        if (started) r = jj_dbl(r);
        if (bit) {
            r = started ? jj_add(r, p) : p;
            started = true;
        }
    }
    return r;
}

// a^((t-1)/2): the exponent is a compile-time constant, shifted out of registers like jj_mul's scalar
MASP_HD Fr fr_pow_sqrt_exp(const Fr& a) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = JubjubCfg::SQRT_EXP[i];
    Fr r = fe_one<FrCfg>();
    for (int i = 0; i < 256; ++i) {
        const bool bit = e[7] >> 31;
#pragma unroll
        for (int w = 7; w > 0; --w) e[w] = (e[w] << 1) | (e[w - 1] >> 31);
        e[0] <<= 1;
        r = fe_sqr(r);
        if (bit) r = fe_mul(r, a);
    }
    return r;
}

// square root in Fr by Tonelli-Shanks (2-adicity 32); false for a non-square.  Which of the two roots comes out does not matter: the
// caller fixes the sign.
MASP_HD bool fr_sqrt(Fr& out, const Fr& a) {
    if (fe_is_zero(a)) {
        out = a;
        return true;
    }
    const Fr one = fe_one<FrCfg>();
    const Fr w = fr_pow_sqrt_exp(a);   // a^((t-1)/2)
    Fr x = fe_mul(a, w);               // a^((t+1)/2)
    Fr b = fe_mul(x, w);               // a^t; invariant x^2 = a b
    Fr z = fr_lit(FrCfg::ROOT_OF_UNITY);
    int m = JubjubCfg::TWO_ADICITY;
    while (!fe_eq(b, one)) {
        // least k with b^(2^k) = 1 (b^(2^32) = a^(r-1) = 1); k = m means b^(2^(m-1)) = -1: a is not a square
        int k = 0;
        Fr b2k = b;
        do {
            b2k = fe_sqr(b2k);
            ++k;
        } while (!fe_eq(b2k, one) && k < m);
        if (k >= m) return false;
        Fr j = z;
        for (int i = 0; i < m - k - 1; ++i) j = fe_sqr(j);
        z = fe_sqr(j);
        x = fe_mul(x, j);
        b = fe_mul(b, z);
        m = k;
    }
    out = x;
    return true;
}

// JPoint::from_bytes (host/jubjub.h) bit for bit: v = the low 255 bits (refused if >= r), the top bit the sign (parity) of u,
// u^2 = (v^2 - 1) / (d v^2 + 1) (the denominator never vanishes: -1/d is a non-square), refused if that is a non-square, and u = 0
// with the sign bit set refused (ZIP 216).  w: the encoding as eight little-endian words.
MASP_HD int jj_decode(JExt& out, const uint32_t* w) {
    Fr v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v.v[i] = w[i];
    const uint32_t sign = w[7] >> 31;
    v.v[7] &= 0x7fffffffu;
    if (fe_canonical_ge_mod(v)) return JJ_NOT_CANONICAL;
    v = fe_to_mont(v);
    const Fr one = fe_one<FrCfg>();
    const Fr v2 = fe_sqr(v);
    const Fr u2 = fe_mul(fe_sub(v2, one), fe_inv(fe_add(fe_mul(fr_lit(JubjubCfg::D), v2), one)));
    Fr u;
    if (!fr_sqrt(u, u2)) return JJ_NOT_ON_CURVE;
    if ((fe_from_mont(u).v[0] & 1u) != sign) u = fe_neg(u);
    if (fe_is_zero(u) && sign) return JJ_NEGATIVE_ZERO;
    out = {u, v, one, fe_mul(u, v)};
    return JJ_OK;
}

// the 32-byte encoding (JPoint::to_bytes) as eight little-endian words: v with the parity of u in bit 255
MASP_HD void jj_encode(uint32_t* w, const JExt& p) {
    const Fr zi = fe_inv(p.Z);
    const Fr u = fe_from_mont(fe_mul(p.U, zi)), v = fe_from_mont(fe_mul(p.V, zi));
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = v.v[i];
    w[7] |= (u.v[0] & 1u) << 31;
}

}  // namespace masp
