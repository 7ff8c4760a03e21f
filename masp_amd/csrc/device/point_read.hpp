// Compressed zcash / bellman point encodings -> affine points on the device: the square roots in Fp and Fp2 and the two readers with
// `Proof::read`'s refusals (PT_* of io.hpp).  Shared by the Groth16 verifier's kernels (pairing.hpp) and the bundle pre-check
// (k_bundle_check.hip); no kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "io.hpp"

namespace masp {

// ---- square roots / decompression ---------------------------------------------------------------------------
// p = 3 mod 4: a^((p+1)/4) is a square root of a if one exists
__device__ inline bool fp_sqrt(const Fp& a, Fp& out) {
    uint32_t e[12];
    uint64_t carry = 1;  // (p + 1) / 4 = (p >> 2) + 1 because p = 3 mod 4
    for (int i = 0; i < 12; ++i) {
        uint32_t w = (FpCfg::MOD[i] >> 2) | (i < 11 ? FpCfg::MOD[i + 1] << 30 : 0u);
        carry += w;
        e[i] = (uint32_t)carry;
        carry >>= 32;
    }
    Fp r = fe_pow(a, e, 12);
    out = r;
    return fe_eq(fe_sqr_nc(r), a);
}
__device__ inline bool fp2_sqrt(const Fp2& v, Fp2& out) {  // host/pairing.h Fp2::sqrt
    if (Fp2Ops::is_zero(v)) {
        out = v;
        return true;
    }
    if (fe_is_zero(v.c1)) {
        Fp s;
        if (fp_sqrt(v.c0, s)) {
            out = {s, fe_zero<FpCfg>()};
            return true;
        }
        if (fp_sqrt(fe_neg(v.c0), s)) {
            out = {fe_zero<FpCfg>(), s};
            return true;
        }
        return false;
    }
    Fp n;
    if (!fp_sqrt(fe_add(fe_sqr_nc(v.c0), fe_sqr_nc(v.c1)), n)) return false;
    Fp two = fe_dbl(fe_one<FpCfg>());
    Fp half = fe_inv_fermat(two);
    Fp d = fe_mul_nc(fe_add(v.c0, n), half), x0;
    if (!fp_sqrt(d, x0)) {
        d = fe_mul_nc(fe_sub(v.c0, n), half);
        if (!fp_sqrt(d, x0)) return false;
    }
    Fp x1 = fe_mul_nc(v.c1, fe_inv_fermat(fe_dbl(x0)));
    out = {x0, x1};
    return Fp2Ops::eq(Fp2Ops::sqr(out), v);
}
// subgroup membership of G1 / G2 points (g1_in_subgroup, g2_in_subgroup): device/subgroup.hpp
// the encoding of the point at infinity: compression and infinity flags, nothing else (bellman rejects stray bits)
__device__ inline bool infinity_encoding_is_clean(const uint8_t* in, int len) {
    if ((in[0] & 0x3f) != 0) return false;
    uint32_t acc = 0;
    for (int i = 1; i < len; ++i) acc |= in[i];
    return acc == 0;
}

// zcash compressed encodings -> affine (Montgomery).  PT_* status; PT_BAD_FLAGS also for "not on the curve"
__device__ inline int g1_read_compressed(const uint8_t* in, G1Affine& p) {
    if (!(in[0] & 0x80)) return PT_BAD_FLAGS;
    if (in[0] & 0x40) {
        p.x = fe_zero<FpCfg>();
        p.y = fe_zero<FpCfg>();
        return infinity_encoding_is_clean(in, 48) ? PT_INFINITY : PT_BAD_FLAGS;
    }
    uint8_t t[48];
    for (int i = 0; i < 48; ++i) t[i] = in[i];
    const bool big = t[0] & 0x20;
    t[0] &= 0x1f;
    Fp xc = fe_load_be<FpCfg>(t);
    if (fe_canonical_ge_mod(xc)) return PT_NOT_CANONICAL;
    p.x = fe_to_mont(xc);
    Fp four = fe_dbl(fe_dbl(fe_one<FpCfg>()));
    Fp rhs = fe_add(fe_mul_nc(fe_sqr_nc(p.x), p.x), four);
    if (!fp_sqrt(rhs, p.y)) return PT_BAD_FLAGS;
    if (fe_canonical_gt_half(fe_from_mont(p.y)) != big) p.y = fe_neg(p.y);
    return PT_OK;
}
__device__ inline int g2_read_compressed(const uint8_t* in, G2Affine& p) {
    if (!(in[0] & 0x80)) return PT_BAD_FLAGS;
    if (in[0] & 0x40) {
        p.x = Fp2Ops::zero();
        p.y = Fp2Ops::zero();
        return infinity_encoding_is_clean(in, 96) ? PT_INFINITY : PT_BAD_FLAGS;
    }
    uint8_t t[96];
    for (int i = 0; i < 96; ++i) t[i] = in[i];
    const bool big = t[0] & 0x20;
    t[0] &= 0x1f;
    Fp x1 = fe_load_be<FpCfg>(t), x0 = fe_load_be<FpCfg>(t + 48);
    if (fe_canonical_ge_mod(x0) || fe_canonical_ge_mod(x1)) return PT_NOT_CANONICAL;
    p.x = {fe_to_mont(x0), fe_to_mont(x1)};
    Fp four = fe_dbl(fe_dbl(fe_one<FpCfg>()));
    Fp2 rhs = Fp2Ops::add(Fp2Ops::mul(Fp2Ops::sqr(p.x), p.x), Fp2{four, four});  // y^2 = x^3 + 4 (1 + u)
    if (!fp2_sqrt(rhs, p.y)) return PT_BAD_FLAGS;
    const Fp y1 = fe_from_mont(p.y.c1);
    const bool lg = fe_is_zero(y1) ? fe_canonical_gt_half(fe_from_mont(p.y.c0)) : fe_canonical_gt_half(y1);
    if (lg != big) p.y = Fp2Ops::neg(p.y);
    return PT_OK;
}

}  // namespace masp
