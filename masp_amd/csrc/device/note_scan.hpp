// What the full and the compact note scan do for EVERY (output, ivk) pair, in one copy (k_note_scan.hip: k_ns_trial,
// k_note_scan_compact.hip: k_nsc_trial): the key agreement [8 ivk] epk on wave-uniform digits and the Sapling KDF.  Device only.
#pragma once
#include "blake2b.hpp"
#include "jubjub.hpp"

namespace masp {

// fe_inv (field.hpp) inlined: the out-of-line form takes its operand through scratch and, at 161 VGPRs, would set the kernel's register
// count (a kernel is given the registers of its largest callee)
__device__ __forceinline__ Fr fe_inv_divsteps_inline(const Fr& a) {
    Fr r, r2;
    FeDivsteps<FrCfg>::invert(r.v, a.v);   // (a R)^-1
#pragma unroll
    for (int i = 0; i < 8; ++i) r2.v[i] = FrCfg::R2[i];
    return fe_mul_nc(fe_mul_nc(r, r2), r2);
}

constexpr uint64_t le64_of(const char* s) {
    uint64_t x = 0;
    for (int i = 7; i >= 0; --i) x = (x << 8) | (uint8_t)s[i];
    return x;
}

// key = kdf_sapling(encode([8 k] q), epk) for the ivk k whose digit masks are dg[0..15] (wave-uniform: [0..7] the non-zero digits of its
// plain or signed binary recoding, [8..15] the negative ones), q the decoded epk in Niels form, epk[0..1] the epk's 32 bytes.
// inversion: 0 the divstep inverse, 1 the binary-gcd one (field.hpp), for the one inversion of the encoding.
__device__ __forceinline__ void ns_pair_key(uint32_t key[8], const uint32_t* dg, const JNiels& q, const uint4* __restrict__ epk, int inversion) {
    JExt r = jj_identity();
    bool started = false;
#pragma unroll 1
    for (int w = 7; w >= 0; --w) {
        const uint32_t nz = dg[w], ng = dg[8 + w];
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            if (started) r = jj_dbl(r);
            if ((nz >> b) & 1u) {
                r = jj_add_niels(r, q, (ng >> b) & 1u);   // (the first one adds to the identity: the law is complete)
                started = true;
            }
        }
    }
    r = jj_mul_by_cofactor(r);
    // encode(secret) || epk -> the key
    uint64_t m[16], h[8];
    {
        const Fr zi = inversion == 1 ? fe_inv_bingcd(r.Z) : fe_inv_divsteps_inline(r.Z);
        const Fr u = fe_from_mont(fe_mul(r.U, zi)), v = fe_from_mont(fe_mul(r.V, zi));
        const uint32_t top = v.v[7] | ((u.v[0] & 1u) << 31);
        m[0] = v.v[0] | ((uint64_t)v.v[1] << 32);
        m[1] = v.v[2] | ((uint64_t)v.v[3] << 32);
        m[2] = v.v[4] | ((uint64_t)v.v[5] << 32);
        m[3] = v.v[6] | ((uint64_t)top << 32);
    }
    {
        const uint4 e0 = epk[0], e1 = epk[1];   // (read behind the ladder: eight registers fewer across it)
        m[4] = e0.x | ((uint64_t)e0.y << 32);
        m[5] = e0.z | ((uint64_t)e0.w << 32);
        m[6] = e1.x | ((uint64_t)e1.y << 32);
        m[7] = e1.z | ((uint64_t)e1.w << 32);
    }
#pragma unroll
    for (int i = 8; i < 16; ++i) m[i] = 0;
    blake2b_one_block(h, m, 64, 32, le64_of("MASP__Sa"), le64_of("plingKDF"));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        key[2 * i] = (uint32_t)h[i];
        key[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
}

}  // namespace masp
