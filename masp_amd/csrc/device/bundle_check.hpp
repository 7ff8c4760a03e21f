// The consensus pre-checks of a block's bundles on the device: what BatchValidator::check_bundle (masp_proofs/src/sapling/verifier/batch.rs:78-193)
// does per description before it queues a proof or a signature, and the binding verification key of the final check (verifier.rs:20-204,
// sapling/mod.rs:14-38), for every bundle of a block at once (masp_hip_sapling_check_bundles, include/masp_hip.h; k_bundle_check.hip).
// One function per lane of each kernel, over the call's arrays:
//   bc_point_lane    one Jubjub encoding (a cv, rk or epk): jj_decode with the ZIP 216 rules, the small-order test [8] P = O, and the
//                    canonical (u, v) out of Montgomery form;
//   bc_term_lane     one value-balance entry: |value| and its sign from the i128, the asset's generator times 8 times |value|, negated for
//                    values >= 0 (the term bvk ADDS);
//   bc_row_lane      one description: its status byte from its points' and its proof's statuses, and its public-input row;
//   bc_bvk_lane      one bundle: the sum of its descriptions' cv (outputs negated) and of its terms, encoded, and the bundle's status.
// `Proof::read` itself (point_read.hpp, subgroup.hpp) is device-only and lives in k_bundle_check.hip; its three status bytes per proof
// are an input here.  MASP_HD: the same source runs on the CPU in the tests (tests/native/bundle_check_dev.hip).
#pragma once
#include "group_hash.hpp"
#include "jubjub.hpp"

namespace masp {

// a description's status byte: 0, or the first reason that applies, in this order
enum : uint8_t { BC_OK = 0, BC_CV_ENCODING = 1, BC_KEY_ENCODING = 2, BC_PROOF_ENCODING = 3, BC_CV_SMALL_ORDER = 4, BC_KEY_SMALL_ORDER = 5 };
// a bundle's status byte (1 before 2 before 3; among the entries the first failing one decides)
enum : uint8_t { BC_BUNDLE_OK = 0, BC_BUNDLE_DESCRIPTION = 1, BC_BUNDLE_VALUE_RANGE = 2, BC_BUNDLE_ASSET = 3 };
// a point's status between the kernels
enum : uint8_t { BC_PT_OK = 0, BC_PT_ENCODING = 1, BC_PT_SMALL_ORDER = 2 };

constexpr uint32_t BC_SPEND_INPUTS = 7, BC_CONVERT_INPUTS = 3, BC_OUTPUT_INPUTS = 5;

// The arrays of one call.  Words are little-endian 32-bit words of the 32-byte values as they come.  The encodings lie kind after kind:
// spend cv | spend rk | convert cv | output cv | output epk; the proofs' status bytes (three a proof: A, B, C) spends | converts | outputs.
struct BcArgs {
    // in
    const uint32_t* enc;            // n_points x 8
    const uint32_t* spend_anchor;   // n_spends x 8
    const uint32_t* spend_nf;       // n_spends x 8
    const uint32_t* convert_anchor; // n_converts x 8
    const uint32_t* output_cmu;     // n_outputs x 8
    const uint32_t* asset;          // n_balance x 8
    const uint32_t* value;          // n_balance x 4: i128, two's complement
    const uint32_t* offsets;        // (n_bundles + 1) x 4: where each bundle's spends, converts, outputs and entries start in their arrays
    const uint8_t* proof_status;    // (n_spends + n_converts + n_outputs) x 3
    // between the kernels
    uint8_t* pt_status;             // n_points
    uint32_t* pt_uv;                // n_points x 16: canonical u, then canonical v
    JExt* term;                     // n_balance
    uint8_t* term_status;           // n_balance: 0, BC_BUNDLE_VALUE_RANGE or BC_BUNDLE_ASSET
    // out
    uint8_t* status;                // n_spends + n_converts + n_outputs, kind after kind
    uint32_t* spend_inputs;         // n_spends x 7 x 8
    uint32_t* convert_inputs;       // n_converts x 3 x 8
    uint32_t* output_inputs;        // n_outputs x 5 x 8
    uint32_t* bvk;                  // n_bundles x 8
    uint8_t* bundle_status;         // n_bundles
    uint32_t n_spends, n_converts, n_outputs, n_balance, n_bundles;
};

MASP_HD uint32_t bc_n_points(const BcArgs& a) { return 2 * a.n_spends + a.n_converts + 2 * a.n_outputs; }
MASP_HD uint32_t bc_n_descriptions(const BcArgs& a) { return a.n_spends + a.n_converts + a.n_outputs; }
// where a description's points sit among the encodings
MASP_HD uint32_t bc_spend_cv(const BcArgs& a, uint32_t i) { return i; }
MASP_HD uint32_t bc_spend_rk(const BcArgs& a, uint32_t i) { return a.n_spends + i; }
MASP_HD uint32_t bc_convert_cv(const BcArgs& a, uint32_t i) { return 2 * a.n_spends + i; }
MASP_HD uint32_t bc_output_cv(const BcArgs& a, uint32_t i) { return 2 * a.n_spends + a.n_converts + i; }
MASP_HD uint32_t bc_output_epk(const BcArgs& a, uint32_t i) { return 2 * a.n_spends + a.n_converts + a.n_outputs + i; }

// One encoding: its status and, if it decodes, the canonical coordinates (zeros otherwise).
MASP_HD uint8_t bc_point(uint32_t u[8], uint32_t v[8], const uint32_t w[8]) {
    JExt p;
    if (jj_decode(p, w) != JJ_OK) {
#pragma unroll
        for (int k = 0; k < 8; ++k) u[k] = v[k] = 0;
        return BC_PT_ENCODING;
    }
    const Fr cu = fe_from_mont(p.U), cv = fe_from_mont(p.V);   // (Z = 1 as jj_decode leaves it)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        u[k] = cu.v[k];
        v[k] = cv.v[k];
    }
    return jj_is_identity(jj_mul_by_cofactor(p)) ? BC_PT_SMALL_ORDER : BC_PT_OK;
}

MASP_HD void bc_point_lane(const BcArgs& a, uint32_t i) {
    uint32_t w[8], u[8], v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = a.enc[8 * (size_t)i + k];
    a.pt_status[i] = bc_point(u, v, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a.pt_uv[16 * (size_t)i + k] = u[k];
        a.pt_uv[16 * (size_t)i + 8 + k] = v[k];
    }
}

MASP_HD JExt jj_neg(const JExt& p) { return {fe_neg(p.U), p.V, p.Z, fe_neg(p.T)}; }

// One value-balance entry (masp_compute_value_balance, sapling/mod.rs:14-38): out = -sign(value) [|value|] [8] asset_generator(id), the term
// that bvk adds.  val: the i128 as four words.  -> 0, BC_BUNDLE_VALUE_RANGE (i128::MIN has no absolute value) or BC_BUNDLE_ASSET (the
// identifier has no generator); out is the identity then.
MASP_HD uint8_t bc_balance_term(JExt& out, const uint32_t id[8], const uint32_t val[4]) {
    out = jj_identity();
    if (val[0] == 0 && val[1] == 0 && val[2] == 0 && val[3] == 0x80000000u) return BC_BUNDLE_VALUE_RANGE;
    const bool negative = val[3] >> 31;
    uint32_t k[8];
    uint64_t carry = negative ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        carry += negative ? ~val[j] : val[j];
        k[j] = (uint32_t)carry;
        carry >>= 32;
        k[4 + j] = 0;
    }
    JExt g;
    uint32_t digest[8];
    if (!jj_asset_generator(g, digest, id)) return BC_BUNDLE_ASSET;
    const JExt t = jj_mul(jj_mul_by_cofactor(g), k);
    out = negative ? t : jj_neg(t);
    return 0;
}

MASP_HD void bc_term_lane(const BcArgs& a, uint32_t i) {
    uint32_t id[8], val[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) id[k] = a.asset[8 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) val[k] = a.value[4 * (size_t)i + k];
    JExt t;
    a.term_status[i] = bc_balance_term(t, id, val);
    a.term[i] = t;
}

// bellman's multipack::compute_multipacking over the 256 bits of a nullifier, least significant first (verifier.rs:84-91): the low 254 bits,
// then the two that remain
MASP_HD void bc_multipack(uint32_t lo[8], uint32_t hi[8], const uint32_t nf[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        lo[k] = nf[k];
        hi[k] = 0;
    }
    lo[7] &= 0x3fffffffu;
    hi[0] = nf[7] >> 30;
}

// the first reason that applies (key: the rk or epk's status, BC_PT_OK for a convert; proof_bad: `Proof::read` refuses)
MASP_HD uint8_t bc_description_status(uint8_t cv, uint8_t key, bool proof_bad) {
    if (cv == BC_PT_ENCODING) return BC_CV_ENCODING;
    if (key == BC_PT_ENCODING) return BC_KEY_ENCODING;
    if (proof_bad) return BC_PROOF_ENCODING;
    if (cv == BC_PT_SMALL_ORDER) return BC_CV_SMALL_ORDER;
    if (key == BC_PT_SMALL_ORDER) return BC_KEY_SMALL_ORDER;
    return BC_OK;
}

MASP_HD void bc_copy8(uint32_t* dst, const uint32_t* src) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = src[k];
}

// description d of all (spends, then converts, then outputs): its status byte and its row, zeros if the status is not 0
MASP_HD void bc_row_lane(const BcArgs& a, uint32_t d) {
    const uint8_t* ps = a.proof_status + 3 * (size_t)d;
    const bool proof_bad = (ps[0] | ps[1] | ps[2]) != 0;
    uint32_t cv, key = 0, n_rows;
    uint32_t* row;
    bool has_key = true;
    if (d < a.n_spends) {
        cv = bc_spend_cv(a, d);
        key = bc_spend_rk(a, d);
        row = a.spend_inputs + 8 * (size_t)BC_SPEND_INPUTS * d;
        n_rows = BC_SPEND_INPUTS;
    } else if (d < a.n_spends + a.n_converts) {
        const uint32_t i = d - a.n_spends;
        cv = bc_convert_cv(a, i);
        has_key = false;
        row = a.convert_inputs + 8 * (size_t)BC_CONVERT_INPUTS * i;
        n_rows = BC_CONVERT_INPUTS;
    } else {
        const uint32_t i = d - a.n_spends - a.n_converts;
        cv = bc_output_cv(a, i);
        key = bc_output_epk(a, i);
        row = a.output_inputs + 8 * (size_t)BC_OUTPUT_INPUTS * i;
        n_rows = BC_OUTPUT_INPUTS;
    }
    const uint8_t st = bc_description_status(a.pt_status[cv], has_key ? a.pt_status[key] : (uint8_t)BC_PT_OK, proof_bad);
    a.status[d] = st;
    if (st != BC_OK) {
        for (uint32_t k = 0; k < 8 * n_rows; ++k) row[k] = 0;
        return;
    }
    const uint32_t *cvuv = a.pt_uv + 16 * (size_t)cv, *keyuv = a.pt_uv + 16 * (size_t)key;
    if (d < a.n_spends) {   // rk.u, rk.v, cv.u, cv.v, anchor, the nullifier's two chunks (verifier.rs:71-95)
        bc_copy8(row, keyuv);
        bc_copy8(row + 8, keyuv + 8);
        bc_copy8(row + 16, cvuv);
        bc_copy8(row + 24, cvuv + 8);
        bc_copy8(row + 32, a.spend_anchor + 8 * (size_t)d);
        uint32_t nf[8], lo[8], hi[8];
        bc_copy8(nf, a.spend_nf + 8 * (size_t)d);
        bc_multipack(lo, hi, nf);
        bc_copy8(row + 40, lo);
        bc_copy8(row + 48, hi);
    } else if (!has_key) {   // cv.u, cv.v, anchor (verifier.rs:120-128)
        bc_copy8(row, cvuv);
        bc_copy8(row + 8, cvuv + 8);
        bc_copy8(row + 16, a.convert_anchor + 8 * (size_t)(d - a.n_spends));
    } else {   // cv.u, cv.v, epk.u, epk.v, cmu (verifier.rs:151-165)
        bc_copy8(row, cvuv);
        bc_copy8(row + 8, cvuv + 8);
        bc_copy8(row + 16, keyuv);
        bc_copy8(row + 24, keyuv + 8);
        bc_copy8(row + 32, a.output_cmu + 8 * (size_t)(d - a.n_spends - a.n_converts));
    }
}

// the point (u, v) of pt_uv as an extended point: Z = 1, T = u v
MASP_HD JExt bc_affine(const uint32_t* uv) {
    Fr u, v;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        u.v[k] = uv[k];
        v.v[k] = uv[8 + k];
    }
    u = fe_to_mont(u);
    v = fe_to_mont(v);
    return {u, v, fe_one<FrCfg>(), fe_mul(u, v)};
}

// bundle b: sum cv(spends) + sum cv(converts) - sum cv(outputs) + sum terms, encoded (one inversion), and the bundle's status.  After
// bc_row_lane over every description and bc_term_lane over every entry.
MASP_HD void bc_bvk_lane(const BcArgs& a, uint32_t b) {
    const uint32_t *lo = a.offsets + 4 * (size_t)b, *hi = lo + 4;
    uint32_t* out = a.bvk + 8 * (size_t)b;
    const uint32_t base[3] = {0, a.n_spends, a.n_spends + a.n_converts};
    uint8_t st = BC_BUNDLE_OK;
    for (int kind = 0; kind < 3 && st == BC_BUNDLE_OK; ++kind)
        for (uint32_t i = lo[kind]; i < hi[kind]; ++i)
            if (a.status[base[kind] + i] != BC_OK) {
                st = BC_BUNDLE_DESCRIPTION;
                break;
            }
    for (uint32_t i = lo[3]; i < hi[3] && st == BC_BUNDLE_OK; ++i) st = a.term_status[i];
    a.bundle_status[b] = st;
    if (st != BC_BUNDLE_OK) {
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = 0;
        return;
    }
    JExt acc = jj_identity();
    for (uint32_t i = lo[0]; i < hi[0]; ++i) acc = jj_add(acc, bc_affine(a.pt_uv + 16 * (size_t)bc_spend_cv(a, i)));
    for (uint32_t i = lo[1]; i < hi[1]; ++i) acc = jj_add(acc, bc_affine(a.pt_uv + 16 * (size_t)bc_convert_cv(a, i)));
    for (uint32_t i = lo[2]; i < hi[2]; ++i) acc = jj_add(acc, jj_neg(bc_affine(a.pt_uv + 16 * (size_t)bc_output_cv(a, i))));
    for (uint32_t i = lo[3]; i < hi[3]; ++i) acc = jj_add(acc, a.term[i]);
    uint32_t w[8];
    jj_encode(w, acc);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = w[k];
}

}  // namespace masp
