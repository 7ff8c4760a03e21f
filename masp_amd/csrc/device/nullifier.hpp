// Nullifiers and note commitments of a wallet's notes on the device (k_nullifier.hip): Note::cmu and Note::nf of
// masp_primitives/src/sapling.rs, host/jubjub.h's note_commitment and nullifier, as steps over a state that lives in global memory
// between the kernels, in the manner of compact_note.hpp:
//   g    = the asset generator of the identifier (cofactor not cleared), g_d = the diversifier's base
//   rcm  = the 32 bytes (lead byte 1, below r_J) | PRF^expand(rseed, [4]) mod r_J (lead byte 2)
//   cm   = PedersenHash(NoteCommitment, repr(g) | value | repr(g_d) | pk_d) + [rcm] G_ncr,  cmu = its affine u
//   rho  = cm + [position] G_nf,  nf = BLAKE2s-256("MASP__nf", nk | repr(rho))
// pk_d and nk go into the hashes as the bytes that came; they are only DECODED (jj_decode: canonical and on the curve), which is what
// masp_host_note_cmu checks of pk_d.  The reference's types make both of them points of the prime-order subgroup; nothing here tests that.
//
// cm and rho are plain sums of table points: the 280 Pedersen summands, up to 63 of the G_ncr table and up to 16 of the G_nf table
// (k 16^w G for k = 1..15, Niels form; a zero digit adds nothing).  The addition is complete, so the order of the terms is free: a note's
// terms are dealt to `lanes` lanes (chunk or window t to lane t mod lanes), each adds its share, and the partial sums are folded with jj_add.  The
// affine result, and so every output byte, does not depend on `lanes`.  MASP_HD: the tests run the same source on the CPU.
#pragma once
#include "group_hash.hpp"
#include "pedersen.hpp"

namespace masp {

constexpr uint32_t NF_NCR_WINDOWS = 63, NF_POS_WINDOWS = 16;   // r_J < 2^252: 63 four-bit digits; a position has 64 bits
constexpr uint32_t NF_NCR_TABLE = NF_NCR_WINDOWS * 15, NF_POS_TABLE = NF_POS_WINDOWS * 15;
constexpr uint32_t NF_TABLE = NF_NCR_TABLE + NF_POS_TABLE;     // Niels points: G_ncr's [window][k - 1], then G_nf's

// a note's status: the first check that fails, in this order
enum : uint8_t { NF_OK = 0, NF_BAD_ASSET = 1, NF_BAD_DIVERSIFIER = 2, NF_BAD_PK_D = 3, NF_BAD_RCM = 4, NF_BAD_NK = 5 };

struct NfState {
    uint32_t msg[PED_NC_MSG_WORDS];   // repr(asset generator) | value | repr(g_d) | pk_d: what the commitment hashes
    uint32_t rcm[8];
    JExt cm;
    uint8_t bad[8];                   // bad[s - 1] != 0: check s failed.  Every check writes its own byte: they run in any order, side by side.
};

// the note's arrays as they come (include/masp_hip.h: masp_hip_sapling_note_nullifiers); 32-byte rows are read as words
struct NfIn {
    const uint32_t* ids;
    const uint64_t* values;
    const uint8_t* diversifiers;
    const uint32_t* pk_ds;
    const uint8_t* leads;
    const uint32_t* rseeds;
    const uint32_t* nks;
    const uint64_t* positions;
};

MASP_HD uint8_t nf_status(const NfState& st) {
    uint8_t s = NF_OK;
#pragma unroll
    for (int i = 4; i >= 0; --i)
        if (st.bad[i]) s = (uint8_t)(i + 1);
    return s;
}

// One group hash per call, so that no caller holds two square roots (group_hash.hpp has the two rules; the decoding and the cofactor's
// three doublings are shared here).
//   which = 0: the asset generator.  The digest IS its encoding: msg[0..7]; bad[0].
//   which = 1: g_d, the cleared point: its encoding to msg[10..17]; the value to msg[8..9]; rcm; bad[1], bad[3].
MASP_HD void nf_parse(NfState& st, const NfIn& in, size_t i, int which) {
    uint32_t m[32], h[8];
    if (which == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            m[k] = in.ids[8 * i + k];
            m[8 + k] = 0;
        }
        blake2s_256(h, m, 32, le32_of("MASP"), le32_of("__v_"));
    } else {
        const uint8_t* d = in.diversifiers + 11 * i;
        gh_first_block(m);
        m[16] = d[0] | (d[1] << 8) | (d[2] << 16) | ((uint32_t)d[3] << 24);
        m[17] = d[4] | (d[5] << 8) | (d[6] << 16) | ((uint32_t)d[7] << 24);
        m[18] = d[8] | (d[9] << 8) | (d[10] << 16);
#pragma unroll
        for (int k = 19; k < 32; ++k) m[k] = 0;
        blake2s_256(h, m, 75, le32_of("MASP"), le32_of("__gd"));
    }
    JExt p;
    bool ok = jj_decode(p, h) == JJ_OK;
    if (!ok) p = jj_identity();
    const JExt c = jj_mul_by_cofactor(p);
    ok = ok && !jj_is_identity(c);   // no generator of small order, no g_d that is the identity
    if (which == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st.msg[k] = h[k];
        st.bad[0] = !ok;
        return;
    }
    uint32_t w[8];
    jj_encode(w, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) st.msg[10 + k] = w[k];
    st.bad[1] = !ok;
    const uint64_t value = in.values[i];
    st.msg[8] = (uint32_t)value;
    st.msg[9] = (uint32_t)(value >> 32);
    const uint32_t lead = in.leads[i];
    uint32_t r[8], rcm[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = in.rseeds[8 * i + k];
    bool rok = lead == 1 || lead == 2;
    if (lead == 2) {
        rseed_scalar(rcm, r, 4);
    } else {
        rok = rok && rj_is_canonical(r);   // jubjub::Fr::from_repr(rcm)
#pragma unroll
        for (int k = 0; k < 8; ++k) rcm[k] = r[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) st.rcm[k] = rok ? rcm[k] : 0u;   // (a refused rcm indexes no table)
    st.bad[3] = !rok;
}

// which = 0: pk_d decodes, bad[2], and its bytes go to msg[18..25]; which = 1: nk decodes, bad[4]
MASP_HD void nf_key(NfState& st, const NfIn& in, size_t i, int which) {
    const uint32_t* src = (which == 0 ? in.pk_ds : in.nks) + 8 * i;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = src[k];
    JExt p;
    const bool ok = jj_decode(p, w) == JJ_OK;
    if (which == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st.msg[18 + k] = w[k];
        st.bad[2] = !ok;
    } else {
        st.bad[4] = !ok;
    }
}

// digit w of a scalar's four-bit digits
MASP_HD uint32_t nf_digit(const uint32_t* k, uint32_t w) { return (k[w >> 3] >> (4 * (w & 7u))) & 15u; }

// r + the share of lane `lane` of `lanes` in [k] G: the windows w = lane, lane + lanes, ... of `windows`, from a table of this file's form
MASP_HD JExt nf_table_sum(JExt r, const JNiels* table, uint32_t windows, const uint32_t* k, uint32_t lane, uint32_t lanes) {
#pragma unroll 1
    for (uint32_t w = lane; w < windows; w += lanes) {
        const uint32_t d = nf_digit(k, w);
        if (d) {
            const JNiels q = table[15 * w + d - 1];
            r = jj_add_niels(r, q, false);
        }
    }
    return r;
}

// the share of lane `lane` of `lanes` in cm: the chunks c = lane, lane + lanes, ... of the 280 Pedersen summands, and its windows of
// [rcm] G_ncr.  ped: the Pedersen Niels table (pedersen.hpp); ncr: the G_ncr windows.
MASP_HD JExt nf_commit_partial(const NfState& st, const JNiels* ped, const JNiels* ncr, uint32_t lane, uint32_t lanes) {
    JExt r = jj_identity();
#pragma unroll 1
    for (uint32_t c = lane; c < PED_NC_CHUNKS; c += lanes) {
        const uint32_t a = ped_nc_bit(st.msg, 3 * c), b = ped_nc_bit(st.msg, 3 * c + 1), neg = ped_nc_bit(st.msg, 3 * c + 2);
        const JNiels q = ped[4 * c + a + 2 * b];
        r = jj_add_niels(r, q, neg != 0);
    }
    return nf_table_sum(r, ncr, NF_NCR_WINDOWS, st.rcm, lane, lanes);   // (the digits straight from the state: no indexed array in registers)
}

#if defined(__HIPCC__)
// the sum of the L partial sums of a lane group (L a power of two, groups aligned in the wave), in every lane of the group; device
// only: the kernels of k_nullifier.hip and k_output_build.hip fold with it
template <int L>
__device__ __forceinline__ JExt nf_fold(JExt r) {
    for (int m = 1; m < L; m <<= 1) {
        JExt o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o.U.v[k] = __shfl_xor(r.U.v[k], m);
            o.V.v[k] = __shfl_xor(r.V.v[k], m);
            o.Z.v[k] = __shfl_xor(r.Z.v[k], m);
            o.T.v[k] = __shfl_xor(r.T.v[k], m);
        }
        r = jj_add(r, o);
    }
    return r;
}
#endif

// the folded sum is cm: kept for the nullifier, and its affine u is cmu
MASP_HD void nf_commit_finish(NfState& st, const JExt& cm, uint32_t cmu[8]) {
    st.cm = cm;
    const Fr u = fe_from_mont(fe_mul(cm.U, fe_inv(cm.Z)));
#pragma unroll
    for (int k = 0; k < 8; ++k) cmu[k] = u.v[k];
}

// the share of lane `lane` of `lanes` in rho = cm + [position] G_nf: lane 0 starts from cm, the sixteen windows are dealt like the
// commitment's.  pos: the G_nf windows.
MASP_HD JExt nf_rho_partial(const NfState& st, const JNiels* pos, uint64_t position, uint32_t lane, uint32_t lanes) {
    JExt r = jj_identity();
    if (lane == 0) r = st.cm;
    const uint32_t k[2] = {(uint32_t)position, (uint32_t)(position >> 32)};
    return nf_table_sum(r, pos, NF_POS_WINDOWS, k, lane, lanes);
}

// nf = BLAKE2s-256("MASP__nf", nk | repr(rho)): 64 bytes, one block
MASP_HD void nf_finish(uint32_t nf[8], const JExt& rho, const uint32_t* nk) {
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = nk[k];
    jj_encode(m + 8, rho);
    blake2s_256(nf, m, 64, le32_of("MASP"), le32_of("__nf"));
}

}  // namespace masp
