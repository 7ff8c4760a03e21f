// Stage 2 of the compact note scan (k_note_scan_compact.hip), what is done for a candidate pair once its symmetric key is known, as four
// steps over a state that lives in global memory between them: try_compact_note_decryption_inner of masp_note_encryption/src/lib.rs:607-624
// with sapling_parse_note_plaintext_without_memo and check_note_validity (masp_primitives/src/sapling/note_encryption.rs), in the order of
// host/note_encryption.h's check_note_plaintext.  Each step returns false where the reference returns None.  MASP_HD: the kernels are
// wrappers around these functions, and the tests run the same source on the CPU.
#pragma once
#include "chacha20.hpp"
#include "group_hash.hpp"
#include "pedersen.hpp"

namespace masp {

constexpr uint32_t NSC_ENC_WORDS = 21;   // 84 bytes: lead byte | diversifier 11 | value 8 | asset identifier 32 | rcm or rseed 32

struct NscState {
    uint32_t pt[NSC_ENC_WORDS];       // the decrypted note plaintext without memo
    uint32_t msg[PED_NC_MSG_WORDS];   // repr(asset generator) | value | repr(g_d) | repr(pk_d): what the commitment hashes
    Fr gd_u, gd_v;                    // g_d, affine
};

// decrypts the 84 bytes at `row` (ChaCha20 blocks 1 and 2 under `key`), parses them: the lead byte, AssetType::from_identifier, a canonical
// rcm for lead byte 1, diversifier.g_d() with its affine form and encoding.  Writes st.pt, st.msg[0..17], st.gd_*.
MASP_HD bool nsc_parse(NscState& st, const uint32_t key[8], const uint32_t* row, int lead) {
    uint32_t pt[NSC_ENC_WORDS];
    {
        const uint32_t nonce[3] = {0, 0, 0};
        uint32_t ks[16];
        chacha20_block(ks, key, 1, nonce);
#pragma unroll
        for (int i = 0; i < 16; ++i) pt[i] = row[i] ^ ks[i];
        chacha20_block(ks, key, 2, nonce);
#pragma unroll
        for (int i = 16; i < 21; ++i) pt[i] = row[i] ^ ks[i - 16];
    }
    if ((pt[0] & 0xffu) != (uint32_t)lead) return false;
    uint32_t msg[18];
    JExt p;
    if (!jj_asset_generator(p, msg, pt + 5)) return false;           // AssetType::from_identifier
    if (lead == 1 && !rj_is_canonical(pt + 13)) return false;        // jubjub::Fr::from_repr(rcm)
    const uint32_t d[3] = {(pt[0] >> 8) | (pt[1] << 24), (pt[1] >> 8) | (pt[2] << 24), pt[2] >> 8};
    if (!jj_group_hash_gd(p, d)) return false;                       // diversifier.g_d()
    const Fr zi = fe_inv(p.Z);
    const Fr u = fe_mul(p.U, zi), v = fe_mul(p.V, zi);
    {
        const Fr uc = fe_from_mont(u), vc = fe_from_mont(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) msg[10 + i] = vc.v[i];
        msg[17] |= (uc.v[0] & 1u) << 31;
    }
    msg[8] = pt[3];
    msg[9] = pt[4];
#pragma unroll
    for (int i = 0; i < 21; ++i) st.pt[i] = pt[i];
#pragma unroll
    for (int i = 0; i < 18; ++i) st.msg[i] = msg[i];
    st.gd_u = u;
    st.gd_v = v;
    return true;
}

MASP_HD JExt nsc_gd(const NscState& st) {
    const Fr u = st.gd_u, v = st.gd_v;
    return {u, v, fe_one<FrCfg>(), fe_mul(u, v)};
}

// pk_d = [ivk] g_d, refused if it is the identity (PaymentAddress::from_parts); writes its encoding to st.msg[18..25]
MASP_HD bool nsc_pkd(NscState& st, const uint32_t* ivk) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ivk[i];
    const JExt pk = jj_mul(nsc_gd(st), k);
    if (jj_is_identity(pk)) return false;
    uint32_t w[8];
    jj_encode(w, pk);
#pragma unroll
    for (int i = 0; i < 8; ++i) st.msg[18 + i] = w[i];
    return true;
}

// the note commitment's u against cmu.  table: the Pedersen Niels table with G_ncr (a JExt) behind it.
MASP_HD bool nsc_commit(const NscState& st, const JNiels* table, const uint32_t* cmu, int lead) {
    uint32_t r[8], rcm[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = st.pt[13 + i];
    if (lead == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) rcm[i] = r[i];
    } else {
        rseed_scalar(rcm, r, 4);
    }
    const JExt g_ncr = *(const JExt*)(table + PED_NC_TABLE);
    uint32_t got[8];
    note_commit_u(got, table, g_ncr, st.msg, rcm);
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) same = same && got[i] == cmu[i];
    return same;
}

// ZIP 212: the ephemeral key the rseed implies, [esk] g_d, against epk
MASP_HD bool nsc_esk(const NscState& st, const uint32_t* epk) {
    uint32_t r[8], esk[8], w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = st.pt[13 + i];
    rseed_scalar(esk, r, 5);
    jj_encode(w, jj_mul(nsc_gd(st), esk));
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) same = same && w[i] == epk[i];
    return same;
}

}  // namespace masp
