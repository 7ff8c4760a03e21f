// Output descriptions without their proofs on the device (k_output_build.hip): what SaplingOutputInfo::build of
// masp_primitives/src/transaction/components/sapling/builder.rs puts around an Output proof, host/host_api.cpp's
// masp_host_sapling_build_outputs, as steps over a state that lives in global memory between the kernels, in the manner of nullifier.hpp:
//   rcm  = the 32 bytes (lead byte 1, below r_J) | PRF^expand(rseed, [4]) mod r_J (lead byte 2)
//   esk  = the given 32 bytes (lead byte 1, below r_J) | PRF^expand(rseed, [5]) mod r_J (lead byte 2)
//   cv   = [value] [8] g + [rcv] G_vcr, g the asset generator;  cmu = nullifier.hpp's, through nf_commit_partial and nf_commit_finish
//   epk  = [esk] g_d,  K_enc = KDF([8 esk] pk_d, epk)
//   enc_ciphertext = ChaCha20-Poly1305(K_enc, lead | d | value | id | rseed | memo): 596 + 16 bytes
//   out_ciphertext = ChaCha20-Poly1305(PRF^ock(ovk, cv, cmu, epk), pk_d | esk), or (r[0:32], r[32:96]) of 96 given bytes without an ovk
// pk_d is only DECODED (canonical and on the curve), as nullifier.hpp does; a zero esk is not refused, as on the host.
// The two ciphertexts are written in 16-byte columns (column c of output o at col[c * stride + o]; a lone row: stride 1), and the memo is
// read from such columns: in the kernels the lanes run along the outputs, so a wave's loads and stores are whole lines.
// MASP_HD: the kernels are wrappers around these functions, and the tests run the same source on the CPU.
#pragma once
#include "chacha20.hpp"
#include "conversion.hpp"
#include "nullifier.hpp"
#include "out_recovery.hpp"

namespace masp {

constexpr uint32_t OB_VCR_WINDOWS = 63, OB_VCR_TABLE = OB_VCR_WINDOWS * 15;   // G_vcr's windows, in the form of nullifier.hpp's tables
constexpr uint32_t OB_ENC_COLS = 39, OB_OUT_COLS = 5, OB_COLS = OB_ENC_COLS + OB_OUT_COLS;   // 612 bytes (three words of padding), 80 bytes
constexpr uint32_t OB_MEMO_COLS = 32, OB_ENC_WORDS = 153, OB_OUT_WORDS = 20, OB_PT_WORDS = 149;

// an output's status: the first check that fails, in this order; 1 to 4 are nullifier.hpp's
enum : uint8_t { OB_OK = 0, OB_BAD_ASSET = 1, OB_BAD_DIVERSIFIER = 2, OB_BAD_PK_D = 3, OB_BAD_RCM = 4, OB_BAD_ESK = 5, OB_BAD_RCV = 6 };

struct ObState {
    NfState nf;            // msg, rcm and bad[0..5] as nullifier.hpp keeps them: nf_commit_partial reads it
    uint32_t esk[8];
    Fr gd_u, gd_v;         // g_d, affine
    Fr pk_u, pk_v;         // pk_d, affine
    JExt vbase;            // [8] g: the value commitment's base
    uint32_t secret[8];    // repr([8 esk] pk_d)
};

// the outputs' arrays as they come (include/masp_hip.h: masp_hip_sapling_build_outputs); 32-byte rows are read as words
struct ObIn {
    const uint32_t* ids;
    const uint64_t* values;
    const uint8_t* diversifiers;
    const uint32_t* pk_ds;
    const uint8_t* leads;
    const uint32_t* rseeds;
    const uint32_t* esks;          // may be null: no lead byte is 1
    const uint32_t* rcvs;
    const uint32_t* ovks;
    const uint8_t* ovk_flags;      // may be null: every ovk is present
    const uint32_t* out_randoms;   // 24 words an output; may be null: no flag is 0
};

MASP_HD uint8_t ob_status(const ObState& st) {
    uint8_t s = OB_OK;
#pragma unroll
    for (int i = 5; i >= 0; --i)
        if (st.nf.bad[i]) s = (uint8_t)(i + 1);
    return s;
}

// One check per call, each writing its own bytes of the state, so that they run side by side and no caller holds two square roots:
//   which = 0: the asset generator: its encoding (the digest) to msg[0..7], [8] g to vbase; bad[0]
//   which = 1: g_d: its affine form, its encoding to msg[10..17], the value to msg[8..9]; bad[1]
//   which = 2: pk_d decodes: its affine form, its bytes to msg[18..25]; bad[2]
//   which = 3: the scalars: rcm, esk, and rcv below r_J; bad[3], bad[4], bad[5]
MASP_HD void ob_parse(ObState& st, const ObIn& in, size_t i, int which) {
    if (which == 3) {
        const uint32_t lead = in.leads[i];
        uint32_t r[8], e[8], rcm[8], esk[8], rcv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            r[k] = in.rseeds[8 * i + k];
            e[k] = in.esks && lead == 1 ? in.esks[8 * i + k] : 0u;
            rcv[k] = in.rcvs[8 * i + k];
        }
        bool rok = lead == 1 || lead == 2, eok = true;
        if (lead == 2) {
            rseed_scalar(rcm, r, 4);
            rseed_scalar(esk, r, 5);
        } else {
            rok = rok && rj_is_canonical(r);                 // jubjub::Fr::from_repr(rcm)
            eok = lead != 1 || rj_is_canonical(e);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                rcm[k] = r[k];
                esk[k] = e[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            st.nf.rcm[k] = rok ? rcm[k] : 0u;                // (a refused rcm indexes no table)
            st.esk[k] = eok ? esk[k] : 0u;
        }
        st.nf.bad[3] = !rok;
        st.nf.bad[4] = !eok;
        st.nf.bad[5] = !rj_is_canonical(rcv);
        return;
    }
    uint32_t h[8];
    if (which == 0) {
        uint32_t m[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            m[k] = in.ids[8 * i + k];
            m[8 + k] = 0;
        }
        blake2s_256(h, m, 32, le32_of("MASP"), le32_of("__v_"));
    } else if (which == 1) {
        const uint8_t* d = in.diversifiers + 11 * i;
        uint32_t m[32];
        gh_first_block(m);
        m[16] = d[0] | (d[1] << 8) | (d[2] << 16) | ((uint32_t)d[3] << 24);
        m[17] = d[4] | (d[5] << 8) | (d[6] << 16) | ((uint32_t)d[7] << 24);
        m[18] = d[8] | (d[9] << 8) | (d[10] << 16);
#pragma unroll
        for (int k = 19; k < 32; ++k) m[k] = 0;
        blake2s_256(h, m, 75, le32_of("MASP"), le32_of("__gd"));
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = in.pk_ds[8 * i + k];
    }
    JExt p;
    bool ok = jj_decode(p, h) == JJ_OK;
    if (!ok) p = jj_identity();
    if (which == 2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st.nf.msg[18 + k] = h[k];
        st.pk_u = p.U;
        st.pk_v = p.V;
        st.nf.bad[2] = !ok;
        return;
    }
    const JExt c = jj_mul_by_cofactor(p);
    ok = ok && !jj_is_identity(c);   // no generator of small order, no g_d that is the identity
    if (which == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st.nf.msg[k] = h[k];
        st.vbase = c;
        st.nf.bad[0] = !ok;
        return;
    }
    const Fr zi = fe_inv(c.Z);
    const Fr u = fe_mul(c.U, zi), v = fe_mul(c.V, zi);
    const Fr uc = fe_from_mont(u), vc = fe_from_mont(v);
#pragma unroll
    for (int k = 0; k < 8; ++k) st.nf.msg[10 + k] = vc.v[k];
    st.nf.msg[17] |= (uc.v[0] & 1u) << 31;
    st.gd_u = u;
    st.gd_v = v;
    st.nf.bad[1] = !ok;
    const uint64_t value = in.values[i];
    st.nf.msg[8] = (uint32_t)value;
    st.nf.msg[9] = (uint32_t)(value >> 32);
}

// cv = [value] [8] g + [rcv] G_vcr as its encoding.  vcr: G_vcr's windows (k 16^w G for k = 1..15, Niels form); rcv below r_J.
MASP_HD void ob_value_commitment(uint32_t cv[8], const ObState& st, const JNiels* vcr, const uint32_t* rcv) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = rcv[i];
    const JExt vb = st.vbase;
    const JExt r = nf_table_sum(cv_mul64(vb, st.nf.msg[8], st.nf.msg[9]), vcr, OB_VCR_WINDOWS, k, 0, 1);
    jj_encode(cv, r);
}

// which = 0: epk = [esk] g_d, its encoding to `epk`; which = 1: the shared secret [8 esk] pk_d, its encoding to the state.
// The scalar differs per lane: jj_mul, as compact_note.hpp's nsc_pkd.
MASP_HD void ob_ladder(ObState& st, uint32_t* epk, int which) {
    uint32_t k[8], w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = st.esk[i];
    const Fr u = which == 0 ? st.gd_u : st.pk_u, v = which == 0 ? st.gd_v : st.pk_v;
    const JExt base = {u, v, fe_one<FrCfg>(), fe_mul(u, v)};
    JExt r = jj_mul(base, k);
    if (which == 1) r = jj_mul_by_cofactor(r);
    jj_encode(w, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) (which == 0 ? epk : st.secret)[i] = w[i];
}

// K_enc = kdf_sapling(secret, epk)
MASP_HD void ob_kdf(uint32_t key[8], const uint32_t* secret, const uint32_t* epk) {
    uint64_t m[16], h[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = or_u64(secret[2 * i], secret[2 * i + 1]);
        m[4 + i] = or_u64(epk[2 * i], epk[2 * i + 1]);
    }
#pragma unroll
    for (int i = 8; i < 16; ++i) m[i] = 0;
    blake2b_one_block(h, m, 64, 32, or_le64_of("MASP__Sa"), or_le64_of("plingKDF"));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        key[2 * i] = (uint32_t)h[i];
        key[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
}

// the first 21 words of the note plaintext, what stands before the memo: lead | d | value | id | rseed
MASP_HD void ob_plaintext_head(uint32_t hdr[21], const ObIn& in, size_t i) {
    const uint8_t* d = in.diversifiers + 11 * i;
    hdr[0] = in.leads[i] | (d[0] << 8) | (d[1] << 16) | ((uint32_t)d[2] << 24);
    hdr[1] = d[3] | (d[4] << 8) | (d[5] << 16) | ((uint32_t)d[6] << 24);
    hdr[2] = d[7] | (d[8] << 8) | (d[9] << 16) | ((uint32_t)d[10] << 24);
    const uint64_t value = in.values[i];
    hdr[3] = (uint32_t)value;
    hdr[4] = (uint32_t)(value >> 32);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        hdr[5 + k] = in.ids[8 * i + k];
        hdr[13 + k] = in.rseeds[8 * i + k];
    }
}

MASP_HD uint32_t ob_word(const uint4& x, uint32_t k) { return k == 0 ? x.x : k == 1 ? x.y : k == 2 ? x.z : x.w; }

// enc_ciphertext under `key`: ChaCha20 block 0 for the Poly1305 key, blocks 1 to 10 over the 149 plaintext words, 38 Poly1305 blocks of
// ciphertext (the last one a word and the AEAD's padding) and the lengths.  hdr: ob_plaintext_head; memo: the memo's column 0 (column c at
// memo[c * mstride]), or null for the empty memo (0xf6, then zeros).  enc: the ciphertext's column 0, 39 columns, the tag in words 149..152.
// Plaintext word 21 + m is memo word m: for ChaCha20 block j, word k of the block is memo word 16 j - 37 + k, component (k + 3) % 4 of
// memo column 4 j - 10 + (k + 3) / 4.
MASP_HD void ob_seal_enc(const uint32_t key[8], const uint32_t hdr[21], const uint4* memo, size_t mstride, uint4* enc, size_t estride) {
    const uint32_t nonce[3] = {0, 0, 0};
    Poly1305State st;
    uint32_t pad[4];
    {
        uint32_t b0[16];
        chacha20_block(b0, key, 0, nonce);
        poly1305_init(st, b0);
#pragma unroll
        for (int i = 0; i < 4; ++i) pad[i] = b0[4 + i];
    }
#pragma unroll 1
    for (uint32_t j = 1; j <= 10; ++j) {
        uint32_t c[16];
        {
            uint4 mc[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const int col = 4 * (int)j - 10 + q;
                mc[q] = make_uint4(0u, 0u, 0u, 0u);
                if (col >= 0 && col < (int)OB_MEMO_COLS) {
                    if (memo)
                        mc[q] = memo[(size_t)col * mstride];
                    else if (col == 0)
                        mc[q].x = 0xf6u;
                }
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                uint32_t w = ob_word(mc[(k + 3) >> 2], (k + 3) & 3);
                if (j == 1) w = hdr[k];
                if (j == 2 && k < 5) w = hdr[16 + k];
                c[k] = w;
            }
        }
        {
            uint32_t ks[16];
            chacha20_block(ks, key, j, nonce);
#pragma unroll
            for (int k = 0; k < 16; ++k) c[k] ^= ks[k];
        }
        if (j < 10) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                poly1305_block(st, c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
                enc[(size_t)(4 * (j - 1) + q) * estride] = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
            }
        } else {   // words 144..148 are the plaintext's last; the tag follows them
            poly1305_block(st, c[0], c[1], c[2], c[3]);
            enc[(size_t)36 * estride] = make_uint4(c[0], c[1], c[2], c[3]);
            poly1305_block(st, c[4], 0, 0, 0);            // pad16: zeros up to the block's end
            poly1305_block(st, 0, 0, 4 * OB_PT_WORDS, 0);   // the lengths: no associated data, 596 bytes of ciphertext
            uint32_t tag[4];
            poly1305_finish(st, pad, tag);
            enc[(size_t)37 * estride] = make_uint4(c[4], tag[0], tag[1], tag[2]);
            enc[(size_t)38 * estride] = make_uint4(tag[3], 0u, 0u, 0u);
        }
    }
}

// out_ciphertext = ChaCha20-Poly1305(ock, op) over the 64 bytes op, as five columns (the tag the last).  With an ovk: ock = PRF^ock(ovk, cv,
// cmu, epk) (one BLAKE2b compression of a full block), op = pk_d | esk.  Without: ock | op are the 24 words `random`.
MASP_HD void ob_seal_out(bool have_ovk, const uint32_t* ovk, const uint32_t* cv, const uint32_t* cmu, const uint32_t* epk, const uint32_t* pk_d,
                         const uint32_t* esk, const uint32_t* random, uint4* out, size_t ostride) {
    uint32_t ock[8], op[16];
    if (have_ovk) {
        uint64_t m[16], h[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            m[i] = or_u64(ovk[2 * i], ovk[2 * i + 1]);
            m[4 + i] = or_u64(cv[2 * i], cv[2 * i + 1]);
            m[8 + i] = or_u64(cmu[2 * i], cmu[2 * i + 1]);
            m[12 + i] = or_u64(epk[2 * i], epk[2 * i + 1]);
        }
        blake2b_one_block(h, m, 128, 32, or_le64_of("MASP__De"), or_le64_of("rive_ock"));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ock[2 * i] = (uint32_t)h[i];
            ock[2 * i + 1] = (uint32_t)(h[i] >> 32);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            op[i] = pk_d[i];
            op[8 + i] = esk[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) ock[i] = random[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) op[i] = random[8 + i];
    }
    const uint32_t nonce[3] = {0, 0, 0};
    uint32_t b0[16], ks[16];
    chacha20_block(b0, ock, 0, nonce);
    chacha20_block(ks, ock, 1, nonce);
    Poly1305State st;
    poly1305_init(st, b0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 x = make_uint4(op[4 * q] ^ ks[4 * q], op[4 * q + 1] ^ ks[4 * q + 1], op[4 * q + 2] ^ ks[4 * q + 2], op[4 * q + 3] ^ ks[4 * q + 3]);
        poly1305_block(st, x.x, x.y, x.z, x.w);
        out[(size_t)q * ostride] = x;
    }
    poly1305_block(st, 0, 0, 64, 0);   // the lengths: no associated data, 64 bytes of ciphertext
    uint32_t tag[4];
    poly1305_finish(st, b0 + 4, tag);
    out[(size_t)4 * ostride] = make_uint4(tag[0], tag[1], tag[2], tag[3]);
}

// The seal step of output i: the KDF, enc_ciphertext and out_ciphertext.  cv, cmu, epk: the output's eight words each, as the steps before
// left them; cols: column 0 of the output's 44 (enc_ciphertext's 39, then out_ciphertext's 5).
MASP_HD void ob_seal(const ObState& st, const ObIn& in, size_t i, const uint32_t* cv, const uint32_t* cmu, const uint32_t* epk, const uint4* memo,
                     size_t mstride, uint4* cols, size_t stride) {
    uint32_t key[8], hdr[21];
    ob_kdf(key, st.secret, epk);
    ob_plaintext_head(hdr, in, i);
    ob_seal_enc(key, hdr, memo, mstride, cols, stride);
    const bool have_ovk = !in.ovk_flags || in.ovk_flags[i] != 0;
    ob_seal_out(have_ovk, in.ovks + 8 * i, cv, cmu, epk, in.pk_ds + 8 * i, st.esk, have_ovk ? nullptr : in.out_randoms + 24 * i,
                cols + (size_t)OB_ENC_COLS * stride, stride);
}

}  // namespace masp
