// Spend descriptions without their proofs, and RedJubjub signatures, on the device (k_spend_build.hip): what the builder of
// masp_primitives/src/transaction/components/sapling/builder.rs puts around a Spend proof, and spend_sig_internal (sapling.rs:167-195)
// over redjubjub.rs:121-160, host/host_api.cpp's masp_host_sapling_build_spends and masp_host_redjubjub_sign_batch, as steps over a state
// that lives in global memory between the kernels, in the manner of nullifier.hpp and output_build.hpp:
//   nk   = [nsk] G_pgk,  rk = ak + [ar] G_spend,  cv = [value] [8] g + [rcv] G_vcr (output_build.hpp's),
//   cmu, nf = nullifier.hpp's, with nk taken from the state
//   rsk  = sk + alpha mod r_J,  vk = [rsk] G_kind,  r = H*(T | vk | sighash),  Rbar = repr([r] G_kind),
//   S    = r + H*(Rbar | vk | sighash) rsk mod r_J;  H* = BLAKE2b-512 personalised "MASP__RedJubjubH", reduced mod r_J
// ak is decoded (canonical and on the curve) and [8] ak must not be the identity, which is what the Spend circuit asserts; whether ak lies
// in the prime-order subgroup is not tested.  rsk = 0 is not refused: the reference signs with it, and vk is then the identity's encoding.
// MASP_HD: the kernels are wrappers around these functions, and the tests run the same source on the CPU.
#pragma once
#include "output_build.hpp"

namespace masp {

constexpr uint32_t SB_WINDOWS = 63, SB_BASE_TABLE = SB_WINDOWS * 15;   // a basepoint's windows, in the form of nullifier.hpp's tables
constexpr uint32_t SB_TABLE = 2 * SB_BASE_TABLE;                       // G_spend's [window][k - 1], then G_pgk's

// [k] G from G's windows (k 16^w G for k = 1..15, Niels form; 63 windows): k a plain integer below 2^252 in eight words.  A zero digit
// adds nothing; otherwise no digit is special.
MASP_HD JExt fixed_base_mul(const JNiels* table, const uint32_t* k) { return nf_table_sum(jj_identity(), table, SB_WINDOWS, k, 0, 1); }

// ---- arithmetic mod r_J ----
using Rj = Fe<RjCfg>;
struct RjConst {
    static constexpr uint32_t R1[8] = {0xb99607d9u, 0x25f80bb3u, 0x66b6e750u, 0xf315d62fu, 0xeb8814f4u, 0x932514eeu, 0x479155c6u, 0x09a6fc6fu};   // 2^256 mod r_J
};

MASP_HD Rj rj_load(const uint32_t* w) {
    Rj r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = w[i];
    return r;
}

// jubjub::Fr::from_bytes_wide: the 512-bit little-endian integer lo + 2^256 hi in in[0..15] mod r_J, as two Montgomery products by
// constants: mont(R mod r_J, lo) = lo and mont(R^2 mod r_J, hi) = hi R (mod r_J), R = 2^256.  A product a b with a < r_J and b < R is
// inside Montgomery's bound a b < r_J R, so the raw halves go in unreduced (as the second operand: the host form of fe_mul keeps its
// running value below 2 r_J for a first operand below r_J and any second).  Same values as pedersen.hpp's rj_from_bytes_wide.
MASP_HD void rj_reduce_wide(uint32_t out[8], const uint32_t in[16]) {
    const Rj lo = fe_mul(rj_load(RjConst::R1), rj_load(in)), hi = fe_mul(rj_load(RjCfg::R2), rj_load(in + 8));
    const Rj s = fe_add(lo, hi);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s.v[i];
}

// r + c k mod r_J, all three plain and below r_J
MASP_HD void rj_mul_add(uint32_t out[8], const uint32_t* r, const uint32_t* c, const uint32_t* k) {
    const Rj ck = fe_mul(fe_mul(rj_load(RjCfg::R2), rj_load(c)), rj_load(k));   // (c R) k / R
    const Rj s = fe_add(rj_load(r), ck);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s.v[i];
}

// ---- BLAKE2b-512 of more than one block (blake2b.hpp has the one-block form and the rounds) ----
MASP_HD void b2b_start(uint64_t h[8], uint32_t outlen, uint64_t personal0, uint64_t personal1) {
    const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                            0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = iv[i];
    h[0] ^= 0x01010000ull ^ outlen;
    h[6] ^= personal0;
    h[7] ^= personal1;
}
// one compression: m a block, t the bytes hashed up to its end, last: the final block
MASP_HD void b2b_compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
    const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                            0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = h[i];
        v[i + 8] = iv[i];
    }
    v[12] ^= t;
    if (last) v[14] = ~v[14];
    MASP_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    MASP_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    MASP_B2B_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    MASP_B2B_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    MASP_B2B_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    MASP_B2B_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    MASP_B2B_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    MASP_B2B_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    MASP_B2B_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    MASP_B2B_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    MASP_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    MASP_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

// the digest's 64 bytes as a scalar
MASP_HD void rs_hash_scalar(uint32_t out[8], const uint64_t h[8]) {
    uint32_t wide[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wide[2 * i] = (uint32_t)h[i];
        wide[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
    rj_reduce_wide(out, wide);
}

// ---- RedJubjub signatures ----
// an item's status: the first check that fails
enum : uint8_t { RS_OK = 0, RS_BAD_SK = 1, RS_BAD_ALPHA = 2 };

// rsk and r are signing material: rs_finish clears them
struct RsState {
    uint32_t rsk[8], r[8];
    uint32_t vk[8], rbar[8];
    uint32_t status;
};

// the items' arrays as they come (include/masp_hip.h: masp_hip_redjubjub_sign_batch); rows are read as words
struct RsIn {
    const uint32_t* sks;
    const uint32_t* alphas;      // may be null: no randomisation
    const uint32_t* sighashes;
    const uint8_t* kinds;
    const uint32_t* randoms;     // 20 words an item: the reference's T
};

// the windows of the two basepoints a signature may stand on: [0] G_spend (kind 0), [1] G_vcr (kind 1)
struct RsTables {
    const JNiels* base[2];
};

// the range checks, rsk = sk + alpha, vk = [rsk] G_kind
MASP_HD void rs_key(RsState& st, const RsIn& in, const RsTables& t, size_t i) {
    uint32_t sk[8], al[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sk[k] = in.sks[8 * i + k];
        al[k] = in.alphas ? in.alphas[8 * i + k] : 0u;
    }
    const uint32_t status = !rj_is_canonical(sk) ? RS_BAD_SK : !rj_is_canonical(al) ? RS_BAD_ALPHA : RS_OK;
    st.status = status;
    if (status != RS_OK) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st.rsk[k] = st.r[k] = st.vk[k] = st.rbar[k] = 0u;
        return;
    }
    const Rj rsk = fe_add(rj_load(sk), rj_load(al));
#pragma unroll
    for (int k = 0; k < 8; ++k) st.rsk[k] = rsk.v[k];
    uint32_t w[8];
    jj_encode(w, fixed_base_mul(t.base[in.kinds[i] & 1u], st.rsk));   // (the digits straight from the state: no indexed array in registers)
#pragma unroll
    for (int k = 0; k < 8; ++k) st.vk[k] = w[k];
}

// r = H*(T | vk | sighash): 144 bytes, two blocks
MASP_HD void rs_nonce_hash(RsState& st, const RsIn& in, size_t i) {
    uint64_t m[16], h[8];
    const uint32_t *T = in.randoms + 20 * i, *sh = in.sighashes + 8 * i;
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = or_u64(T[2 * k], T[2 * k + 1]);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[10 + k] = or_u64(st.vk[2 * k], st.vk[2 * k + 1]);
    m[14] = or_u64(sh[0], sh[1]);
    m[15] = or_u64(sh[2], sh[3]);
    b2b_start(h, 64, or_le64_of("MASP__Re"), or_le64_of("dJubjubH"));
    b2b_compress(h, m, 128, false);
    m[0] = or_u64(sh[4], sh[5]);
    m[1] = or_u64(sh[6], sh[7]);
#pragma unroll
    for (int k = 2; k < 16; ++k) m[k] = 0;
    b2b_compress(h, m, 144, true);
    uint32_t r[8];
    rs_hash_scalar(r, h);
#pragma unroll
    for (int k = 0; k < 8; ++k) st.r[k] = r[k];
}

// Rbar = repr([r] G_kind)
MASP_HD void rs_nonce_point(RsState& st, const RsIn& in, const RsTables& t, size_t i) {
    uint32_t w[8];
    jj_encode(w, fixed_base_mul(t.base[in.kinds[i] & 1u], st.r));
#pragma unroll
    for (int k = 0; k < 8; ++k) st.rbar[k] = w[k];
}

// c = H*(Rbar | vk | sighash) (96 bytes, one block), S = r + c rsk; sig = Rbar | S (16 words), vk (8 words, may be null); rsk and r leave
// the state
MASP_HD void rs_finish(RsState& st, const RsIn& in, size_t i, uint32_t* sig, uint32_t* vk) {
    uint64_t m[16], h[8];
    const uint32_t* sh = in.sighashes + 8 * i;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m[k] = or_u64(st.rbar[2 * k], st.rbar[2 * k + 1]);
        m[4 + k] = or_u64(st.vk[2 * k], st.vk[2 * k + 1]);
        m[8 + k] = or_u64(sh[2 * k], sh[2 * k + 1]);
        m[12 + k] = 0;
    }
    blake2b_one_block(h, m, 96, 64, or_le64_of("MASP__Re"), or_le64_of("dJubjubH"));
    uint32_t c[8], s[8];
    rs_hash_scalar(c, h);
    rj_mul_add(s, st.r, c, st.rsk);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sig[k] = st.rbar[k];
        sig[8 + k] = s[k];
        if (vk) vk[k] = st.vk[k];
        st.rsk[k] = 0u;
        st.r[k] = 0u;
    }
}

// ---- spend descriptions ----
// a spend's status: the first check that fails, in this order; 1 to 4 are nullifier.hpp's
enum : uint8_t { SB_OK = 0, SB_BAD_ASSET = 1, SB_BAD_DIVERSIFIER = 2, SB_BAD_PK_D = 3, SB_BAD_RCM = 4, SB_BAD_AK = 5, SB_SMALL_AK = 6,
                 SB_BAD_NSK = 7, SB_BAD_AR = 8, SB_BAD_RCV = 9 };

struct SbState {
    ObState ob;          // nf (msg, rcm, cm, bad[0..3]) and vbase as output_build.hpp and nullifier.hpp keep them; the rest is not used
    uint32_t nk[8], rk[8];
    uint8_t bad[8];      // bad[s - 5] != 0: check s failed.  Every check writes its own byte.
};

// the spends' arrays as they come (include/masp_hip.h: masp_hip_sapling_build_spends); 32-byte rows are read as words
struct SbIn {
    NfIn note;           // (nks: null, nk comes from the state)
    const uint32_t* aks;
    const uint32_t* nsks;
    const uint32_t* ars;
    const uint32_t* rcvs;
};

MASP_HD uint8_t sb_status(const SbState& st) {
    uint8_t s = SB_OK;
#pragma unroll
    for (int i = 4; i >= 0; --i)
        if (st.bad[i]) s = (uint8_t)(i + 5);
#pragma unroll
    for (int i = 3; i >= 0; --i)
        if (st.ob.nf.bad[i]) s = (uint8_t)(i + 1);
    return s;
}

// the note's three checks, each writing its own bytes of the state:
//   which = 0: the asset generator and [8] g (ob_parse);  which = 1: g_d, the value and rcm (nf_parse);  which = 2: pk_d decodes (nf_key)
MASP_HD void sb_parse(SbState& st, const SbIn& in, size_t i, int which) {
    if (which == 0) {
        ObIn o = {};
        o.ids = in.note.ids;
        ob_parse(st.ob, o, i, 0);
    } else if (which == 1) {
        nf_parse(st.ob.nf, in.note, i, 1);
    } else {
        nf_key(st.ob.nf, in.note, i, 0);
        st.ob.nf.bad[4] = 0;   // (nk is computed, never refused)
    }
}

// the keys, each task writing its own bytes of the state.  tab: G_spend's windows, then G_pgk's.
//   which = 0: ak decodes (bad[0]), [8] ak is not the identity (bad[1]), ar below r_J (bad[3]), rk = ak + [ar] G_spend
//   which = 1: nsk below r_J (bad[2]), nk = [nsk] G_pgk
//   which = 2: rcv below r_J (bad[4])
MASP_HD void sb_keys(SbState& st, const SbIn& in, const JNiels* tab, size_t i, int which) {
    uint32_t k[8], w[8];
    if (which == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = in.rcvs[8 * i + j];
        st.bad[4] = !rj_is_canonical(k);
        return;
    }
    const uint32_t* src = (which == 0 ? in.ars : in.nsks) + 8 * i;
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = src[j];
    const bool kok = rj_is_canonical(k);
    if (!kok) {   // (a refused scalar indexes no table)
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = 0u;
    }
    JExt p = jj_identity();
    if (which == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = in.aks[8 * i + j];
        const bool ok = jj_decode(p, w) == JJ_OK;
        if (!ok) p = jj_identity();
        st.bad[0] = !ok;
        st.bad[1] = ok && jj_is_identity(jj_mul_by_cofactor(p));
        st.bad[3] = !kok;
    } else {
        st.bad[2] = !kok;
    }
    JExt q = fixed_base_mul(tab + (which == 0 ? 0 : SB_BASE_TABLE), k);
    if (which == 0) q = jj_add(p, q);
    jj_encode(w, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) (which == 0 ? st.rk : st.nk)[j] = w[j];
}

}  // namespace masp
