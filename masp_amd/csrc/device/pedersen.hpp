// The Sapling note commitment on the device, for the compact note scan (k_note_scan_compact.hip):
//   the Pedersen hash with the NoteCommitment personalisation (six 1 bits) over the 832 bits of
//       repr(asset generator) | value (u64 LE) | repr(g_d) | repr(pk_d)
//   (host/jubjub.h: pedersen_hash, note_commitment), + [rcm] G_ncr, of which cmu is the affine u;
//   PRF^expand(rseed, [t]) mod r_J: the rcm (t = 4) and esk (t = 5) of a ZIP 212 note (host/note_encryption.h: rseed_scalar).
// 838 bits are 280 three-bit chunks (a, b, c) over 5 segments of 63 four-bit windows: chunk j of segment s adds
// (-1)^c (1 + a + 2b) 16^j G_s.  The summands come from a table of Niels points in global memory, (k + 1) 16^w G_s for k < 4, built on the
// host from masp_host::pedersen_windows() and converted to the device's Montgomery limbs: 5 x 63 x 4 x 96 bytes = 118 KiB.  One hash is
// 280 mixed additions of 7 products.  MASP_HD: the same source runs on the CPU in the tests.
#pragma once
#include "blake2b.hpp"
#include "jubjub.hpp"

namespace masp {

constexpr uint32_t PED_NC_SEGMENTS = 5, PED_WINDOWS = 63, PED_NC_CHUNKS = 280, PED_NC_BITS = 838;
constexpr uint32_t PED_NC_TABLE = PED_NC_SEGMENTS * PED_WINDOWS * 4;   // Niels points
constexpr uint32_t PED_NC_MSG_WORDS = 26;                              // 104 bytes

// bit i of (six ones | the message's bits, least significant first in every byte), zero beyond the end
MASP_HD uint32_t ped_nc_bit(const uint32_t* msg, uint32_t i) {
    if (i < 6) return 1u;
    if (i >= PED_NC_BITS) return 0u;
    const uint32_t j = i - 6;
    return (msg[j >> 5] >> (j & 31)) & 1u;
}

// msg: 26 words (any memory).  table: PED_NC_TABLE Niels points, [segment][window][k].
MASP_HD JExt pedersen_note_commit_hash(const JNiels* table, const uint32_t* msg) {
    JExt r = jj_identity();
#pragma unroll 1
    for (uint32_t c = 0; c < PED_NC_CHUNKS; ++c) {   // (c = 63 s + j: the table is laid out in chunk order)
        const uint32_t a = ped_nc_bit(msg, 3 * c), b = ped_nc_bit(msg, 3 * c + 1), neg = ped_nc_bit(msg, 3 * c + 2);
        const JNiels q = table[4 * c + a + 2 * b];
        r = jj_add_niels(r, q, neg != 0);
    }
    return r;
}

// jubjub::Fr::from_bytes_wide: the 512-bit little-endian integer in in[0..15] mod r_J, bit by bit like the host's (it runs once per
// candidate note): a = 2a + bit (a < r_J < 2^252: no overflow), then one conditional subtraction
MASP_HD void rj_from_bytes_wide(uint32_t out[8], const uint32_t in[16]) {
    uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 15; w >= 0; --w) {
        const uint32_t word = in[w];
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
#pragma unroll
            for (int i = 7; i > 0; --i) a[i] = (a[i] << 1) | (a[i - 1] >> 31);
            a[0] = (a[0] << 1) | ((word >> b) & 1u);
            uint32_t d[8], borrow = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint64_t t = (uint64_t)a[i] - RjCfg::MOD[i] - borrow;
                d[i] = (uint32_t)t;
                borrow = (uint32_t)(t >> 32) & 1u;
            }
            if (!borrow) {   // a >= r_J
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = d[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = a[i];
}

constexpr uint64_t ped_le64_of(const char* s) {
    uint64_t x = 0;
    for (int i = 7; i >= 0; --i) x = (x << 8) | (uint8_t)s[i];
    return x;
}

// PRF^expand(rseed, [domain]) = BLAKE2b-512 personalised "MASP__ExpandSeed" over the 33 bytes, reduced mod r_J
MASP_HD void rseed_scalar(uint32_t out[8], const uint32_t rseed[8], uint32_t domain) {
    uint64_t m[16], h[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = rseed[2 * i] | ((uint64_t)rseed[2 * i + 1] << 32);
    m[4] = domain & 0xffu;
#pragma unroll
    for (int i = 5; i < 16; ++i) m[i] = 0;
    blake2b_one_block(h, m, 33, 64, ped_le64_of("MASP__Ex"), ped_le64_of("pandSeed"));
    uint32_t wide[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wide[2 * i] = (uint32_t)h[i];
        wide[2 * i + 1] = (uint32_t)(h[i] >> 32);
    }
    rj_from_bytes_wide(out, wide);
}

// cmu: the canonical affine u of PedersenHash(NoteCommitment, msg) + [rcm] G_ncr, as eight little-endian words.  g_ncr: the
// note-commitment randomness generator (Z = 1).  rcm: any 256-bit integer.
MASP_HD void note_commit_u(uint32_t cmu[8], const JNiels* table, const JExt& g_ncr, const uint32_t* msg, const uint32_t rcm[8]) {
    const JExt h = pedersen_note_commit_hash(table, msg);
    const JExt s = jj_add(jj_mul(g_ncr, rcm), h);
    const Fr u = fe_from_mont(fe_mul(s.U, fe_inv(s.Z)));
#pragma unroll
    for (int i = 0; i < 8; ++i) cmu[i] = u.v[i];
}

}  // namespace masp
