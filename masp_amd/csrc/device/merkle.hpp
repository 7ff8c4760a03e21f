// The Sapling Merkle hash on the device, for the frozen commitment tree (k_merkle.hip): the parent of two nodes at `level` is the affine u of
//   PedersenHash(MerkleTree(level), lhs[0..255) | rhs[0..255))
// (host/jubjub.h: merkle_hash; masp_primitives/src/sapling.rs:54-85).  The message is 516 bits: the six bits of the level, least significant
// first, then bits 0..254 of lhs, then bits 0..254 of rhs; 516 = 3 x 172, so it is 172 whole three-bit chunks (a, b, c) over segments 0, 1
// and 2 of the Pedersen table (63 + 63 + 46 windows), and chunk j adds (-1)^c times entry [4 j + a + 2 b] of the Niels table that
// device/pedersen.hpp describes ((k + 1) 16^w G_s, laid out in chunk order): its first 172 x 4 points.  One hash is 172 mixed additions of
// 7 products and one inversion.  The message lives in 17 registers that are shifted down three bits per chunk: nothing is indexed at run
// time, so nothing goes to scratch.  MASP_HD: the same source runs on the CPU in the tests.
#pragma once
#include "pedersen.hpp"

namespace masp {

constexpr uint32_t MT_DEPTH = 32;                     // SAPLING_COMMITMENT_TREE_DEPTH
constexpr uint32_t MT_CHUNKS = 172, MT_BITS = 516;    // 6 + 255 + 255
constexpr uint32_t MT_TABLE = MT_CHUNKS * 4;          // the Niels points of the table's head that a Merkle hash reads
constexpr uint32_t MT_MSG_WORDS = 17;
static_assert(MT_BITS == 3 * MT_CHUNKS && MT_TABLE <= PED_NC_TABLE && MT_CHUNKS == 2 * PED_WINDOWS + 46, "the Merkle hash's chunks");

// a < q, the BLS12-381 scalar modulus, as eight little-endian words (Node::read accepts exactly these)
MASP_HD bool fr_is_canonical(const uint32_t a[8]) {
    Fr x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x.v[i] = a[i];
    return !fe_canonical_ge_mod(x);
}

// level (6 bits) | lhs (255 bits) | rhs (255 bits), least significant bit first
MASP_HD void merkle_message(uint32_t m[MT_MSG_WORDS], uint32_t level, const uint32_t lhs[8], const uint32_t rhs[8]) {
    uint32_t l[9], r[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        l[i] = lhs[i];
        r[i] = rhs[i];
    }
    l[7] &= 0x7fffffffu;
    r[7] &= 0x7fffffffu;
    l[8] = r[8] = 0;
#pragma unroll
    for (int i = 0; i < (int)MT_MSG_WORDS; ++i) m[i] = 0;
    m[0] = level & 63u;
#pragma unroll
    for (int i = 0; i < 9; ++i) {   // lhs from bit 6, rhs from bit 261 = 8 x 32 + 5
        m[i] |= (l[i] << 6) | (i ? l[i - 1] >> 26 : 0u);
        m[8 + i] |= (r[i] << 5) | (i ? r[i - 1] >> 27 : 0u);
    }
}

// table: the Pedersen Niels table, [segment][window][k] (at least its first MT_TABLE points).  level < 64; lhs, rhs: eight words each.
MASP_HD JExt merkle_combine_point(const JNiels* table, uint32_t level, const uint32_t lhs[8], const uint32_t rhs[8]) {
    uint32_t m[MT_MSG_WORDS];
    merkle_message(m, level, lhs, rhs);
    JExt p = jj_identity();
#pragma unroll 1
    for (uint32_t c = 0; c < MT_CHUNKS; ++c) {
        const uint32_t bits = m[0] & 7u;
#pragma unroll
        for (int i = 0; i + 1 < (int)MT_MSG_WORDS; ++i) m[i] = (m[i] >> 3) | (m[i + 1] << 29);
        m[MT_MSG_WORDS - 1] >>= 3;
        const JNiels q = table[4 * c + (bits & 3u)];
        p = jj_add_niels(p, q, (bits & 4u) != 0);
    }
    return p;
}

// the parent node: the canonical affine u as eight little-endian words
MASP_HD void merkle_combine(uint32_t out[8], const JNiels* table, uint32_t level, const uint32_t lhs[8], const uint32_t rhs[8]) {
    const JExt p = merkle_combine_point(table, level, lhs, rhs);
    const Fr u = fe_from_mont(fe_mul(p.U, fe_inv(p.Z)));
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = u.v[i];
}

// The node vector of FrozenCommitmentTree::complete (masp_primitives/src/merkle_tree.rs:177-205) over a row of n nodes at height0: every
// row padded to an even width, the next one directly behind it, the last one the single node of level 32.  mt_row(n, i, start, width):
// the start and the unpadded width of row i (level height0 + i), for the host's layout and the path kernel alike.
MASP_HD void mt_row(uint64_t n, uint32_t i, uint64_t& start, uint64_t& width) {
    start = 0;
    width = n;
    for (uint32_t h = 0; h < i; ++h) {
        width += width & 1u;
        start += width;
        width >>= 1;
    }
}

}  // namespace masp
