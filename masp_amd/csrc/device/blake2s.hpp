// BLAKE2s-256 (RFC 7693) on the device for messages of one or two blocks: unkeyed, with an 8-byte personalisation, up to 128 bytes of
// input.  What the group hashes of the compact note scan need (k_note_scan_compact.hip): "MASP__v_" over a 32-byte asset identifier (one
// block) and "MASP__gd" over GH_FIRST_BLOCK and an 11-byte diversifier (75 bytes: two blocks).  host/jubjub.h's Blake2s is the general
// form.  MASP_HD: the same source runs on the CPU in the tests.
#pragma once
#include "field.hpp"

namespace masp {

MASP_HD uint32_t b2s_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

#define MASP_B2S_G(a, b, c, d, x, y)      \
    do {                                  \
        v[a] = v[a] + v[b] + (x);         \
        v[d] = b2s_rotr(v[d] ^ v[a], 16); \
        v[c] = v[c] + v[d];               \
        v[b] = b2s_rotr(v[b] ^ v[c], 12); \
        v[a] = v[a] + v[b] + (y);         \
        v[d] = b2s_rotr(v[d] ^ v[a], 8);  \
        v[c] = v[c] + v[d];               \
        v[b] = b2s_rotr(v[b] ^ v[c], 7);  \
    } while (0)

// one round with the message schedule as compile-time indices (as blake2b.hpp does: the message words stay in registers)
#define MASP_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                                      \
        MASP_B2S_G(0, 4, 8, 12, m[s0], m[s1]);                                                \
        MASP_B2S_G(1, 5, 9, 13, m[s2], m[s3]);                                                \
        MASP_B2S_G(2, 6, 10, 14, m[s4], m[s5]);                                               \
        MASP_B2S_G(3, 7, 11, 15, m[s6], m[s7]);                                               \
        MASP_B2S_G(0, 5, 10, 15, m[s8], m[s9]);                                               \
        MASP_B2S_G(1, 6, 11, 12, m[s10], m[s11]);                                             \
        MASP_B2S_G(2, 7, 8, 13, m[s12], m[s13]);                                              \
        MASP_B2S_G(3, 4, 9, 14, m[s14], m[s15]);                                              \
    } while (0)

// the compression function: h the chaining value, m one 64-byte block as sixteen little-endian words, t the bytes hashed so far
// including this block's, last: the final block
MASP_HD void blake2s_compress(uint32_t h[8], const uint32_t m[16], uint32_t t, bool last) {
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = h[i];
        v[i + 8] = iv[i];
    }
    v[12] ^= t;                  // (messages of at most 128 bytes: the counter's high word stays zero)
    if (last) v[14] = ~v[14];
    MASP_B2S_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    MASP_B2S_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    MASP_B2S_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    MASP_B2S_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    MASP_B2S_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    MASP_B2S_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    MASP_B2S_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    MASP_B2S_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    MASP_B2S_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    MASP_B2S_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

// h[0..7] = BLAKE2s-256 of the `len` <= 128 bytes held little-endian in m[0..31] (zero beyond the message; m[16..31] is not read when
// len <= 64), personal: the 8 personalisation bytes as two little-endian words.  A message of exactly 64 bytes is ONE (final) block.
MASP_HD void blake2s_256(uint32_t h[8], const uint32_t* m, uint32_t len, uint32_t personal0, uint32_t personal1) {
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = iv[i];
    h[0] ^= 0x01010000u ^ 32u;   // digest length 32, no key, fanout 1, depth 1
    h[6] ^= personal0;
    h[7] ^= personal1;
    if (len <= 64) {
        blake2s_compress(h, m, len, true);
    } else {
        blake2s_compress(h, m, 64, false);
        blake2s_compress(h, m + 16, len, true);
    }
}

constexpr uint32_t le32_of(const char* s) {
    return (uint32_t)(uint8_t)s[0] | ((uint32_t)(uint8_t)s[1] << 8) | ((uint32_t)(uint8_t)s[2] << 16) | ((uint32_t)(uint8_t)s[3] << 24);
}

}  // namespace masp
