// BLAKE2b (RFC 7693) on the device for messages of one block: unkeyed, with a 16-byte personalisation, up to 128 bytes of input, a
// digest of up to 64 bytes.  One compression, which is all the Sapling KDF needs (64 bytes: the shared secret and epk,
// k_note_scan.hip); host/blake2b.h is the general form.  MASP_HD: the same source runs on the CPU in the tests.
#pragma once
#include "field.hpp"

namespace masp {

MASP_HD uint64_t b2b_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

#define MASP_B2B_G(a, b, c, d, x, y)      \
    do {                                  \
        v[a] = v[a] + v[b] + (x);         \
        v[d] = b2b_rotr(v[d] ^ v[a], 32); \
        v[c] = v[c] + v[d];               \
        v[b] = b2b_rotr(v[b] ^ v[c], 24); \
        v[a] = v[a] + v[b] + (y);         \
        v[d] = b2b_rotr(v[d] ^ v[a], 16); \
        v[c] = v[c] + v[d];               \
        v[b] = b2b_rotr(v[b] ^ v[c], 63); \
    } while (0)

// one round with the message schedule as compile-time indices (the twelve rounds below spell the sigma table out: the message
// words then stay in registers, where a table lookup would index them at run time)
#define MASP_B2B_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                                      \
        MASP_B2B_G(0, 4, 8, 12, m[s0], m[s1]);                                                \
        MASP_B2B_G(1, 5, 9, 13, m[s2], m[s3]);                                                \
        MASP_B2B_G(2, 6, 10, 14, m[s4], m[s5]);                                               \
        MASP_B2B_G(3, 7, 11, 15, m[s6], m[s7]);                                               \
        MASP_B2B_G(0, 5, 10, 15, m[s8], m[s9]);                                               \
        MASP_B2B_G(1, 6, 11, 12, m[s10], m[s11]);                                             \
        MASP_B2B_G(2, 7, 8, 13, m[s12], m[s13]);                                              \
        MASP_B2B_G(3, 4, 9, 14, m[s14], m[s15]);                                              \
    } while (0)

// h[0..7] = BLAKE2b of the `len` <= 128 bytes held little-endian in m[0..15] (zero beyond the message), digest length outlen <= 64
// (the first outlen bytes of h, little-endian), personal: the 16 personalisation bytes as two little-endian words
MASP_HD void blake2b_one_block(uint64_t h[8], const uint64_t m[16], uint32_t len, uint32_t outlen, uint64_t personal0, uint64_t personal1) {
    const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                            0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = iv[i];
        v[i + 8] = iv[i];
    }
    h[0] ^= 0x01010000ull ^ outlen;   // digest length, no key, fanout 1, depth 1
    h[6] ^= personal0;
    h[7] ^= personal1;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i];
    v[12] ^= len;       // the byte counter
    v[14] = ~v[14];     // the last (only) block
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

}  // namespace masp
