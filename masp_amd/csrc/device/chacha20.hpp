// The ChaCha20 block function (RFC 8439) on the device, in words: key eight, nonce three little-endian 32-bit words.  The note scan
// (k_note_scan.hip) needs block 0 alone, whose first 32 bytes key Poly1305; it never decrypts.  MASP_HD: also compiled for the CPU in tests.
#pragma once
#include "field.hpp"

namespace masp {

MASP_HD uint32_t cc_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define MASP_CC_QR(a, b, c, d)             \
    do {                                   \
        x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 16); \
        x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 12); \
        x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 8);  \
        x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 7);  \
    } while (0)

MASP_HD void chacha20_block(uint32_t out[16], const uint32_t key[8], uint32_t counter, const uint32_t nonce[3]) {
    uint32_t s[16], x[16];
    s[0] = 0x61707865u; s[1] = 0x3320646eu; s[2] = 0x79622d32u; s[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[4 + i] = key[i];
    s[12] = counter;
#pragma unroll
    for (int i = 0; i < 3; ++i) s[13 + i] = nonce[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        MASP_CC_QR(0, 4, 8, 12); MASP_CC_QR(1, 5, 9, 13); MASP_CC_QR(2, 6, 10, 14); MASP_CC_QR(3, 7, 11, 15);
        MASP_CC_QR(0, 5, 10, 15); MASP_CC_QR(1, 6, 11, 12); MASP_CC_QR(2, 7, 8, 13); MASP_CC_QR(3, 4, 9, 14);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

}  // namespace masp
