// Poly1305 (RFC 8439) on the device: the accumulator and r in five 26-bit limbs, so that a block is 25 products of 32 x 32 -> 64 bits
// and no carry chain longer than five.  The caller feeds 16-byte blocks as four little-endian words; a message's last partial block
// comes padded by the caller with its 1 byte and `full` = false.  MASP_HD: also compiled for the CPU in tests.
#pragma once
#include "field.hpp"

namespace masp {

struct Poly1305State {
    uint32_t r[5], h[5];
};

// key: the first four words of the one-time key (r before clamping)
MASP_HD void poly1305_init(Poly1305State& st, const uint32_t key[4]) {
    st.r[0] = key[0] & 0x3ffffff;
    st.r[1] = ((key[0] >> 26) | (key[1] << 6)) & 0x3ffff03;
    st.r[2] = ((key[1] >> 20) | (key[2] << 12)) & 0x3ffc0ff;
    st.r[3] = ((key[2] >> 14) | (key[3] << 18)) & 0x3f03fff;
    st.r[4] = (key[3] >> 8) & 0x00fffff;
#pragma unroll
    for (int i = 0; i < 5; ++i) st.h[i] = 0;
}

// h = (h + block) r mod 2^130 - 5.  full: a whole 16-byte block (2^128 is added); otherwise the caller has placed the 1 byte
MASP_HD void poly1305_block(Poly1305State& st, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, bool full = true) {
    const uint32_t r0 = st.r[0], r1 = st.r[1], r2 = st.r[2], r3 = st.r[3], r4 = st.r[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint32_t h0 = st.h[0] + (m0 & 0x3ffffff);
    const uint32_t h1 = st.h[1] + (((m0 >> 26) | (m1 << 6)) & 0x3ffffff);
    const uint32_t h2 = st.h[2] + (((m1 >> 20) | (m2 << 12)) & 0x3ffffff);
    const uint32_t h3 = st.h[3] + (((m2 >> 14) | (m3 << 18)) & 0x3ffffff);
    const uint32_t h4 = st.h[4] + ((m3 >> 8) | (full ? 1u << 24 : 0u));
    uint64_t d0 = (uint64_t)h0 * r0 + (uint64_t)h1 * s4 + (uint64_t)h2 * s3 + (uint64_t)h3 * s2 + (uint64_t)h4 * s1;
    uint64_t d1 = (uint64_t)h0 * r1 + (uint64_t)h1 * r0 + (uint64_t)h2 * s4 + (uint64_t)h3 * s3 + (uint64_t)h4 * s2;
    uint64_t d2 = (uint64_t)h0 * r2 + (uint64_t)h1 * r1 + (uint64_t)h2 * r0 + (uint64_t)h3 * s4 + (uint64_t)h4 * s3;
    uint64_t d3 = (uint64_t)h0 * r3 + (uint64_t)h1 * r2 + (uint64_t)h2 * r1 + (uint64_t)h3 * r0 + (uint64_t)h4 * s4;
    uint64_t d4 = (uint64_t)h0 * r4 + (uint64_t)h1 * r3 + (uint64_t)h2 * r2 + (uint64_t)h3 * r1 + (uint64_t)h4 * r0;
    uint32_t c;
    c = (uint32_t)(d0 >> 26); st.h[0] = (uint32_t)d0 & 0x3ffffff; d1 += c;
    c = (uint32_t)(d1 >> 26); st.h[1] = (uint32_t)d1 & 0x3ffffff; d2 += c;
    c = (uint32_t)(d2 >> 26); st.h[2] = (uint32_t)d2 & 0x3ffffff; d3 += c;
    c = (uint32_t)(d3 >> 26); st.h[3] = (uint32_t)d3 & 0x3ffffff; d4 += c;
    c = (uint32_t)(d4 >> 26); st.h[4] = (uint32_t)d4 & 0x3ffffff;
    st.h[0] += c * 5;
    c = st.h[0] >> 26; st.h[0] &= 0x3ffffff;
    st.h[1] += c;
}

// tag = (h mod 2^130 - 5) + s mod 2^128; pad: the last four words of the one-time key (s)
MASP_HD void poly1305_finish(const Poly1305State& st, const uint32_t pad[4], uint32_t tag[4]) {
    uint32_t h0 = st.h[0], h1 = st.h[1], h2 = st.h[2], h3 = st.h[3], h4 = st.h[4], c;
    c = h1 >> 26; h1 &= 0x3ffffff; h2 += c;
    c = h2 >> 26; h2 &= 0x3ffffff; h3 += c;
    c = h3 >> 26; h3 &= 0x3ffffff; h4 += c;
    c = h4 >> 26; h4 &= 0x3ffffff; h0 += c * 5;
    c = h0 >> 26; h0 &= 0x3ffffff; h1 += c;
    // h - p, taken if it does not borrow
    uint32_t g0 = h0 + 5; c = g0 >> 26; g0 &= 0x3ffffff;
    uint32_t g1 = h1 + c; c = g1 >> 26; g1 &= 0x3ffffff;
    uint32_t g2 = h2 + c; c = g2 >> 26; g2 &= 0x3ffffff;
    uint32_t g3 = h3 + c; c = g3 >> 26; g3 &= 0x3ffffff;
    const uint32_t g4 = h4 + c - (1u << 26);
    const uint32_t take = (g4 >> 31) - 1;   // all ones if h >= p
    h0 = (h0 & ~take) | (g0 & take);
    h1 = (h1 & ~take) | (g1 & take);
    h2 = (h2 & ~take) | (g2 & take);
    h3 = (h3 & ~take) | (g3 & take);
    h4 = (h4 & ~take) | (g4 & take);
    const uint32_t w[4] = {h0 | (h1 << 26), (h1 >> 6) | (h2 << 20), (h2 >> 12) | (h3 << 14), (h3 >> 18) | (h4 << 8)};
    uint64_t f = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f += (uint64_t)w[i] + pad[i];
        tag[i] = (uint32_t)f;
        f >>= 32;
    }
}

}  // namespace masp
