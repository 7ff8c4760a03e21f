// ChaCha20 and Poly1305 (RFC 8439) and the AEAD built from them, as note encryption uses it (masp_note_encryption/src/lib.rs:
// ChaCha20Poly1305 with a 96-bit all-zero nonce and empty associated data): the Poly1305 key is the first 32 bytes of ChaCha20
// block 0, the data is encrypted from block 1 on, and the tag is Poly1305 over the ciphertext padded to 16 bytes followed by the
// two 64-bit lengths (0 and the ciphertext's).  In the style of blake2b.h: small, header-only, no tables.
#pragma once
#include <cstdint>
#include <cstring>

namespace masp_host {

inline uint32_t cc_le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t cc_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// one 64-byte ChaCha20 block: key 32 bytes, block counter, nonce 12 bytes
inline void chacha20_block(uint8_t out[64], const uint8_t key[32], uint32_t counter, const uint8_t nonce[12]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int i = 0; i < 8; ++i) s[4 + i] = cc_le32(key + 4 * i);
    s[12] = counter;
    for (int i = 0; i < 3; ++i) s[13 + i] = cc_le32(nonce + 4 * i);
    uint32_t x[16];
    memcpy(x, s, sizeof x);
    auto qr = [&](int a, int b, int c, int d) {
        x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 16);
        x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 12);
        x[a] += x[b]; x[d] = cc_rotl(x[d] ^ x[a], 8);
        x[c] += x[d]; x[b] = cc_rotl(x[b] ^ x[c], 7);
    };
    for (int r = 0; r < 10; ++r) {
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
    }
    for (int i = 0; i < 16; ++i) {
        const uint32_t v = x[i] + s[i];
        out[4 * i] = (uint8_t)v; out[4 * i + 1] = (uint8_t)(v >> 8); out[4 * i + 2] = (uint8_t)(v >> 16); out[4 * i + 3] = (uint8_t)(v >> 24);
    }
}

// out = in xor keystream from block `counter` on (in == out allowed)
inline void chacha20_xor(uint8_t* out, const uint8_t* in, size_t n, const uint8_t key[32], uint32_t counter, const uint8_t nonce[12]) {
    uint8_t ks[64];
    for (size_t off = 0; off < n; off += 64, ++counter) {
        chacha20_block(ks, key, counter, nonce);
        const size_t take = n - off < 64 ? n - off : 64;
        for (size_t i = 0; i < take; ++i) out[off + i] = in[off + i] ^ ks[i];
    }
}

// Poly1305 in five 26-bit limbs; update() takes whole messages or pieces, a trailing partial block gets its 1 byte on finalize
class Poly1305 {
  public:
    explicit Poly1305(const uint8_t key[32]) {
        r_[0] = cc_le32(key) & 0x3ffffff;
        r_[1] = (cc_le32(key + 3) >> 2) & 0x3ffff03;
        r_[2] = (cc_le32(key + 6) >> 4) & 0x3ffc0ff;
        r_[3] = (cc_le32(key + 9) >> 6) & 0x3f03fff;
        r_[4] = (cc_le32(key + 12) >> 8) & 0x00fffff;
        for (int i = 0; i < 4; ++i) pad_[i] = cc_le32(key + 16 + 4 * i);
    }
    void update(const uint8_t* m, size_t n) {
        while (n) {
            const size_t take = n < 16 - buflen_ ? n : 16 - buflen_;
            memcpy(buf_ + buflen_, m, take);
            buflen_ += take;
            m += take;
            n -= take;
            if (buflen_ == 16) {
                block(buf_, 1u << 24);
                buflen_ = 0;
            }
        }
    }
    void finalize(uint8_t tag[16]) {
        if (buflen_) {
            buf_[buflen_] = 1;
            memset(buf_ + buflen_ + 1, 0, 15 - buflen_);
            block(buf_, 0);
        }
        uint32_t h0 = h_[0], h1 = h_[1], h2 = h_[2], h3 = h_[3], h4 = h_[4], c;
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
        const uint32_t take_g = (g4 >> 31) - 1;   // all ones if h >= p
        h0 = (h0 & ~take_g) | (g0 & take_g);
        h1 = (h1 & ~take_g) | (g1 & take_g);
        h2 = (h2 & ~take_g) | (g2 & take_g);
        h3 = (h3 & ~take_g) | (g3 & take_g);
        h4 = (h4 & ~take_g) | (g4 & take_g);
        const uint32_t w[4] = {h0 | (h1 << 26), (h1 >> 6) | (h2 << 20), (h2 >> 12) | (h3 << 14), (h3 >> 18) | (h4 << 8)};
        uint64_t f = 0;
        for (int i = 0; i < 4; ++i) {
            f += (uint64_t)w[i] + pad_[i];
            tag[4 * i] = (uint8_t)f; tag[4 * i + 1] = (uint8_t)(f >> 8); tag[4 * i + 2] = (uint8_t)(f >> 16); tag[4 * i + 3] = (uint8_t)(f >> 24);
            f >>= 32;
        }
    }

  private:
    void block(const uint8_t* m, uint32_t hibit) {
        const uint32_t r0 = r_[0], r1 = r_[1], r2 = r_[2], r3 = r_[3], r4 = r_[4];
        const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
        const uint32_t h0 = h_[0] + (cc_le32(m) & 0x3ffffff);
        const uint32_t h1 = h_[1] + ((cc_le32(m + 3) >> 2) & 0x3ffffff);
        const uint32_t h2 = h_[2] + ((cc_le32(m + 6) >> 4) & 0x3ffffff);
        const uint32_t h3 = h_[3] + ((cc_le32(m + 9) >> 6) & 0x3ffffff);
        const uint32_t h4 = h_[4] + ((cc_le32(m + 12) >> 8) | hibit);
        uint64_t d0 = (uint64_t)h0 * r0 + (uint64_t)h1 * s4 + (uint64_t)h2 * s3 + (uint64_t)h3 * s2 + (uint64_t)h4 * s1;
        uint64_t d1 = (uint64_t)h0 * r1 + (uint64_t)h1 * r0 + (uint64_t)h2 * s4 + (uint64_t)h3 * s3 + (uint64_t)h4 * s2;
        uint64_t d2 = (uint64_t)h0 * r2 + (uint64_t)h1 * r1 + (uint64_t)h2 * r0 + (uint64_t)h3 * s4 + (uint64_t)h4 * s3;
        uint64_t d3 = (uint64_t)h0 * r3 + (uint64_t)h1 * r2 + (uint64_t)h2 * r1 + (uint64_t)h3 * r0 + (uint64_t)h4 * s4;
        uint64_t d4 = (uint64_t)h0 * r4 + (uint64_t)h1 * r3 + (uint64_t)h2 * r2 + (uint64_t)h3 * r1 + (uint64_t)h4 * r0;
        uint32_t c;
        c = (uint32_t)(d0 >> 26); h_[0] = (uint32_t)d0 & 0x3ffffff; d1 += c;
        c = (uint32_t)(d1 >> 26); h_[1] = (uint32_t)d1 & 0x3ffffff; d2 += c;
        c = (uint32_t)(d2 >> 26); h_[2] = (uint32_t)d2 & 0x3ffffff; d3 += c;
        c = (uint32_t)(d3 >> 26); h_[3] = (uint32_t)d3 & 0x3ffffff; d4 += c;
        c = (uint32_t)(d4 >> 26); h_[4] = (uint32_t)d4 & 0x3ffffff;
        h_[0] += c * 5;
        c = h_[0] >> 26; h_[0] &= 0x3ffffff;
        h_[1] += c;
    }
    uint32_t r_[5], h_[5] = {0, 0, 0, 0, 0}, pad_[4];
    uint8_t buf_[16];
    size_t buflen_ = 0;
};

// the AEAD's tag over a ciphertext (no associated data): Poly1305 keyed by ChaCha20 block 0
inline void aead_tag(uint8_t tag[16], const uint8_t key[32], const uint8_t nonce[12], const uint8_t* ct, size_t n) {
    uint8_t b0[64];
    chacha20_block(b0, key, 0, nonce);
    Poly1305 mac(b0);
    static const uint8_t zeros[16] = {0};
    mac.update(ct, n);
    if (n % 16) mac.update(zeros, 16 - n % 16);
    uint8_t lens[16] = {0};
    for (int i = 0; i < 8; ++i) lens[8 + i] = (uint8_t)((uint64_t)n >> (8 * i));
    mac.update(lens, 16);
    mac.finalize(tag);
}
inline void aead_encrypt(uint8_t* ct, uint8_t tag[16], const uint8_t key[32], const uint8_t nonce[12], const uint8_t* pt, size_t n) {
    chacha20_xor(ct, pt, n, key, 1, nonce);
    aead_tag(tag, key, nonce, ct, n);
}
// false (and pt untouched) if the tag does not verify
inline bool aead_decrypt(uint8_t* pt, const uint8_t key[32], const uint8_t nonce[12], const uint8_t* ct, size_t n, const uint8_t tag[16]) {
    uint8_t want[16];
    aead_tag(want, key, nonce, ct, n);
    uint8_t diff = 0;
    for (int i = 0; i < 16; ++i) diff |= want[i] ^ tag[i];
    if (diff) return false;
    chacha20_xor(pt, ct, n, key, 1, nonce);
    return true;
}

}  // namespace masp_host
