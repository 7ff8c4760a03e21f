// What the output recovery scan does for EVERY (output, ovk) pair, in one copy (k_out_recovery.hip: k_or_trial): PRF^ock (one BLAKE2b
// compression of a full 128-byte block, masp_primitives/src/sapling/note_encryption.rs:90-110), ChaCha20 block 0 under the ock for the
// Poly1305 key, and Poly1305 over the 64 ciphertext bytes of out_ciphertext against its tag (the first step of
// try_output_recovery_with_ock, masp_note_encryption/src/lib.rs:666-673).  No decryption and no curve arithmetic: a pair whose tag fails
// is finished.  MASP_HD: the kernel is a wrapper around this function, and the tests run the same source on the CPU.
#pragma once
#include "blake2b.hpp"
#include "chacha20.hpp"
#include "poly1305.hpp"

namespace masp {

constexpr uint32_t OR_COLS = 11;   // 16-byte columns of an output's 176 bytes: cv 0-1 | cmu 2-3 | epk 4-5 | c_out 6-9 | its tag 10

constexpr uint64_t or_le64_of(const char* s) {
    uint64_t x = 0;
    for (int i = 7; i >= 0; --i) x = (x << 8) | (uint8_t)s[i];
    return x;
}

MASP_HD uint64_t or_u64(uint32_t lo, uint32_t hi) { return lo | ((uint64_t)hi << 32); }

// ock = PRF^ock(ovk, cv, cmu, epk); true if out_ciphertext's tag verifies under it.  ovk: eight words (wave-uniform in the kernel);
// col: the output's column 0, column c at col[c * stride] (the kernel: the padded output count; a lone row: 1).
MASP_HD bool or_pair(uint32_t ock[8], const uint32_t* ovk, const uint4* col, size_t stride) {
    {
        uint64_t m[16], h[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = or_u64(ovk[2 * i], ovk[2 * i + 1]);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const uint4 x = col[(size_t)c * stride];
            m[4 + 2 * c] = or_u64(x.x, x.y);
            m[5 + 2 * c] = or_u64(x.z, x.w);
        }
        blake2b_one_block(h, m, 128, 32, or_le64_of("MASP__De"), or_le64_of("rive_ock"));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ock[2 * i] = (uint32_t)h[i];
            ock[2 * i + 1] = (uint32_t)(h[i] >> 32);
        }
    }
    const uint32_t nonce[3] = {0, 0, 0};
    uint32_t b0[16];
    chacha20_block(b0, ock, 0, nonce);
    Poly1305State st;
    poly1305_init(st, b0);
#pragma unroll
    for (int c = 6; c < 10; ++c) {   // 64 bytes: four whole blocks, so the AEAD's pad16 adds nothing
        const uint4 x = col[(size_t)c * stride];
        poly1305_block(st, x.x, x.y, x.z, x.w);
    }
    poly1305_block(st, 0, 0, 64, 0);   // the lengths: no associated data, 64 bytes of ciphertext
    uint32_t tag[4];
    poly1305_finish(st, b0 + 4, tag);
    const uint4 t = col[(size_t)10 * stride];
    return tag[0] == t.x && tag[1] == t.y && tag[2] == t.z && tag[3] == t.w;
}

}  // namespace masp
