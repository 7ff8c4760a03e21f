// Allowed conversions on the device (k_conversion.hip): AllowedConversion::from(I128Sum) and AllowedConversion::cmu of
// masp_primitives/src/convert.rs:39-64, 86-118, host/host_api.cpp's masp_host_allowed_conversion and masp_host_convert_cmu, for many
// conversions at once.  For conversion c with the terms (id_j, v_j), v_j an i128:
//   G_j       = the asset generator of id_j, cofactor NOT cleared (jj_asset_generator)
//   k_j       = |v_j| as u64: the LOW 64 bits of the absolute value; i128::MIN has none
//   generator = sum_j sign(v_j) [k_j] G_j, as its 32-byte encoding
//   cm        = PedersenHash(NoteCommitment, the 256 bits of repr(generator)),  cmu = its affine u
// The hashed message is the six personalisation ones and 256 bits: 262 bits, EXACTLY 88 three-bit chunks, the last one padded with two
// zero bits.  They are the first 88 chunk positions of the note commitment's table (pedersen.hpp: chunks 0..62 segment 0, 63..87 segment
// 1).  A zero chunk still adds 1 16^j G_s, so the 280-chunk routine over a message padded with zeros gives another point: the sum ends at 88.
//
// The terms are summed AS GIVEN: equal identifiers are not merged and zeros are not dropped (with the 64-bit truncation, merging before and
// after summing differ; merging is the caller's).  A conversion without terms has the identity as its generator.
// A term is a point and a status byte (cv_term); a conversion's terms and then its 88 summands are dealt to `lanes` lanes (term or chunk t
// to lane t mod lanes), each adds its share, and the partial sums are folded with jj_add.  The addition is complete, so the order is free
// and the affine results, every output byte, do not depend on `lanes`.  There is no reduction ACROSS lane groups: one very long conversion
// is a serial loop of its lanes.  MASP_HD: the tests run the same source on the CPU.
#pragma once
#include "group_hash.hpp"
#include "pedersen.hpp"

namespace masp {

constexpr uint32_t CV_CHUNKS = 88, CV_MSG_WORDS = 9;   // 262 bits

// a conversion's status: 1 if any of its terms has no generator, else 2 if any of its terms is i128::MIN; whatever the terms' order
enum : uint8_t { CV_OK = 0, CV_BAD_ASSET = 1, CV_BAD_VALUE = 2 };

MASP_HD JExt cv_neg(const JExt& p) { return {fe_neg(p.U), p.V, p.Z, fe_neg(p.T)}; }

// [k] p for a 64-bit k = hi : lo.  jj_mul's left-to-right double-and-add over two words instead of eight: the scalar is shifted out at the
// top, and the doublings start at the lane's top set bit.
MASP_HD JExt cv_mul64(const JExt& p, uint32_t lo, uint32_t hi) {
    JExt r = jj_identity();
    bool started = false;
    for (int i = 0; i < 64; ++i) {
        const bool bit = hi >> 31;
        hi = (hi << 1) | (lo >> 31);
        lo <<= 1;
        if (started) r = jj_dbl(r);
        if (bit) {
            r = started ? jj_add(r, p) : p;
            started = true;
        }
    }
    return r;
}

// One term: id = the identifier's eight words, v = the i128's four words, least significant first.  -> the term's status byte; out =
// sign(v) [|v| as u64] G, the identity for a refused term (never summed: its conversion is refused as a whole).
MASP_HD uint8_t cv_term(JExt& out, const uint32_t* id, const uint32_t* v) {
    uint32_t w[8], digest[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = id[k];
    out = jj_identity();
    JExt g;
    if (!jj_asset_generator(g, digest, w)) return CV_BAD_ASSET;
    uint32_t lo = v[0], hi = v[1];
    const bool negative = v[3] >> 31;
    if (negative) {
        if (v[3] == 0x80000000u && (v[2] | v[1] | v[0]) == 0) return CV_BAD_VALUE;   // i128::MIN
        lo = ~lo + 1u;                                                              // the low 64 bits of -v
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
    const JExt t = cv_mul64(g, lo, hi);
    out = negative ? cv_neg(t) : t;
    return CV_OK;
}

// the share of lane `lane` of `lanes` in a conversion's status: bit 0 = one of its terms' bytes is CV_BAD_ASSET, bit 1 = one is
// CV_BAD_VALUE.  The lanes' masks are OR-ed (cv_status_of).  term_status: the bytes of cv_term; the conversion owns [begin, end).
MASP_HD uint32_t cv_status_partial(const uint8_t* term_status, uint64_t begin, uint64_t end, uint32_t lane, uint32_t lanes) {
    uint32_t mask = 0;
    for (uint64_t t = begin + lane; t < end; t += lanes) {
        const uint32_t s = term_status[t];
        mask |= (s == CV_BAD_ASSET ? 1u : 0u) | (s == CV_BAD_VALUE ? 2u : 0u);
    }
    return mask;
}

MASP_HD uint8_t cv_status_of(uint32_t mask) { return (mask & 1u) ? CV_BAD_ASSET : (mask & 2u) ? CV_BAD_VALUE : CV_OK; }

// the share of lane `lane` of `lanes` in the generator: the terms begin + lane, begin + lane + lanes, ... of `points`
MASP_HD JExt cv_sum_partial(const JExt* points, uint64_t begin, uint64_t end, uint32_t lane, uint32_t lanes) {
    JExt r = jj_identity();
#pragma unroll 1
    for (uint64_t t = begin + lane; t < end; t += lanes) {
        const JExt q = points[t];
        r = jj_add(r, q);
    }
    return r;
}

// m >>= s over the nine message words, 0 < s < 32
MASP_HD void cv_shift(uint32_t m[CV_MSG_WORDS], uint32_t s) {
#pragma unroll
    for (uint32_t i = 0; i + 1 < CV_MSG_WORDS; ++i) m[i] = (m[i] >> s) | (m[i + 1] << (32 - s));
    m[CV_MSG_WORDS - 1] >>= s;
}

// the share of lane `lane` of `lanes` (lanes <= 10: three bits a chunk, shifts below 32) in cm: the chunks c = lane, lane + lanes, ...
// of the 88.  gen: the generator's encoding, eight words.  ped: the Pedersen Niels table (pedersen.hpp).  The message lives in nine
// registers and is shifted out at the bottom, three bits a chunk: no register is indexed at run time.
MASP_HD JExt cv_hash_partial(const uint32_t gen[8], const JNiels* ped, uint32_t lane, uint32_t lanes) {
    uint32_t m[CV_MSG_WORDS];
    m[0] = 0x3fu | (gen[0] << 6);
#pragma unroll
    for (int i = 1; i < 8; ++i) m[i] = (gen[i - 1] >> 26) | (gen[i] << 6);
    m[8] = gen[7] >> 26;   // bits 256..261; everything above is zero: chunk 87's padding
    if (lane) cv_shift(m, 3 * lane);
    JExt r = jj_identity();
#pragma unroll 1
    for (uint32_t c = lane; c < CV_CHUNKS; c += lanes) {
        const uint32_t bits = m[0] & 7u;
        const JNiels q = ped[4 * c + (bits & 3u)];   // (1 + a + 2 b) 16^j G_s
        r = jj_add_niels(r, q, (bits & 4u) != 0);
        cv_shift(m, 3 * lanes);
    }
    return r;
}

// cmu: the canonical affine u of cm, eight little-endian words
MASP_HD void cv_cmu(uint32_t cmu[8], const JExt& cm) {
    const Fr u = fe_from_mont(fe_mul(cm.U, fe_inv(cm.Z)));
#pragma unroll
    for (int k = 0; k < 8; ++k) cmu[k] = u.v[k];
}

}  // namespace masp
