// Group hashing into Jubjub on the device: BLAKE2s-256 of the input, the digest decoded as a point (jj_decode).  The two rules of
// host/jubjub.h, bit for bit:
//   jj_group_hash_gd      `group_hash` with the personalisation "MASP__gd" over a diversifier (Diversifier::g_d): the message is the 64-byte
//                         GH_FIRST_BLOCK followed by the 11 bytes; the decoded point is multiplied by the cofactor, the identity is refused,
//                         and the CLEARED point is the result;
//   jj_asset_generator    `asset_generator` ("MASP__v_" over the 32-byte identifier, no first block): the cofactor is NOT cleared, a point of
//                         small order is refused, and the decoded point itself is the result.
// MASP_HD: the same source runs on the CPU in the tests.
#pragma once
#include "blake2s.hpp"
#include "jubjub.hpp"

namespace masp {

// "096b36a5804bfacef1691e173c366a47ff5ba84a44f26ddd7e8d9f79d5b42df0" (GH_FIRST_BLOCK: 64 ASCII characters) as little-endian words
MASP_HD void gh_first_block(uint32_t m[16]) {
    const uint32_t w[16] = {0x62363930u, 0x35613633u, 0x62343038u, 0x65636166u, 0x39363166u, 0x37316531u, 0x36336333u, 0x37346136u,
                            0x62356666u, 0x61343861u, 0x32663434u, 0x64646436u, 0x64386537u, 0x39376639u, 0x34623564u, 0x30666432u};
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = w[i];
}

// d: the diversifier's 11 bytes in three little-endian words (the top byte of d[2] is ignored).  false: the diversifier has no g_d.
MASP_HD bool jj_group_hash_gd(JExt& out, const uint32_t d[3]) {
    uint32_t m[32], h[8];
    gh_first_block(m);
    m[16] = d[0];
    m[17] = d[1];
    m[18] = d[2] & 0x00ffffffu;
#pragma unroll
    for (int i = 19; i < 32; ++i) m[i] = 0;
    blake2s_256(h, m, 75, le32_of("MASP"), le32_of("__gd"));
    JExt p;
    if (jj_decode(p, h) != JJ_OK) return false;
    p = jj_mul_by_cofactor(p);
    if (jj_is_identity(p)) return false;
    out = p;
    return true;
}

// id: the asset identifier as eight little-endian words.  false: the identifier has no generator.  digest: the BLAKE2s digest, which IS the
// generator's 32-byte encoding (jj_decode accepts canonical encodings only, so encoding the decoded point gives the digest back): the note
// commitment hashes these bytes and needs no inversion for them.
MASP_HD bool jj_asset_generator(JExt& out, uint32_t digest[8], const uint32_t id[8]) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m[i] = id[i];
        m[8 + i] = 0;
    }
    blake2s_256(digest, m, 32, le32_of("MASP"), le32_of("__v_"));
    JExt p;
    if (jj_decode(p, digest) != JJ_OK) return false;
    if (jj_is_identity(jj_mul_by_cofactor(p))) return false;
    out = p;
    return true;
}

}  // namespace masp
