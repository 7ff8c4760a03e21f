// Sapling note encryption for MASP on the host: key agreement, KDF, the AEAD, note-plaintext parsing and the full trial decryption of
// `try_sapling_note_decryption` (masp_note_encryption/src/lib.rs:492-577 over masp_primitives/src/sapling/note_encryption.rs:62-86,
// :112-150, :194-260).  The single-output API of the product, the finisher of the GPU scan's hits (k_note_scan.hip stops at the
// tag) and what that scan is tested against; and the compact (ZIP 307) form of lib.rs:589-624, which has no tag and which the GPU's
// compact scan (k_note_scan_compact.hip) is tested and measured against.  Outgoing ciphertexts and ovk recovery are not here.
#pragma once
#include "blake2b.h"
#include "chacha20poly1305.h"
#include "jubjub.h"

namespace masp_host {

constexpr size_t NOTE_PLAINTEXT_SIZE = 1 + 11 + 8 + 32 + 32 + 512;   // lead byte, diversifier, value, asset identifier, rseed / rcm, memo
constexpr size_t ENC_CIPHERTEXT_SIZE = NOTE_PLAINTEXT_SIZE + 16;

// r_J, the order of Jubjub's prime-order subgroup, little-endian 64-bit limbs
static const uint64_t RJ[4] = {0xd0970e5ed6f72cb7ull, 0xa6682093ccc81082ull, 0x06673b0101343b00ull, 0x0e7db4ea6533afa9ull};

inline bool rj_is_canonical(const uint8_t le32[32]) {
    for (int i = 3; i >= 0; --i) {
        uint64_t w;
        memcpy(&w, le32 + 8 * i, 8);
        if (w != RJ[i]) return w < RJ[i];
    }
    return false;
}
// jubjub::Fr::from_bytes_wide: a 512-bit little-endian integer mod r_J (bit by bit: it runs once per decrypted note)
inline void rj_from_bytes_wide(uint8_t out32[32], const uint8_t in64[64]) {
    uint64_t a[4] = {0, 0, 0, 0};
    for (int bit = 511; bit >= 0; --bit) {
        // a = 2a + bit (a < r_J < 2^252: no overflow), then one conditional subtraction
        for (int i = 3; i > 0; --i) a[i] = (a[i] << 1) | (a[i - 1] >> 63);
        a[0] = (a[0] << 1) | ((in64[bit / 8] >> (bit % 8)) & 1);
        bool ge = true;
        for (int i = 3; i >= 0; --i)
            if (a[i] != RJ[i]) {
                ge = a[i] > RJ[i];
                break;
            }
        if (ge) {
            unsigned __int128 borrow = 0;
            for (int i = 0; i < 4; ++i) {
                const unsigned __int128 d = (unsigned __int128)a[i] - RJ[i] - (uint64_t)borrow;
                a[i] = (uint64_t)d;
                borrow = (d >> 64) & 1;
            }
        }
    }
    memcpy(out32, a, 32);
}

// PRF^expand(sk, t) = BLAKE2b-512 personalised "MASP__ExpandSeed" (masp_primitives/src/keys.rs:5-22)
inline void prf_expand(uint8_t out64[64], const uint8_t* sk, size_t sklen, const uint8_t* t, size_t tlen) {
    Blake2b h((const uint8_t*)"MASP__ExpandSeed", 64);
    h.update(sk, sklen);
    h.update(t, tlen);
    h.finalize(out64);
}
// rcm (domain byte 4) or esk (5) of a ZIP 212 rseed (masp_primitives/src/sapling.rs:856-884)
inline void rseed_scalar(uint8_t out32[32], const uint8_t rseed[32], uint8_t domain) {
    uint8_t wide[64];
    prf_expand(wide, rseed, 32, &domain, 1);
    rj_from_bytes_wide(out32, wide);
}
// sapling_ka_agree: [8 sk] P on the full curve
inline JPoint ka_agree(const uint8_t sk[32], const JPoint& p) { return p.mul(sk).mul_by_cofactor(); }
// kdf_sapling: BLAKE2b-256 personalised "MASP__SaplingKDF" over encode(secret) || epk bytes
inline void kdf_sapling(uint8_t key[32], const uint8_t secret[32], const uint8_t epk[32]) {
    Blake2b h((const uint8_t*)"MASP__SaplingKDF", 32);
    h.update(secret, 32);
    h.update(epk, 32);
    h.finalize(key);
}

static const uint8_t NOTE_NONCE[12] = {0};

// epk = [esk] g_d(diversifier), enc = AEAD(kdf([8 esk] pk_d, epk), plaintext).  false: the diversifier has no g_d or pk_d does not decode.
inline bool note_encrypt(const uint8_t esk[32], const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t* plaintext, uint8_t epk[32],
                         uint8_t* enc) {
    JPoint gd, pk;
    if (!group_hash(gd, diversifier, 11, "MASP__gd") || !JPoint::from_bytes(pk, pk_d)) return false;
    gd.mul(esk).to_bytes(epk);
    uint8_t secret[32], key[32];
    ka_agree(esk, pk).to_bytes(secret);
    kdf_sapling(key, secret, epk);
    aead_encrypt(enc, enc + NOTE_PLAINTEXT_SIZE, key, NOTE_NONCE, plaintext, NOTE_PLAINTEXT_SIZE);
    return true;
}

// Everything after decryption, shared by the full and the compact path: sapling_parse_note_plaintext_without_memo (the lead byte,
// AssetType::from_identifier, a canonical rcm for lead byte 1, g_d, pk_d = [ivk] g_d != identity) and check_note_validity (the commitment,
// then for lead byte 2 the ephemeral key the rseed implies).  pt: the first 84 bytes of the note plaintext.
constexpr size_t COMPACT_NOTE_SIZE = 1 + 11 + 8 + 32 + 32;   // the note plaintext without its memo: what a compact output carries
inline bool check_note_plaintext(const uint8_t* pt, const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], int lead_byte,
                                 uint8_t pk_d_out[32]) {
    // sapling_parse_note_plaintext_without_memo
    if (pt[0] != (uint8_t)lead_byte || (lead_byte != 1 && lead_byte != 2)) return false;
    const uint8_t *diversifier = pt + 1, *asset = pt + 20, *r = pt + 52;
    uint64_t value = 0;
    for (int i = 0; i < 8; ++i) value |= (uint64_t)pt[12 + i] << (8 * i);
    JPoint asset_gen, gd;
    if (!asset_generator(asset_gen, asset)) return false;            // AssetType::from_identifier
    if (pt[0] == 1 && !rj_is_canonical(r)) return false;              // jubjub::Fr::from_repr(rcm)
    if (!group_hash(gd, diversifier, 11, "MASP__gd")) return false;   // diversifier.g_d()
    const JPoint pk = gd.mul(ivk);
    if (pk.is_identity()) return false;                               // PaymentAddress::from_parts
    // check_note_validity: the commitment, then (ZIP 212) the ephemeral key the rseed implies
    uint8_t rcm[32], got[32];
    if (pt[0] == 1)
        memcpy(rcm, r, 32);
    else
        rseed_scalar(rcm, r, 4);
    note_commitment(asset_gen, value, gd, pk, rcm).to_affine().u.to_bytes(got);
    if (memcmp(got, cmu, 32) != 0) return false;
    if (pt[0] == 2) {
        uint8_t esk[32];
        rseed_scalar(esk, r, 5);
        gd.mul(esk).to_bytes(got);
        if (memcmp(got, epk, 32) != 0) return false;
    }
    pk.to_bytes(pk_d_out);
    return true;
}

// try_note_decryption_inner: everything after the KDF.  On success the 596-byte plaintext and pk_d = [ivk] g_d are written.
inline bool finish_note_decryption(const uint8_t key[32], const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t* enc,
                                   int lead_byte, uint8_t* plaintext_out, uint8_t pk_d_out[32]) {
    uint8_t pt[NOTE_PLAINTEXT_SIZE], pk[32];
    if (!aead_decrypt(pt, key, NOTE_NONCE, enc, NOTE_PLAINTEXT_SIZE, enc + NOTE_PLAINTEXT_SIZE)) return false;
    if (!check_note_plaintext(pt, ivk, epk, cmu, lead_byte, pk)) return false;
    memcpy(plaintext_out, pt, NOTE_PLAINTEXT_SIZE);
    memcpy(pk_d_out, pk, 32);
    return true;
}

// try_compact_note_decryption_inner (masp_note_encryption/src/lib.rs:607-624): no tag to check: the keystream from block 1 over the 84
// bytes, then the same parsing and validity check.  candidate (may be null): whether decrypted byte 0 equals lead_byte, the only
// cheap filter the compact form has.
inline bool finish_compact_note_decryption(const uint8_t key[32], const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32],
                                           const uint8_t* enc84, int lead_byte, uint8_t* plaintext84_out, uint8_t pk_d_out[32],
                                           bool* candidate = nullptr) {
    uint8_t pt[COMPACT_NOTE_SIZE], pk[32];
    chacha20_xor(pt, enc84, COMPACT_NOTE_SIZE, key, 1, NOTE_NONCE);
    if (candidate) *candidate = pt[0] == (uint8_t)lead_byte;
    if (!check_note_plaintext(pt, ivk, epk, cmu, lead_byte, pk)) return false;
    memcpy(plaintext84_out, pt, COMPACT_NOTE_SIZE);
    memcpy(pk_d_out, pk, 32);
    return true;
}

// try_note_decryption for one ivk and one output
inline bool try_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t* enc, int lead_byte,
                                uint8_t* plaintext_out, uint8_t pk_d_out[32]) {
    JPoint e;
    if (!JPoint::from_bytes(e, epk)) return false;   // Domain::epk
    uint8_t secret[32], key[32];
    ka_agree(ivk, e).to_bytes(secret);
    kdf_sapling(key, secret, epk);
    return finish_note_decryption(key, ivk, epk, cmu, enc, lead_byte, plaintext_out, pk_d_out);
}

// try_compact_note_decryption for one ivk and one compact output (masp_note_encryption/src/lib.rs:589-624)
inline bool try_compact_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t* enc84, int lead_byte,
                                        uint8_t* plaintext84_out, uint8_t pk_d_out[32]) {
    JPoint e;
    if (!JPoint::from_bytes(e, epk)) return false;   // Domain::epk
    uint8_t secret[32], key[32];
    ka_agree(ivk, e).to_bytes(secret);
    kdf_sapling(key, secret, epk);
    return finish_compact_note_decryption(key, ivk, epk, cmu, enc84, lead_byte, plaintext84_out, pk_d_out);
}

}  // namespace masp_host
