// Sapling note encryption for MASP on the host: key agreement, KDF, the AEAD, note-plaintext parsing and the full trial decryption of
// `try_sapling_note_decryption` (masp_note_encryption/src/lib.rs:492-577 over masp_primitives/src/sapling/note_encryption.rs:62-86,
// :112-150, :194-260).  The single-output API of the product, the finisher of the GPU scan's hits (k_note_scan.hip stops at the
// tag) and what that scan is tested against; and the compact (ZIP 307) form of lib.rs:589-624, which has no tag and which the GPU's
// compact scan (k_note_scan_compact.hip) is tested and measured against.  And the sender's side: PRF^ock, out_ciphertext, and
// try_output_recovery_with_ovk / _with_ock (masp_note_encryption/src/lib.rs:626-718), the finisher of the GPU's output recovery scan
// (k_out_recovery.hip stops at out_ciphertext's tag) and what that scan is tested and measured against.
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

// sapling_parse_note_plaintext_without_memo up to the point where the paths differ in how they come by pk_d: the lead byte,
// AssetType::from_identifier, a canonical rcm for lead byte 1, diversifier.g_d().  pt: the first 84 bytes of the note plaintext.
constexpr size_t COMPACT_NOTE_SIZE = 1 + 11 + 8 + 32 + 32;   // the note plaintext without its memo: what a compact output carries
struct ParsedNote {
    JPoint asset_gen, gd;
    uint64_t value;
    const uint8_t* r;   // rcm (lead byte 1) or rseed (2), inside pt
};
inline bool parse_note_plaintext(ParsedNote& n, const uint8_t* pt, int lead_byte) {
    if (pt[0] != (uint8_t)lead_byte || (lead_byte != 1 && lead_byte != 2)) return false;
    const uint8_t *diversifier = pt + 1, *asset = pt + 20;
    n.r = pt + 52;
    n.value = 0;
    for (int i = 0; i < 8; ++i) n.value |= (uint64_t)pt[12 + i] << (8 * i);
    if (!asset_generator(n.asset_gen, asset)) return false;             // AssetType::from_identifier
    if (pt[0] == 1 && !rj_is_canonical(n.r)) return false;               // jubjub::Fr::from_repr(rcm)
    return group_hash(n.gd, diversifier, 11, "MASP__gd");                // diversifier.g_d()
}
// check_note_validity: the commitment, then (ZIP 212) the ephemeral key the rseed implies
inline bool check_note_validity(const ParsedNote& n, const uint8_t* pt, const JPoint& pk, const uint8_t epk[32], const uint8_t cmu[32]) {
    uint8_t rcm[32], got[32];
    if (pt[0] == 1)
        memcpy(rcm, n.r, 32);
    else
        rseed_scalar(rcm, n.r, 4);
    note_commitment(n.asset_gen, n.value, n.gd, pk, rcm).to_affine().u.to_bytes(got);
    if (memcmp(got, cmu, 32) != 0) return false;
    if (pt[0] == 2) {
        uint8_t esk[32];
        rseed_scalar(esk, n.r, 5);
        n.gd.mul(esk).to_bytes(got);
        if (memcmp(got, epk, 32) != 0) return false;
    }
    return true;
}

// Everything after decryption, shared by the full and the compact path: sapling_parse_note_plaintext_without_memo (the lead byte,
// AssetType::from_identifier, a canonical rcm for lead byte 1, g_d, pk_d = [ivk] g_d != identity) and check_note_validity (the commitment,
// then for lead byte 2 the ephemeral key the rseed implies).  pt: the first 84 bytes of the note plaintext.
inline bool check_note_plaintext(const uint8_t* pt, const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], int lead_byte,
                                 uint8_t pk_d_out[32]) {
    ParsedNote n;
    if (!parse_note_plaintext(n, pt, lead_byte)) return false;
    const JPoint pk = n.gd.mul(ivk);
    if (pk.is_identity()) return false;                               // PaymentAddress::from_parts
    if (!check_note_validity(n, pt, pk, epk, cmu)) return false;
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

// ---- the sender's side: out_ciphertext and recovery with an ovk (masp_note_encryption/src/lib.rs:450-481, :626-718) ----
constexpr size_t OUT_PLAINTEXT_SIZE = 32 + 32;   // pk_d | esk
constexpr size_t OUT_CIPHERTEXT_SIZE = OUT_PLAINTEXT_SIZE + 16;

// PRF^ock: BLAKE2b-256 personalised "MASP__Derive_ock" over ovk | cv | cmu | epk (sapling/note_encryption.rs:90-110)
inline void prf_ock(uint8_t ock[32], const uint8_t ovk[32], const uint8_t cv[32], const uint8_t cmu[32], const uint8_t epk[32]) {
    Blake2b h((const uint8_t*)"MASP__Derive_ock", 32);
    h.update(ovk, 32);
    h.update(cv, 32);
    h.update(cmu, 32);
    h.update(epk, 32);
    h.finalize(ock);
}
// encrypt_outgoing_plaintext from the ock on: c_out = AEAD(ock, pk_d | esk)
inline void encrypt_outgoing(uint8_t c_out[OUT_CIPHERTEXT_SIZE], const uint8_t ock[32], const uint8_t pk_d[32], const uint8_t esk[32]) {
    uint8_t op[OUT_PLAINTEXT_SIZE];
    memcpy(op, pk_d, 32);
    memcpy(op + 32, esk, 32);
    aead_encrypt(c_out, c_out + OUT_PLAINTEXT_SIZE, ock, NOTE_NONCE, op, OUT_PLAINTEXT_SIZE);
}

// try_output_recovery_with_ock (lib.rs:655-718), in its order.  On success the 596-byte plaintext and pk_d (from op) are written.
inline bool try_output_recovery_with_ock(const uint8_t ock[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t* enc,
                                         const uint8_t c_out[OUT_CIPHERTEXT_SIZE], int lead_byte, uint8_t* plaintext_out, uint8_t pk_d_out[32]) {
    uint8_t op[OUT_PLAINTEXT_SIZE];
    if (!aead_decrypt(op, ock, NOTE_NONCE, c_out, OUT_PLAINTEXT_SIZE, c_out + OUT_PLAINTEXT_SIZE)) return false;
    JPoint pk;
    if (!JPoint::from_bytes(pk, op) || !pk.is_torsion_free()) return false;   // extract_pk_d: jubjub::SubgroupPoint::from_bytes
    const uint8_t* esk = op + 32;
    if (!rj_is_canonical(esk)) return false;                                  // extract_esk: jubjub::Fr::from_repr
    uint8_t secret[32], key[32], pt[NOTE_PLAINTEXT_SIZE], got[32];
    ka_agree(esk, pk).to_bytes(secret);
    kdf_sapling(key, secret, epk);
    if (!aead_decrypt(pt, key, NOTE_NONCE, enc, NOTE_PLAINTEXT_SIZE, enc + NOTE_PLAINTEXT_SIZE)) return false;
    // parse_note_plaintext_without_memo_ovk: pk_d is the one of op once [esk] g_d encodes to epk
    ParsedNote n;
    if (!parse_note_plaintext(n, pt, lead_byte)) return false;
    n.gd.mul(esk).to_bytes(got);
    if (memcmp(got, epk, 32) != 0) return false;
    if (pk.is_identity()) return false;                                       // PaymentAddress::from_parts
    if (pt[0] == 2) {   // ZIP 212: the esk of op is the one the note derives
        rseed_scalar(got, n.r, 5);
        if (memcmp(got, esk, 32) != 0) return false;
    }
    if (!check_note_validity(n, pt, pk, epk, cmu)) return false;
    memcpy(plaintext_out, pt, NOTE_PLAINTEXT_SIZE);
    memcpy(pk_d_out, op, 32);   // (decoding accepts canonical encodings only: these are pk_d's bytes)
    return true;
}

// try_output_recovery_with_ovk (lib.rs:635-644)
inline bool try_output_recovery(const uint8_t ovk[32], const uint8_t cv[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t* enc,
                                const uint8_t c_out[OUT_CIPHERTEXT_SIZE], int lead_byte, uint8_t* plaintext_out, uint8_t pk_d_out[32]) {
    uint8_t ock[32];
    prf_ock(ock, ovk, cv, cmu, epk);
    return try_output_recovery_with_ock(ock, epk, cmu, enc, c_out, lead_byte, plaintext_out, pk_d_out);
}

}  // namespace masp_host
