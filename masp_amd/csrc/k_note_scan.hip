// Batch trial decryption of Sapling notes on the GPU: the C ABI entry point masp_hip_sapling_trial_decrypt (include/masp_hip.h), the
// device half of masp_note_encryption::batch::try_note_decryption over SaplingDomain (masp_note_encryption/src/batch.rs:43-86).
//
// For every (output, ivk) pair the device does what is done for EVERY pair: the key agreement [8 ivk] epk, the KDF (one BLAKE2b
// compression), ChaCha20 block 0 for the Poly1305 key and Poly1305 over the ciphertext, compared with the tag.  It does not decrypt:
// the tag is over the ciphertext, so the pairs that fail it (all but the caller's own notes) are finished, and the rare pair that
// passes goes back to the host with its symmetric key, where masp_host_sapling_finish_note_decryption decrypts, parses and checks the
// commitment.
//
// Kernels:  k_ns_decode   one lane per output: jj_decode of epk once, not once per ivk, stored in the affine form (v - u, v + u, 2d u v)
//                         that makes the ladder's additions mixed ones of 7 products, and a status byte;
//           k_ns_repitch  the 612-byte ciphertext rows into 16-byte columns (KERNELS.md: why);
//                         (also the first kernel of the compact scan, k_note_scan_compact.hip);
//           k_ns_trial    one lane per pair, the ivk constant across the workgroup (blockIdx.y): the scalar's digits are wave-uniform, so the
//                         `if (digit)` of the double-and-add is a uniform branch, the scalar lives in SGPRs and no lane needs a table.
#include <mutex>

#include "device/blake2b.hpp"
#include "device/chacha20.hpp"
#include "device/jubjub.hpp"
#include "device/note_scan.hpp"
#include "device/poly1305.hpp"
#include "scan_host.h"

using namespace masp;

namespace {

constexpr size_t NS_ENC = 612;            // enc_ciphertext: 596 bytes of note plaintext under ChaCha20, the 16-byte tag
constexpr uint32_t NS_ENC_WORDS = 153;
constexpr uint32_t NS_COLS = 39;          // 16-byte columns of a repitched row (156 words: three of padding)

__global__ __launch_bounds__(NS_BLOCK) void k_ns_decode(const uint4* __restrict__ epks, uint32_t n, uint8_t* __restrict__ status,
                                                        JNiels* __restrict__ pts) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x;
    if (o >= n) return;
    const uint4 p0 = epks[2 * o], p1 = epks[2 * o + 1];
    const uint32_t w[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    JExt p;
    const int rc = jj_decode(p, w);
    status[o] = (uint8_t)rc;
    if (rc != JJ_OK) return;
    pts[o] = {fe_sub(p.V, p.U), fe_add(p.V, p.U), fe_mul(p.T, fr_lit(JubjubCfg::D2))};   // (Z = 1: T = u v)
}

// raw: n rows of 153 words; ct4[c * n_pad + o] = words 4c .. 4c + 3 of row o (zero beyond the row).  Lanes run along o: the writes and
// k_ns_trial's reads are whole 1 KiB lines per wave, the strided reads happen here, once per output instead of once per pair.
__global__ __launch_bounds__(NS_BLOCK) void k_ns_repitch(const uint32_t* __restrict__ raw, uint32_t n, uint32_t n_pad, uint4* __restrict__ ct4) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x, c = blockIdx.y;
    if (o >= n) return;
    const uint32_t* row = raw + (size_t)o * NS_ENC_WORDS;
    uint4 v;
    v.x = row[4 * c];   // (4 * 38 = 152: the last column holds one word)
    v.y = 4 * c + 1 < NS_ENC_WORDS ? row[4 * c + 1] : 0u;
    v.z = 4 * c + 2 < NS_ENC_WORDS ? row[4 * c + 2] : 0u;
    v.w = 4 * c + 3 < NS_ENC_WORDS ? row[4 * c + 3] : 0u;
    ct4[(size_t)c * n_pad + o] = v;
}

// digits: per ivk 16 words, [0..7] the mask of non-zero digits of its (plain or signed) binary recoding, [8..15] the mask of negative ones.
// hits: count[0] pairs verified their tag; pair i < cap is (hit_idx[i] = output, ivk) with its key in hit_keys[2 i], [2 i + 1].
// inversion: 0 the divstep inverse, 1 the binary-gcd one (field.hpp), for the one inversion of the encoding.
__global__ __launch_bounds__(NS_BLOCK) void k_ns_trial(const uint32_t* __restrict__ digits, const JNiels* __restrict__ pts,
                                                       const uint8_t* __restrict__ status, const uint4* __restrict__ epks,
                                                       const uint4* __restrict__ ct4, uint32_t n, uint32_t n_pad, uint32_t out_base, int inversion,
                                                       uint32_t* __restrict__ count, uint32_t cap, uint2* __restrict__ hit_idx,
                                                       uint4* __restrict__ hit_keys) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x, k = blockIdx.y;
    if (o >= n || status[o] != JJ_OK) return;
    const JNiels q = pts[o];
    uint32_t key[8];
    ns_pair_key(key, digits + 16 * k, q, epks + 2 * o, inversion);   // (digits: wave-uniform, scalar loads)
    const uint32_t nonce[3] = {0, 0, 0};
    uint32_t b0[16];
    chacha20_block(b0, key, 0, nonce);
    Poly1305State st;
    poly1305_init(st, b0);
    const uint4* col = ct4 + o;
#pragma unroll 4
    for (uint32_t c = 0; c < 37; ++c) {
        const uint4 x = col[(size_t)c * n_pad];
        poly1305_block(st, x.x, x.y, x.z, x.w);
    }
    const uint4 x37 = col[(size_t)37 * n_pad], x38 = col[(size_t)38 * n_pad];
    poly1305_block(st, x37.x, 0, 0, 0);     // bytes 592 .. 595, zero-padded to the block (the AEAD's pad16: a whole block)
    poly1305_block(st, 0, 0, 596, 0);       // the lengths: no associated data, 596 bytes of ciphertext
    uint32_t tag[4];
    poly1305_finish(st, b0 + 4, tag);
    if (tag[0] != x37.y || tag[1] != x37.z || tag[2] != x37.w || tag[3] != x38.x) return;
    const uint32_t slot = atomicAdd(count, 1u);
    if (slot >= cap) return;   // (cap is the launch's pair count: cannot happen; the count still tells)
    hit_idx[slot] = make_uint2(out_base + o, k);
    hit_keys[2 * slot] = make_uint4(key[0], key[1], key[2], key[3]);
    hit_keys[2 * slot + 1] = make_uint4(key[4], key[5], key[6], key[7]);
}

// the digit masks of k_ns_trial for one ivk.  signed_digits: the non-adjacent form (digits -1, 0, 1, no two neighbours non-zero: a third
// of the positions instead of half, at most 253 of them for k < 2^252); otherwise the plain binary digits.
void recode(uint32_t out[16], const uint32_t k_in[8], bool signed_digits) {
    memset(out, 0, 64);
    if (!signed_digits) {
        memcpy(out, k_in, 32);
        return;
    }
    uint32_t k[8];
    memcpy(k, k_in, 32);
    for (int pos = 0; pos < 256; ++pos) {
        if (k[0] & 1u) {
            out[pos >> 5] |= 1u << (pos & 31);
            if ((k[0] & 3u) == 3u) {   // digit -1: k += 1 (k < 2^253: no overflow)
                out[8 + (pos >> 5)] |= 1u << (pos & 31);
                for (int i = 0; i < 8 && ++k[i] == 0; ++i) {
                }
            } else {
                k[0] &= ~1u;
            }
        }
        for (int i = 0; i < 7; ++i) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
        k[7] >>= 1;
    }
}

// enqueues one chunk of outputs on its stream: upload, decode, repitch, trials, and the count's way back
int enqueue_chunk(masp_hip_ctx* ctx, const ChunkInFlight& c, ScanSetHost<3>& h, size_t n_ivk, const uint8_t* epks, const uint8_t* encs,
                  uint32_t* h_count) {
    WalletState& w = ctx->wallet;
    WalletState::NoteScanSet& b = w.ns[c.set];
    hipStream_t s = ctx->streams.vk[c.set];
    const uint32_t n = (uint32_t)c.n, nb = (n + NS_BLOCK - 1) / NS_BLOCK, n_pad = nb * NS_BLOCK;
    const size_t cap = c.n * n_ivk;
    int rc;
    if ((rc = b.epk.reserve(32 * (size_t)n_pad)) || (rc = b.raw.reserve(NS_ENC * (size_t)n_pad)) || (rc = b.ct.reserve(16 * (size_t)NS_COLS * n_pad)) ||
        (rc = b.pts.reserve(sizeof(JNiels) * (size_t)n_pad)) || (rc = b.status.reserve(n_pad)) || (rc = b.count.reserve(1)) ||
        (rc = b.hit_idx.reserve(2 * cap)) || (rc = b.hit_keys.reserve(32 * cap)))
        return rc;
    if ((rc = create_events(h.ev))) return rc;
    HIP_TRY(hipEventRecord(h.ev[0], s));
    HIP_TRY(hipMemcpyAsync(b.epk.p, epks + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.raw.p, encs + NS_ENC * c.o0, NS_ENC * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b.count.p, 0, sizeof(uint32_t), s));
    HIP_TRY(hipEventRecord(h.ev[1], s));
    launch_ns_decode(s, b.epk.p, n, b.status.p, b.pts.p);
    MASP_LAUNCH(k_ns_repitch, dim3(nb, NS_COLS), dim3(NS_BLOCK), 0, s, (const uint32_t*)b.raw.p, n, n_pad, (uint4*)b.ct.p);
    MASP_LAUNCH(k_ns_trial, dim3(nb, (uint32_t)n_ivk), dim3(NS_BLOCK), 0, s, (const uint32_t*)w.ns_digits.p, (const JNiels*)b.pts.p,
                (const uint8_t*)b.status.p, (const uint4*)b.epk.p, (const uint4*)b.ct.p, n, n_pad, (uint32_t)c.o0, w.ns_inversion.load(),
                b.count.p, (uint32_t)cap, (uint2*)b.hit_idx.p, (uint4*)b.hit_keys.p);
    HIP_TRY(hipEventRecord(h.ev[2], s));
    HIP_TRY(hipMemcpyAsync(h_count, b.count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return MASP_HIP_OK;
}

}  // namespace

namespace masp {

int ns_recode_ivks(std::vector<uint32_t>& digits, size_t n_ivk, const uint8_t* ivks, bool signed_digits) {
    digits.assign(16 * n_ivk, 0);
    for (size_t k = 0; k < n_ivk; ++k) {
        uint32_t w[8];
        memcpy(w, ivks + 32 * k, 32);   // (little-endian host)
        if (!rj_is_canonical(w)) return MASP_HIP_E_INVALID_ARG;   // a SaplingIvk is a canonical scalar below r_J
        recode(&digits[16 * k], w, signed_digits);
    }
    return MASP_HIP_OK;
}

void launch_ns_decode(hipStream_t s, const uint8_t* epks, uint32_t n, uint8_t* status, uint8_t* pts) {
    MASP_LAUNCH(k_ns_decode, dim3((n + NS_BLOCK - 1) / NS_BLOCK), dim3(NS_BLOCK), 0, s, (const uint4*)epks, n, status, (JNiels*)pts);
}

}  // namespace masp

extern "C" {

int masp_hip_sapling_trial_decrypt(masp_hip_ctx* ctx, size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks,
                                   const uint8_t* enc_ciphertexts, uint8_t* epk_status, size_t hit_capacity, uint32_t* hit_output, uint32_t* hit_ivk,
                                   uint8_t* hit_keys, size_t* n_hits) {
    if (!ctx || !n_hits || (n_ivk && !ivks) || (n_out && (!epks || !enc_ciphertexts)) || n_ivk > NS_MAX_IVKS || n_out > NS_MAX_OUTPUTS ||
        (hit_capacity && (!hit_output || !hit_ivk || !hit_keys)))
        return MASP_HIP_E_INVALID_ARG;
    *n_hits = 0;
    std::vector<uint32_t> digits;
    if (ns_recode_ivks(digits, n_ivk, ivks, FIRST_DEVICE(ctx)->wallet.ns_signed_digits.load() != 0)) return MASP_HIP_E_INVALID_ARG;
    if (n_ivk == 0 || n_out == 0) {
        if (epk_status && n_out) memset(epk_status, 0, n_out);   // (not looked at: no key asked for them)
        return MASP_HIP_OK;
    }
    WalletCall call(ctx);
    ctx = call.ctx;
    WalletState& w = call.w;
    int rc;
    if ((rc = w.ns_digits.upload(digits.data(), digits.size(), ctx->streams.vk[0]))) return call.done(rc);
    if (hipStreamSynchronize(ctx->streams.vk[0]) != hipSuccess) {   // both streams read the digits
        last_hip_error() = std::string("note scan: upload failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    // chunks of outputs, alternately on the two verifier streams with a buffer set each (chunk_pipeline.h)
    ScanSetHost<3> host[2];   // events: before the upload, behind it, behind the kernels
    uint32_t h_count[2] = {0, 0};
    std::vector<ScanHit<32>> hits;
    double ms[2] = {0, 0};
    rc = run_chunks(
        n_out, chunk_outputs(n_ivk),
        [&](const ChunkInFlight& c) { return enqueue_chunk(ctx, c, host[c.set], n_ivk, epks, enc_ciphertexts, &h_count[c.set]); },
        [&](const ChunkInFlight& c) {
            const WalletState::NoteScanSet& b = w.ns[c.set];
            return scan_collect(
                ctx->streams.vk[c.set], c, host[c.set], [&](size_t& nh) { return (nh = h_count[c.set]) <= c.n * n_ivk; },
                "note scan: hit count beyond the chunk's pairs", epk_status, b.status.p, b.hit_idx.p, b.hit_keys.p, hits, ms);
        },
        [&](int set) { (void)hipStreamSynchronize(ctx->streams.vk[set]); });
    if (rc) return call.done(rc);
    w.ns_timing.store(ms);
    return call.done(scan_finish(hits, hit_capacity, hit_output, hit_ivk, hit_keys, 32, nullptr, n_hits));
}

int masp_hip_note_scan_configure(masp_hip_ctx* ctx, int signed_digits, int inversion) {
    if (!ctx || signed_digits < 0 || signed_digits > 1 || inversion < 0 || inversion > 1) return MASP_HIP_E_INVALID_ARG;
    WalletState& w = FIRST_DEVICE(ctx)->wallet;
    w.ns_signed_digits.store(signed_digits);
    w.ns_inversion.store(inversion);
    return MASP_HIP_OK;
}

int masp_hip_note_scan_last_timing(masp_hip_ctx* ctx, double ms[2]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.ns_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
