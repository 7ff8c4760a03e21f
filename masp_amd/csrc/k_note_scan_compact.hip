// Compact (ZIP 307) batch trial decryption of Sapling notes on the GPU: the C ABI entry point masp_hip_sapling_compact_trial_decrypt
// (include/masp_hip.h), masp_note_encryption::batch::try_compact_note_decryption over SaplingDomain (masp_note_encryption/src/batch.rs:35,
// lib.rs:589-624).  A compact output carries epk, cmu and the first 84 bytes of enc_ciphertext: no tag.  The only cheap test is the lead
// byte, which one random pair in 256 passes, and what remains to tell a note from noise is the note commitment.  So the WHOLE check runs
// here and the hits are final.
//
// Stage 1, every pair:      k_ns_decode (k_note_scan.hip) once per output, then
//           k_nsc_trial     one lane per pair, the ivk in blockIdx.y with wave-uniform digits: the ladder and the KDF of the full scan
//                           (device/note_scan.hpp), ChaCha20 block 1, byte 0 against the lead byte; survivors go through an atomic
//                           counter into the candidate list (output, ivk, key).
// Stage 2, candidates only, one lane each, the per-candidate state in global memory, every kernel over the survivors of the one before;
// the steps themselves are device/compact_note.hpp (cut in four so that no kernel holds three ladders, two square roots and the hash at once: DESIGN.md 8):
//           k_nsc_parse     decrypts the 84 bytes (blocks 1 and 2), parses; the asset generator, a canonical rcm for lead byte 1, g_d and its
//                           affine form and encoding;
//           k_nsc_pkd       pk_d = [ivk] g_d with the ivk as a per-lane scalar, refused if it is the identity; its encoding;
//           k_nsc_commit    the Pedersen hash from the table, rcm, + [rcm] G_ncr, the affine u against cmu;
//           k_nsc_esk       lead byte 2: esk from the rseed, [esk] g_d, its encoding against epk;
//           k_nsc_emit      (output, ivk, plaintext, pk_d) of the pairs that passed, packed.
// The stage 2 kernels are launched over the launch's pair count, the bound of the candidate count, with 64-lane workgroups whose lanes
// leave when they are beyond the count they read from device memory: no host round trip between the stages (KERNELS.md).
#include <mutex>

#include "device/compact_note.hpp"
#include "device/note_scan.hpp"
#include "host/jubjub.h"
#include "scan_host.h"
#include "pedersen_table.h"

using namespace masp;

namespace {

constexpr size_t NSC_ENC = 84;
constexpr uint32_t NSC_BLOCK2 = 64;   // stage 2: a wave per workgroup, so that a thousand candidates spread over the chip

struct NscCand {
    uint32_t out, ivk;   // the output's index in the chunk, the ivk's in the list
    uint32_t key[8];
};

// counts: [0] the candidates, [1 + k] the survivors of stage 2's kernel k; lists: survivors' candidate slots, list k at lists + k * cap
struct NscArgs {
    uint32_t* counts;
    const NscCand* cand;
    NscState* state;
    uint32_t* lists;
    uint32_t cap;
    const uint32_t* enc;     // the chunk's rows of 21 words
    const uint32_t* epks;    // 8 words each
    const uint32_t* cmus;    // 8 words each
    const uint32_t* ivks;    // 8 words each
    const JNiels* table;     // PED_NC_TABLE points, then G_ncr as a JExt
    int lead;
};

__global__ __launch_bounds__(NS_BLOCK) void k_nsc_trial(const uint32_t* __restrict__ digits, const JNiels* __restrict__ pts,
                                                        const uint8_t* __restrict__ status, const uint4* __restrict__ epks,
                                                        const uint32_t* __restrict__ enc, uint32_t n, int inversion, uint32_t lead,
                                                        uint32_t* __restrict__ count, uint32_t cap, NscCand* __restrict__ cand) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x, k = blockIdx.y;
    if (o >= n || status[o] != JJ_OK) return;
    const JNiels q = pts[o];
    uint32_t key[8];
    ns_pair_key(key, digits + 16 * k, q, epks + 2 * o, inversion);
    const uint32_t nonce[3] = {0, 0, 0};
    uint32_t b1[16];
    chacha20_block(b1, key, 1, nonce);
    if (((b1[0] ^ enc[(size_t)NSC_ENC_WORDS * o]) & 0xffu) != lead) return;
    const uint32_t slot = atomicAdd(count, 1u);
    if (slot >= cap) return;   // (cap is the launch's pair count: cannot happen)
    NscCand c;
    c.out = o;
    c.ivk = k;
#pragma unroll
    for (int i = 0; i < 8; ++i) c.key[i] = key[i];
    cand[slot] = c;
}

// the slot of survivor i of list `from` (from < 0: the candidates themselves), or false beyond the count
__device__ __forceinline__ bool nsc_slot(const NscArgs& a, int from, uint32_t& slot) {
    const uint32_t i = blockIdx.x * NSC_BLOCK2 + threadIdx.x;
    const uint32_t n = min(a.counts[from + 1], a.cap);
    if (i >= n) return false;
    slot = from < 0 ? i : a.lists[(size_t)from * a.cap + i];
    return slot < a.cap;
}

__device__ __forceinline__ void nsc_pass(const NscArgs& a, int to, uint32_t slot) {
    const uint32_t p = atomicAdd(a.counts + to + 1, 1u);
    if (p < a.cap) a.lists[(size_t)to * a.cap + p] = slot;
}

__global__ __launch_bounds__(NSC_BLOCK2) void k_nsc_parse(const NscArgs a) {
    uint32_t slot;
    if (!nsc_slot(a, -1, slot)) return;
    const NscCand c = a.cand[slot];
    if (nsc_parse(a.state[slot], c.key, a.enc + (size_t)NSC_ENC_WORDS * c.out, a.lead)) nsc_pass(a, 0, slot);
}

__global__ __launch_bounds__(NSC_BLOCK2) void k_nsc_pkd(const NscArgs a) {
    uint32_t slot;
    if (!nsc_slot(a, 0, slot)) return;
    if (nsc_pkd(a.state[slot], a.ivks + 8 * (size_t)a.cand[slot].ivk)) nsc_pass(a, 1, slot);
}

__global__ __launch_bounds__(NSC_BLOCK2) void k_nsc_commit(const NscArgs a) {
    uint32_t slot;
    if (!nsc_slot(a, 1, slot)) return;
    if (nsc_commit(a.state[slot], a.table, a.cmus + 8 * (size_t)a.cand[slot].out, a.lead)) nsc_pass(a, 2, slot);
}

__global__ __launch_bounds__(NSC_BLOCK2) void k_nsc_esk(const NscArgs a) {
    uint32_t slot;
    if (!nsc_slot(a, 2, slot)) return;
    if (nsc_esk(a.state[slot], a.epks + 8 * (size_t)a.cand[slot].out)) nsc_pass(a, 3, slot);
}

// hit i of the final list: idx[i] = (output, ivk), data[29 i ..] = the 21 plaintext words and the 8 of pk_d
__global__ __launch_bounds__(NSC_BLOCK2) void k_nsc_emit(const NscArgs a, int from, uint32_t out_base, uint2* __restrict__ idx,
                                                         uint32_t* __restrict__ data) {
    uint32_t slot;
    if (!nsc_slot(a, from, slot)) return;
    const uint32_t i = blockIdx.x * NSC_BLOCK2 + threadIdx.x;
    const NscState& st = a.state[slot];
    idx[i] = make_uint2(out_base + a.cand[slot].out, a.cand[slot].ivk);
    uint32_t* d = data + 29 * (size_t)i;
    for (int j = 0; j < 21; ++j) d[j] = st.pt[j];
    for (int j = 0; j < 8; ++j) d[21 + j] = st.msg[18 + j];
}

// enqueues one chunk of outputs on its stream: upload, decode, stage 1, stage 2, and the counts' way back
int enqueue_chunk(masp_hip_ctx* ctx, const ChunkInFlight& c, ScanSetHost<4>& h, size_t n_ivk, const uint8_t* epks, const uint8_t* cmus,
                  const uint8_t* encs, int lead, uint32_t* h_counts) {
    WalletState& w = ctx->wallet;
    WalletState::NoteScanSet& b = w.ns[c.set];
    WalletState::NoteScanCompactSet& x = w.nsc[c.set];
    hipStream_t s = ctx->streams.vk[c.set];
    const uint32_t n = (uint32_t)c.n, nb = (n + NS_BLOCK - 1) / NS_BLOCK, n_pad = nb * NS_BLOCK;
    const size_t cap = c.n * n_ivk;
    int rc;
    if ((rc = b.epk.reserve(32 * (size_t)n_pad)) || (rc = b.pts.reserve(sizeof(JNiels) * (size_t)n_pad)) || (rc = b.status.reserve(n_pad)) ||
        (rc = x.cmu.reserve(32 * (size_t)n_pad)) || (rc = x.enc.reserve(NSC_ENC * (size_t)n_pad)) || (rc = x.count.reserve(5)) ||
        (rc = x.cand.reserve(sizeof(NscCand) * cap)) || (rc = x.state.reserve(sizeof(NscState) * cap)) || (rc = x.list.reserve(4 * cap)) ||
        (rc = x.hit_idx.reserve(8 * cap)) || (rc = x.hit_data.reserve(116 * cap)))
        return rc;
    if ((rc = create_events(h.ev))) return rc;
    HIP_TRY(hipEventRecord(h.ev[0], s));
    HIP_TRY(hipMemcpyAsync(b.epk.p, epks + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(x.cmu.p, cmus + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(x.enc.p, encs + NSC_ENC * c.o0, NSC_ENC * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(x.count.p, 0, 5 * sizeof(uint32_t), s));
    HIP_TRY(hipEventRecord(h.ev[1], s));
    launch_ns_decode(s, b.epk.p, n, b.status.p, b.pts.p);
    MASP_LAUNCH(k_nsc_trial, dim3(nb, (uint32_t)n_ivk), dim3(NS_BLOCK), 0, s, (const uint32_t*)w.ns_digits.p, (const JNiels*)b.pts.p,
                (const uint8_t*)b.status.p, (const uint4*)b.epk.p, (const uint32_t*)x.enc.p, n, w.ns_inversion.load(), (uint32_t)lead,
                x.count.p, (uint32_t)cap, (NscCand*)x.cand.p);
    HIP_TRY(hipEventRecord(h.ev[2], s));
    NscArgs a;
    a.counts = x.count.p;
    a.cand = (const NscCand*)x.cand.p;
    a.state = (NscState*)x.state.p;
    a.lists = x.list.p;
    a.cap = (uint32_t)cap;
    a.enc = (const uint32_t*)x.enc.p;
    a.epks = (const uint32_t*)b.epk.p;
    a.cmus = (const uint32_t*)x.cmu.p;
    a.ivks = (const uint32_t*)w.nsc_ivks.p;
    a.table = (const JNiels*)w.nsc_table.p;
    a.lead = lead;
    const dim3 grid2((uint32_t)((cap + NSC_BLOCK2 - 1) / NSC_BLOCK2)), block2(NSC_BLOCK2);
    MASP_LAUNCH(k_nsc_parse, grid2, block2, 0, s, a);
    MASP_LAUNCH(k_nsc_pkd, grid2, block2, 0, s, a);
    MASP_LAUNCH(k_nsc_commit, grid2, block2, 0, s, a);
    if (lead == 2) MASP_LAUNCH(k_nsc_esk, grid2, block2, 0, s, a);
    MASP_LAUNCH(k_nsc_emit, grid2, block2, 0, s, a, lead == 2 ? 3 : 2, (uint32_t)c.o0, (uint2*)x.hit_idx.p, (uint32_t*)x.hit_data.p);
    HIP_TRY(hipEventRecord(h.ev[3], s));
    HIP_TRY(hipMemcpyAsync(h_counts, x.count.p, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_compact_trial_decrypt(masp_hip_ctx* ctx, size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks,
                                           const uint8_t* cmus, const uint8_t* enc_compact, int lead_byte, uint8_t* epk_status,
                                           size_t hit_capacity, uint32_t* hit_output, uint32_t* hit_ivk, uint8_t* hit_plaintexts,
                                           uint8_t* hit_pk_d, size_t* n_hits, size_t* n_candidates) {
    if (!ctx || !n_hits || (n_ivk && !ivks) || (n_out && (!epks || !cmus || !enc_compact)) || n_ivk > NS_MAX_IVKS || n_out > NS_MAX_OUTPUTS ||
        (lead_byte != 1 && lead_byte != 2) || (hit_capacity && (!hit_output || !hit_ivk || !hit_plaintexts || !hit_pk_d)))
        return MASP_HIP_E_INVALID_ARG;
    *n_hits = 0;
    if (n_candidates) *n_candidates = 0;
    std::vector<uint32_t> digits;
    if (ns_recode_ivks(digits, n_ivk, ivks, FIRST_DEVICE(ctx)->wallet.ns_signed_digits.load() != 0)) return MASP_HIP_E_INVALID_ARG;
    if (n_ivk == 0 || n_out == 0) {
        if (epk_status && n_out) memset(epk_status, 0, n_out);   // (not looked at: no key asked for them)
        return MASP_HIP_OK;
    }
    (void)pedersen_table_bytes();   // built outside the locks
    WalletCall call(ctx);
    ctx = call.ctx;
    WalletState& w = call.w;
    int rc;
    if ((rc = w.ns_digits.upload(digits.data(), digits.size(), ctx->streams.vk[0])) ||
        (rc = w.nsc_ivks.upload(ivks, 32 * n_ivk, ctx->streams.vk[0])) ||
        (rc = pedersen_table_ensure(w, ctx->streams.vk[0])))   // (shared with the trees and the nullifiers)
        return call.done(rc);
    if (hipStreamSynchronize(ctx->streams.vk[0]) != hipSuccess) {   // both streams read the digits, the ivks and the table
        last_hip_error() = std::string("compact note scan: upload failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    // chunks of outputs, alternately on the two verifier streams with a buffer set each (chunk_pipeline.h): a chunk's upload and stage 1
    // run beside the thin stage 2 of the chunk before
    ScanSetHost<4> host[2];   // events: before the upload, behind it, behind stage 1, behind stage 2
    uint32_t h_counts[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
    std::vector<ScanHit<116>> hits;   // plaintext 84 | pk_d 32
    size_t candidates = 0;
    double ms[3] = {0, 0, 0};
    rc = run_chunks(
        n_out, chunk_outputs(n_ivk),
        [&](const ChunkInFlight& c) { return enqueue_chunk(ctx, c, host[c.set], n_ivk, epks, cmus, enc_compact, lead_byte, h_counts[c.set]); },
        [&](const ChunkInFlight& c) {
            const WalletState::NoteScanCompactSet& x = w.nsc[c.set];
            auto count = [&](size_t& nh) {   // the candidates of stage 1, of them the survivors of stage 2
                const size_t nc = h_counts[c.set][0];
                nh = h_counts[c.set][lead_byte == 2 ? 4 : 3];
                if (nc > c.n * n_ivk || nh > nc) return false;
                candidates += nc;
                return true;
            };
            return scan_collect(ctx->streams.vk[c.set], c, host[c.set], count, "compact note scan: a count beyond the chunk's pairs", epk_status,
                                w.ns[c.set].status.p, x.hit_idx.p, x.hit_data.p, hits, ms);
        },
        [&](int set) { (void)hipStreamSynchronize(ctx->streams.vk[set]); });
    if (rc) return call.done(rc);
    w.nsc_timing.store(ms);
    if (n_candidates) *n_candidates = candidates;
    return call.done(scan_finish(hits, hit_capacity, hit_output, hit_ivk, hit_plaintexts, 84, hit_pk_d, n_hits));
}

int masp_hip_note_scan_compact_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.nsc_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
