// Batch output recovery with outgoing viewing keys on the GPU: the C ABI entry point masp_hip_sapling_output_recovery_scan
// (include/masp_hip.h), the device half of try_sapling_output_recovery (masp_primitives/src/sapling/note_encryption.rs:539-551 over
// masp_note_encryption/src/lib.rs:635-718) for outputs x ovks.
//
// For every (output, ovk) pair the device does what is done for EVERY pair: PRF^ock (one BLAKE2b compression), ChaCha20 block 0 for the
// Poly1305 key and Poly1305 over the 64 ciphertext bytes of out_ciphertext, compared with its tag (device/out_recovery.hpp).  It does not
// decrypt and does no curve arithmetic: the pairs that fail the tag (all but the caller's own sent notes) are finished, and the rare
// pair that passes goes back to the host with its ock, where masp_host_sapling_try_output_recovery_with_ock does everything else
// (DESIGN.md).
//
// Kernels:  k_or_repitch  the 176 bytes of an output (cv, cmu, epk, out_ciphertext) into eleven 16-byte columns, once per output;
//           k_or_trial    one lane per pair, the ovk constant across the workgroup (blockIdx.y): its four message words are wave-uniform
//                         and come from scalar loads, the per-pair reads are whole lines per wave.
#include <mutex>

#include "device/out_recovery.hpp"
#include "scan_host.h"

using namespace masp;

namespace {

constexpr size_t OR_OUT = 80;   // out_ciphertext: pk_d | esk under ChaCha20, the 16-byte tag

// cols[c * n_pad + o] = column c of output o (out_recovery.hpp: OR_COLS).  Lanes run along o: the writes and k_or_trial's reads are whole
// lines per wave; the strided reads happen here, once per output instead of once per pair.
__global__ __launch_bounds__(NS_BLOCK) void k_or_repitch(const uint4* __restrict__ cvs, const uint4* __restrict__ cmus,
                                                         const uint4* __restrict__ epks, const uint4* __restrict__ couts, uint32_t n,
                                                         uint32_t n_pad, uint4* __restrict__ cols) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x, c = blockIdx.y;   // (c: uniform)
    if (o >= n) return;
    uint4 v;
    if (c < 2)
        v = cvs[2 * (size_t)o + c];
    else if (c < 4)
        v = cmus[2 * (size_t)o + (c - 2)];
    else if (c < 6)
        v = epks[2 * (size_t)o + (c - 4)];
    else
        v = couts[5 * (size_t)o + (c - 6)];
    cols[(size_t)c * n_pad + o] = v;
}

// hits: count[0] pairs verified their tag; pair i < cap is (hit_idx[i] = output, ovk) with its ock in hit_ocks[2 i], [2 i + 1]
__global__ __launch_bounds__(NS_BLOCK) void k_or_trial(const uint32_t* __restrict__ ovks, const uint4* __restrict__ cols, uint32_t n,
                                                       uint32_t n_pad, uint32_t out_base, uint32_t* __restrict__ count, uint32_t cap,
                                                       uint2* __restrict__ hit_idx, uint4* __restrict__ hit_ocks) {
    const uint32_t o = blockIdx.x * NS_BLOCK + threadIdx.x, k = blockIdx.y;
    if (o >= n) return;
    uint32_t ock[8];
    if (!or_pair(ock, ovks + 8 * (size_t)k, cols + o, n_pad)) return;   // (ovks + 8 k: wave-uniform, scalar loads)
    const uint32_t slot = atomicAdd(count, 1u);
    if (slot >= cap) return;   // (cap is the launch's pair count: cannot happen; the count still tells)
    hit_idx[slot] = make_uint2(out_base + o, k);
    hit_ocks[2 * slot] = make_uint4(ock[0], ock[1], ock[2], ock[3]);
    hit_ocks[2 * slot + 1] = make_uint4(ock[4], ock[5], ock[6], ock[7]);
}

struct Rows {
    const uint8_t *cvs, *epks, *cmus, *couts;
};

// enqueues one chunk of outputs on its stream: upload, repitch, trials, and the count's way back
int enqueue_chunk(masp_hip_ctx* ctx, const ChunkInFlight& c, ScanSetHost<3>& h, size_t n_ovk, const Rows& r, uint32_t* h_count) {
    WalletState& w = ctx->wallet;
    WalletState::OutRecoverySet& b = w.orc[c.set];
    hipStream_t s = ctx->streams.vk[c.set];
    const uint32_t n = (uint32_t)c.n, nb = (n + NS_BLOCK - 1) / NS_BLOCK, n_pad = nb * NS_BLOCK;
    const size_t cap = c.n * n_ovk;
    int rc;
    if ((rc = b.cv.reserve(32 * (size_t)n_pad)) || (rc = b.cmu.reserve(32 * (size_t)n_pad)) || (rc = b.epk.reserve(32 * (size_t)n_pad)) ||
        (rc = b.cout.reserve(OR_OUT * (size_t)n_pad)) || (rc = b.cols.reserve(16 * (size_t)OR_COLS * n_pad)) || (rc = b.count.reserve(1)) ||
        (rc = b.hit_idx.reserve(2 * cap)) || (rc = b.hit_ocks.reserve(32 * cap)))
        return rc;
    if ((rc = create_events(h.ev))) return rc;
    HIP_TRY(hipEventRecord(h.ev[0], s));
    HIP_TRY(hipMemcpyAsync(b.cv.p, r.cvs + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.cmu.p, r.cmus + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.epk.p, r.epks + 32 * c.o0, 32 * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.cout.p, r.couts + OR_OUT * c.o0, OR_OUT * c.n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b.count.p, 0, sizeof(uint32_t), s));
    HIP_TRY(hipEventRecord(h.ev[1], s));
    MASP_LAUNCH(k_or_repitch, dim3(nb, OR_COLS), dim3(NS_BLOCK), 0, s, (const uint4*)b.cv.p, (const uint4*)b.cmu.p, (const uint4*)b.epk.p,
                (const uint4*)b.cout.p, n, n_pad, (uint4*)b.cols.p);
    MASP_LAUNCH(k_or_trial, dim3(nb, (uint32_t)n_ovk), dim3(NS_BLOCK), 0, s, (const uint32_t*)w.orc_ovks.p, (const uint4*)b.cols.p, n, n_pad,
                (uint32_t)c.o0, b.count.p, (uint32_t)cap, (uint2*)b.hit_idx.p, (uint4*)b.hit_ocks.p);
    HIP_TRY(hipEventRecord(h.ev[2], s));
    HIP_TRY(hipMemcpyAsync(h_count, b.count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_output_recovery_scan(masp_hip_ctx* ctx, size_t n_ovk, const uint8_t* ovks, size_t n_out, const uint8_t* cvs,
                                          const uint8_t* epks, const uint8_t* cmus, const uint8_t* out_ciphertexts, size_t hit_capacity,
                                          uint32_t* hit_output, uint32_t* hit_ovk, uint8_t* hit_ocks, size_t* n_hits) {
    if (!ctx || !n_hits || (n_ovk && !ovks) || (n_out && (!cvs || !epks || !cmus || !out_ciphertexts)) || n_ovk > NS_MAX_IVKS ||
        n_out > NS_MAX_OUTPUTS || (hit_capacity && (!hit_output || !hit_ovk || !hit_ocks)))
        return MASP_HIP_E_INVALID_ARG;
    *n_hits = 0;
    if (n_ovk == 0 || n_out == 0) return MASP_HIP_OK;   // (an ovk is any 32 bytes: nothing to refuse)
    std::vector<uint32_t> words(8 * n_ovk);
    memcpy(words.data(), ovks, 32 * n_ovk);   // (little-endian host)
    WalletCall call(ctx);
    ctx = call.ctx;
    WalletState& w = call.w;
    int rc;
    if ((rc = w.orc_ovks.upload(words.data(), words.size(), ctx->streams.vk[0]))) return call.done(rc);
    if (hipStreamSynchronize(ctx->streams.vk[0]) != hipSuccess) {   // both streams read the ovks
        last_hip_error() = std::string("output recovery scan: upload failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    // chunks of outputs, alternately on the two verifier streams with a buffer set each (chunk_pipeline.h)
    const Rows rows = {cvs, epks, cmus, out_ciphertexts};
    ScanSetHost<3> host[2];   // events: before the upload, behind it, behind the kernels
    uint32_t h_count[2] = {0, 0};
    std::vector<ScanHit<32>> hits;
    double ms[2] = {0, 0};
    rc = run_chunks(
        n_out, chunk_outputs(n_ovk),
        [&](const ChunkInFlight& c) { return enqueue_chunk(ctx, c, host[c.set], n_ovk, rows, &h_count[c.set]); },
        [&](const ChunkInFlight& c) {
            const WalletState::OutRecoverySet& b = w.orc[c.set];
            return scan_collect(
                ctx->streams.vk[c.set], c, host[c.set], [&](size_t& nh) { return (nh = h_count[c.set]) <= c.n * n_ovk; },
                "output recovery scan: hit count beyond the chunk's pairs", nullptr, nullptr, b.hit_idx.p, b.hit_ocks.p, hits, ms);
        },
        [&](int set) { (void)hipStreamSynchronize(ctx->streams.vk[set]); });
    if (rc) return call.done(rc);
    w.orc_timing.store(ms);
    return call.done(scan_finish(hits, hit_capacity, hit_output, hit_ovk, hit_ocks, 32, nullptr, n_hits));
}

int masp_hip_out_recovery_last_timing(masp_hip_ctx* ctx, double ms[2]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.orc_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
