// Nullifiers and note commitments of a wallet's notes on the GPU: the C ABI entry point masp_hip_sapling_note_nullifiers
// (include/masp_hip.h), Note::cmu and Note::nf(&nk, position) of masp_primitives/src/sapling.rs for n notes at once.
// The steps themselves are device/nullifier.hpp; the kernels are wrappers around them, over a per-note state in global memory, cut so
// that no kernel holds two square roots or a square root next to the Pedersen sum:
//           k_nf_parse     gridDim.y = 2, one lane per (note, group hash): y = 0 the asset generator, y = 1 g_d with its encoding, the
//                          value and rcm (PRF^expand of the rseed for lead byte 2);
//           k_nf_keys      gridDim.y = 2, one lane per (note, key): y = 0 pk_d decodes, y = 1 nk decodes;
//           k_nf_commit    L lanes per note: the note's status from the four checks before, then the 280 Pedersen summands and the
//                          windows of [rcm] G_ncr, a share per lane, folded over __shfl_xor; the group's first lane writes cm and cmu;
//           k_nf_finish    L lanes per note: cm + the windows of [position] G_nf, folded the same way; the first lane encodes rho
//                          and hashes nk | rho.
// A note whose status is set is skipped by the two last kernels; its outputs stay the zeros they were set to.
// One lane per note leaves the chip empty at wallet sizes (4 096 notes are 64 waves on 1 024 SIMDs, each on a chain of about 360
// dependent additions), so the two last kernels exist for L = 8 too: below NF_WIDE_BELOW notes the call uses L = 8.  The bytes are the
// same for both (the affine sums are).
#include "device/nullifier.hpp"
#include "util.h"

namespace masp {

constexpr uint32_t NF_BLOCK = 64;   // a wave per workgroup: a few thousand notes spread over the chip
// Below this many notes a call runs the lane groups of eight.  Measured on an MI355X (tools/nullifier_bench.py: profiles/nullifier_bench.json
// and, between its sizes, profiles/nullifier_bench_crossover.json; DESIGN.md 13 "Lane groups"), the four kernels' time with eight lanes
// against one: 1.84 / 3.21 ms at 256 notes, 1.97 / 3.26 at 4 096, 2.86 / 3.74 at 32 768, 3.96 / 4.16 at 49 152, and then 4.51 / 4.29 at
// 65 536 and 58.3 / 48.3 at 2^20: the crossover lies between the last two measured sizes of either side.
constexpr size_t NF_WIDE_BELOW = 65536;

struct NfArgs {
    NfIn in;
    NfState* state;
    const JNiels* ped;   // the Pedersen Niels table (pedersen_table.h)
    const JNiels* tab;   // G_ncr's windows, then G_nf's (nullifier_table.h)
    uint8_t* status;
    uint32_t* cmus;      // 8 words a note
    uint32_t* nfs;       // 8 words a note
    uint32_t n;
};

__global__ __launch_bounds__(NF_BLOCK) void k_nf_parse(const NfArgs a) {
    const uint32_t i = blockIdx.x * NF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    nf_parse(a.state[i], a.in, i, (int)blockIdx.y);
}

__global__ __launch_bounds__(NF_BLOCK) void k_nf_keys(const NfArgs a) {
    const uint32_t i = blockIdx.x * NF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    nf_key(a.state[i], a.in, i, (int)blockIdx.y);
}

// (a lane group is wholly inside the notes or wholly outside, and a note's status is the same for its lanes: the lanes that fold are
// all there)
template <int L>
__global__ __launch_bounds__(NF_BLOCK) void k_nf_commit(const NfArgs a) {
    static_assert(L == 1 || L == 8, "lanes per note");
    const uint32_t t = blockIdx.x * NF_BLOCK + threadIdx.x, g = t / L, lane = t % L;
    if (g >= a.n) return;
    NfState& st = a.state[g];
    const uint8_t status = nf_status(st);
    if (status != NF_OK) {
        if (lane == 0) a.status[g] = status;
        return;
    }
    const JExt cm = nf_fold<L>(nf_commit_partial(st, a.ped, a.tab, lane, L));
    if (lane != 0) return;
    uint32_t cmu[8];
    nf_commit_finish(st, cm, cmu);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.cmus[8 * (size_t)g + k] = cmu[k];
    a.status[g] = NF_OK;
}

template <int L>
__global__ __launch_bounds__(NF_BLOCK) void k_nf_finish(const NfArgs a) {
    static_assert(L == 1 || L == 8, "lanes per note");
    const uint32_t t = blockIdx.x * NF_BLOCK + threadIdx.x, g = t / L, lane = t % L;
    if (g >= a.n || a.status[g] != NF_OK) return;
    const JExt rho = nf_fold<L>(nf_rho_partial(a.state[g], a.tab + NF_NCR_TABLE, a.in.positions[g], lane, L));
    if (lane != 0) return;
    uint32_t nf[8];
    nf_finish(nf, rho, a.in.nks + 8 * (size_t)g);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.nfs[8 * (size_t)g + k] = nf[k];
}

// the four kernels over a.n >= 1 notes on `s`; lanes: 1 or 8
inline void nf_enqueue(hipStream_t s, const NfArgs& a, int lanes) {
    const uint32_t nb = (a.n + NF_BLOCK - 1) / NF_BLOCK;
    MASP_LAUNCH(k_nf_parse, dim3(nb, 2), dim3(NF_BLOCK), 0, s, a);
    MASP_LAUNCH(k_nf_keys, dim3(nb, 2), dim3(NF_BLOCK), 0, s, a);
    if (lanes == 8) {
        const uint32_t nb8 = (uint32_t)(((uint64_t)a.n * 8 + NF_BLOCK - 1) / NF_BLOCK);
        MASP_LAUNCH(k_nf_commit<8>, dim3(nb8), dim3(NF_BLOCK), 0, s, a);
        MASP_LAUNCH(k_nf_finish<8>, dim3(nb8), dim3(NF_BLOCK), 0, s, a);
    } else {
        MASP_LAUNCH(k_nf_commit<1>, dim3(nb), dim3(NF_BLOCK), 0, s, a);
        MASP_LAUNCH(k_nf_finish<1>, dim3(nb), dim3(NF_BLOCK), 0, s, a);
    }
}

}  // namespace masp

#ifndef MASP_NF_KERNELS_ONLY   // (tests/native/nullifier_dev.hip runs the kernels above for both lane widths without a context)
#include "internal.h"
#include "nullifier_table.h"

using namespace masp;

namespace {

constexpr size_t NF_MAX_NOTES = (size_t)1 << 22;
constexpr size_t NF_CHUNK = (size_t)1 << 19;   // notes per launch sequence: 272 bytes of state, 156 in and 65 out a note, 250 MB in all

struct NfHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *nks;
    const uint64_t *values, *positions;
    uint8_t *status, *cmus, *nfs;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall
int run_nullifiers(masp_hip_ctx* ctx, size_t n, const NfHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const size_t cap = std::min(NF_CHUNK, (n + 63) / 64 * 64);   // every array of the input buffer starts on a multiple of 8 bytes
    int rc;
    if ((rc = w.nf_in.reserve(156 * cap)) || (rc = w.nf_state.reserve(sizeof(NfState) * cap)) || (rc = w.nf_out.reserve(65 * cap)))
        return rc;
    if ((rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s))) return rc;
    uint8_t* in = w.nf_in.p;
    uint8_t *d_ids = in, *d_pk = in + 32 * cap, *d_rs = in + 64 * cap, *d_nk = in + 96 * cap, *d_val = in + 128 * cap, *d_pos = in + 136 * cap,
            *d_div = in + 144 * cap, *d_lead = in + 155 * cap;
    uint8_t *d_cmu = w.nf_out.p, *d_nf = d_cmu + 32 * cap, *d_status = d_cmu + 64 * cap;
    NfArgs a;
    a.in = {(const uint32_t*)d_ids, (const uint64_t*)d_val, d_div, (const uint32_t*)d_pk, d_lead, (const uint32_t*)d_rs, (const uint32_t*)d_nk,
            (const uint64_t*)d_pos};
    a.state = (NfState*)w.nf_state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.tab = (const JNiels*)w.nf_table.p;
    a.status = d_status;
    a.cmus = (uint32_t*)d_cmu;
    a.nfs = (uint32_t*)d_nf;
    const int forced = w.nf_lanes.load();
    const int lanes = forced ? forced : n < NF_WIDE_BELOW ? 8 : 1;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    for (size_t o = 0; o < n; o += cap) {
        const size_t c = std::min(cap, n - o);
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(hipMemcpyAsync(d_ids, h.ids + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pk, h.pk_ds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rs, h.rseeds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_nk, h.nks + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_val, h.values + o, 8 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pos, h.positions + o, 8 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_div, h.divs + 11 * o, 11 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_lead, h.leads + o, c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_cmu, 0, 64 * cap, s));   // a refused note's outputs are zeros
        HIP_TRY(hipEventRecord(ev[1], s));
        a.n = (uint32_t)c;
        nf_enqueue(s, a, lanes);
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipMemcpyAsync(h.status + o, d_status, c, hipMemcpyDeviceToHost, s));
        if (h.cmus) HIP_TRY(hipMemcpyAsync(h.cmus + 32 * o, d_cmu, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.nfs + 32 * o, d_nf, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev[3], s));
        HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        if ((rc = add_elapsed(ev, 3, ms))) return rc;
    }
    w.nf_timing.store(ms);
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_note_nullifiers(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                     const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                     const uint8_t* nks, const uint64_t* positions, uint8_t* status, uint8_t* cmus_out, uint8_t* nfs_out) {
    if (!ctx || n > NF_MAX_NOTES) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) return MASP_HIP_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !nks || !positions || !status || !nfs_out)
        return MASP_HIP_E_INVALID_ARG;
    (void)pedersen_table_bytes();   // built outside the locks
    (void)nullifier_table();
    WalletCall call(ctx);
    const NfHost h = {asset_identifiers, diversifiers, pk_ds, lead_bytes, rseeds, nks, values, positions, status, cmus_out, nfs_out};
    const int rc = run_nullifiers(call.ctx, n, h);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[0]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_note_nullifiers_configure(masp_hip_ctx* ctx, int lanes_per_note) {
    if (!ctx || (lanes_per_note != 0 && lanes_per_note != 1 && lanes_per_note != 8)) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.nf_lanes.store(lanes_per_note);
    return MASP_HIP_OK;
}

int masp_hip_note_nullifiers_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.nf_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
#endif   // MASP_NF_KERNELS_ONLY
