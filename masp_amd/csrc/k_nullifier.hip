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
#include "column_host.h"
#include "nullifier_table.h"

using namespace masp;

namespace {

constexpr size_t NF_MAX_NOTES = (size_t)1 << 22;
constexpr size_t NF_CHUNK = (size_t)1 << 19;   // notes per launch sequence: 272 bytes of state, 156 in and 65 out a note, 250 MB in all
constexpr ColumnWidths NF_IN{32, 32, 32, 32, 8, 8, 11, 1};   // ids, pk_ds, rseeds, nks, values, positions, diversifiers, lead bytes
constexpr ColumnWidths NF_OUT{32, 32, 1};                    // cmus, nfs, status
static_assert(sizeof(NfState) == 272 && NF_IN.total == 156 && NF_OUT.total == 65, "NF_CHUNK's sizing");

struct NfHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *nks;
    const uint64_t *values, *positions;
    uint8_t *status, *cmus, *nfs;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall and ends it (end_per_item)
int run_nullifiers(masp_hip_ctx* ctx, size_t n, const NfHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    ColumnCall cc(NF_IN, NF_OUT, column_chunk(0, NF_CHUNK, n));
    int rc;
    if ((rc = w.nf.reserve(cc, sizeof(NfState))) || (rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s))) return rc;
    NfArgs a;   // (the columns in NF_IN's and NF_OUT's order)
    a.in.ids = cc.in<uint32_t>(h.ids), a.in.pk_ds = cc.in<uint32_t>(h.pk_ds), a.in.rseeds = cc.in<uint32_t>(h.rseeds);
    a.in.nks = cc.in<uint32_t>(h.nks), a.in.values = cc.in<uint64_t>(h.values), a.in.positions = cc.in<uint64_t>(h.positions);
    a.in.diversifiers = cc.in(h.divs), a.in.leads = cc.in(h.leads);
    a.state = (NfState*)w.nf.state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.tab = (const JNiels*)w.nf_table.p;
    a.cmus = cc.out<uint32_t>(h.cmus), a.nfs = cc.out<uint32_t>(h.nfs), a.status = cc.out(h.status);
    const int forced = w.nf_lanes.load();
    const int lanes = forced ? forced : n < NF_WIDE_BELOW ? 8 : 1;
    return run_per_item(s, w.nf, cc, n, [&](size_t c) { a.n = (uint32_t)c, nf_enqueue(s, a, lanes); });
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
    return call.done(end_per_item(call.ctx->streams.vk[0], call.w.nf, NF_IN, run_nullifiers(call.ctx, n, h)));
}

int masp_hip_note_nullifiers_configure(masp_hip_ctx* ctx, int lanes_per_note) {
    if (!ctx || (lanes_per_note != 0 && lanes_per_note != 1 && lanes_per_note != 8)) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.nf_lanes.store(lanes_per_note);
    return MASP_HIP_OK;
}

int masp_hip_note_nullifiers_last_timing(masp_hip_ctx* ctx, double ms[3]) { return per_item_last_timing(ctx, &WalletState::nf, ms); }

}  // extern "C"
#endif   // MASP_NF_KERNELS_ONLY
