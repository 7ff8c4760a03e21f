// Spend descriptions without their proofs, and RedJubjub signatures, on the GPU: the C ABI entry points masp_hip_sapling_build_spends and
// masp_hip_redjubjub_sign_batch (include/masp_hip.h), what the builder of masp_primitives/src/transaction/components/sapling/builder.rs
// puts around a Spend proof (cv, rk, nf) and spend_sig_internal (sapling.rs:167-195) for n items at once.  The steps
// themselves are device/spend_build.hpp; the kernels are wrappers around them, over a per-item state in global memory, cut as the
// nullifiers' and the outputs' are: no kernel holds two square roots, a square root next to a table sum, or a BLAKE2b state next to a
// point accumulator.
//   signatures, one lane per item:
//           k_rs_key          the range checks of sk and alpha, rsk = sk + alpha, vk = repr([rsk] G_kind) on the basepoint's windows;
//           k_rs_nonce_hash   r = H*(T | vk | sighash): two BLAKE2b blocks and the wide reduction;
//           k_rs_nonce_point  Rbar = repr([r] G_kind);
//           k_rs_finish       c = H*(Rbar | vk | sighash), S = r + c rsk mod r_J, the status; writes Rbar | S and vk, clears rsk and r.
//   spends:
//           k_sb_parse        gridDim.y = 3, one lane per (spend, check): y = 0 the asset generator and [8] g, y = 1 g_d, the value and
//                             rcm, y = 2 pk_d decodes;
//           k_sb_keys         gridDim.y = 3, one lane per (spend, task): y = 0 ak decodes, [8] ak, ar's range, rk = ak + [ar] G_spend,
//                             y = 1 nsk's range and nk = [nsk] G_pgk, y = 2 rcv's range;
//           k_sb_commit       eight lanes per spend: the status from the nine checks before, then the 280 Pedersen summands and the windows
//                             of [rcm] G_ncr, folded over __shfl_xor; the group's first lane writes cmu;
//           k_sb_cv           one lane per spend: [value] [8] g + the windows of [rcv] G_vcr; rk and nk leave the state;
//           k_sb_finish       eight lanes per spend: cm + the windows of [position] G_nf, folded; the first lane hashes nk | rho.
// An item whose status is set is skipped by everything behind the status; its outputs stay the zeros they were set to.
#include "device/spend_build.hpp"
#include "util.h"

namespace masp {

constexpr uint32_t SB_BLOCK = 64;   // a wave per workgroup, as the nullifiers and the outputs
constexpr int SB_LANES = 8;         // lanes per spend in k_sb_commit and k_sb_finish

struct RsArgs {
    RsIn in;
    RsState* state;
    RsTables tab;
    uint8_t* status;
    uint32_t *vks, *sigs;   // 8 and 16 words an item
    uint32_t n;
};

__global__ __launch_bounds__(SB_BLOCK) void k_rs_key(const RsArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    rs_key(a.state[i], a.in, a.tab, i);
}

__global__ __launch_bounds__(SB_BLOCK) void k_rs_nonce_hash(const RsArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n || a.state[i].status != RS_OK) return;
    rs_nonce_hash(a.state[i], a.in, i);
}

__global__ __launch_bounds__(SB_BLOCK) void k_rs_nonce_point(const RsArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n || a.state[i].status != RS_OK) return;
    rs_nonce_point(a.state[i], a.in, a.tab, i);
}

__global__ __launch_bounds__(SB_BLOCK) void k_rs_finish(const RsArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t status = a.state[i].status;
    a.status[i] = (uint8_t)status;
    if (status != RS_OK) return;
    rs_finish(a.state[i], a.in, i, a.sigs + 16 * (size_t)i, a.vks + 8 * (size_t)i);
}

// the four kernels over a.n >= 1 items on `s`
inline void rs_enqueue(hipStream_t s, const RsArgs& a) {
    const uint32_t nb = (a.n + SB_BLOCK - 1) / SB_BLOCK;
    MASP_LAUNCH(k_rs_key, dim3(nb), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_rs_nonce_hash, dim3(nb), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_rs_nonce_point, dim3(nb), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_rs_finish, dim3(nb), dim3(SB_BLOCK), 0, s, a);
}

struct SbArgs {
    SbIn in;
    SbState* state;
    const JNiels *ped, *nft, *vcr, *sbt;   // the Pedersen Niels table; G_ncr's windows, then G_nf's; G_vcr's windows; G_spend's, then G_pgk's
    uint8_t* status;
    uint32_t *cvs, *rks, *nfs, *cmus, *nks;   // 8 words a spend
    uint32_t n;
};

__global__ __launch_bounds__(SB_BLOCK) void k_sb_parse(const SbArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    sb_parse(a.state[i], a.in, i, (int)blockIdx.y);
}

__global__ __launch_bounds__(SB_BLOCK) void k_sb_keys(const SbArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    sb_keys(a.state[i], a.in, a.sbt, i, (int)blockIdx.y);
}

// (a lane group is wholly inside the spends or wholly outside, and a spend's status is the same for its lanes: the lanes that fold are
// all there)
__global__ __launch_bounds__(SB_BLOCK) void k_sb_commit(const SbArgs a) {
    const uint32_t t = blockIdx.x * SB_BLOCK + threadIdx.x, g = t / SB_LANES, lane = t % SB_LANES;
    if (g >= a.n) return;
    SbState& st = a.state[g];
    const uint8_t status = sb_status(st);
    if (status != SB_OK) {
        if (lane == 0) a.status[g] = status;
        return;
    }
    const JExt cm = nf_fold<SB_LANES>(nf_commit_partial(st.ob.nf, a.ped, a.nft, lane, SB_LANES));
    if (lane != 0) return;
    uint32_t cmu[8];
    nf_commit_finish(st.ob.nf, cm, cmu);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.cmus[8 * (size_t)g + k] = cmu[k];
    a.status[g] = SB_OK;
}

__global__ __launch_bounds__(SB_BLOCK) void k_sb_cv(const SbArgs a) {
    const uint32_t i = blockIdx.x * SB_BLOCK + threadIdx.x;
    if (i >= a.n || a.status[i] != SB_OK) return;
    const SbState& st = a.state[i];
    uint32_t cv[8];
    ob_value_commitment(cv, st.ob, a.vcr, a.in.rcvs + 8 * (size_t)i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a.cvs[8 * (size_t)i + k] = cv[k];
        a.rks[8 * (size_t)i + k] = st.rk[k];
        a.nks[8 * (size_t)i + k] = st.nk[k];
    }
}

__global__ __launch_bounds__(SB_BLOCK) void k_sb_finish(const SbArgs a) {
    const uint32_t t = blockIdx.x * SB_BLOCK + threadIdx.x, g = t / SB_LANES, lane = t % SB_LANES;
    if (g >= a.n || a.status[g] != SB_OK) return;
    const SbState& st = a.state[g];
    const JExt rho = nf_fold<SB_LANES>(nf_rho_partial(st.ob.nf, a.nft + NF_NCR_TABLE, a.in.note.positions[g], lane, SB_LANES));
    if (lane != 0) return;
    uint32_t nf[8];
    nf_finish(nf, rho, st.nk);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.nfs[8 * (size_t)g + k] = nf[k];
}

// the five kernels over a.n >= 1 spends on `s`
inline void sb_enqueue(hipStream_t s, const SbArgs& a) {
    const uint32_t nb = (a.n + SB_BLOCK - 1) / SB_BLOCK, nb8 = (uint32_t)(((uint64_t)a.n * SB_LANES + SB_BLOCK - 1) / SB_BLOCK);
    MASP_LAUNCH(k_sb_parse, dim3(nb, 3), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_sb_keys, dim3(nb, 3), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_sb_commit, dim3(nb8), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_sb_cv, dim3(nb), dim3(SB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_sb_finish, dim3(nb8), dim3(SB_BLOCK), 0, s, a);
}

}  // namespace masp

#ifndef MASP_SB_KERNELS_ONLY   // (tests/native/spend_build_dev.hip runs the kernels above without a context)
#include "column_host.h"
#include "spend_table.h"

using namespace masp;

namespace {

constexpr size_t SB_MAX_ITEMS = (size_t)1 << 20;
// items per launch sequence.  Spends: 252 bytes in, 664 of state and 161 out a spend, 71 MB in all; signatures: 177 in, 132 of state, 97 out.
constexpr size_t SB_CHUNK = (size_t)1 << 16;
// nsks, ars, rcvs (the secret ones stand first: 96 and 144 bytes an item of pinned staging); ids, pk_ds, rseeds, aks, values, positions, diversifiers, lead bytes
constexpr ColumnWidths SB_IN{{32, 32, 32, 32, 32, 32, 32, 8, 8, 11, 1}, 0b111};
constexpr ColumnWidths SB_OUT{32, 32, 32, 32, 32, 1};        // cvs, rks, nfs, cmus, nks, status
constexpr ColumnWidths RS_IN{{32, 32, 80, 32, 1}, 0b111};    // sks, alphas, randoms; sighashes, kinds
constexpr ColumnWidths RS_OUT{32, 64, 1};                    // vks, sigs, status
static_assert(SB_IN.total == 252 && sizeof(SbState) == 664 && SB_OUT.total == 161 && SB_IN.stage_total == 96, "SB_CHUNK's sizing: spends");
static_assert(RS_IN.total == 177 && sizeof(RsState) == 132 && RS_OUT.total == 97 && RS_IN.stage_total == 144, "SB_CHUNK's sizing: signatures");

struct RsHost {
    const uint8_t *sks, *alphas, *sighashes, *kinds, *randoms;
    uint8_t *status, *vks, *sigs;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall and ends it (end_per_item: the scrub)
int run_sign(masp_hip_ctx* ctx, size_t n, const RsHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    ColumnCall cc(RS_IN, RS_OUT, column_chunk(w.rs.chunk.load(), SB_CHUNK, n));
    int rc;
    if ((rc = w.rs.reserve(cc, sizeof(RsState))) || (rc = spend_table_ensure(w, s)) || (rc = output_table_ensure(w, s))) return rc;
    RsArgs a;   // (the columns in RS_IN's and RS_OUT's order)
    a.in.sks = cc.in<uint32_t>(h.sks), a.in.alphas = cc.in<uint32_t>(h.alphas), a.in.randoms = cc.in<uint32_t>(h.randoms);
    a.in.sighashes = cc.in<uint32_t>(h.sighashes), a.in.kinds = cc.in(h.kinds);
    a.state = (RsState*)w.rs.state.p;
    a.tab = {{(const JNiels*)w.sb_table.p, (const JNiels*)w.ob_table.p}};
    a.vks = cc.out<uint32_t>(h.vks), a.sigs = cc.out<uint32_t>(h.sigs), a.status = cc.out(h.status);
    return run_per_item(s, w.rs, cc, n, [&](size_t c) { a.n = (uint32_t)c, rs_enqueue(s, a); });
}

struct SbHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *aks, *nsks, *ars, *rcvs;
    const uint64_t *values, *positions;
    uint8_t *status, *cvs, *rks, *nfs, *cmus, *nks;
};

int run_build_spends(masp_hip_ctx* ctx, size_t n, const SbHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    ColumnCall cc(SB_IN, SB_OUT, column_chunk(w.sb.chunk.load(), SB_CHUNK, n));
    int rc;
    if ((rc = w.sb.reserve(cc, sizeof(SbState))) || (rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s)) ||
        (rc = output_table_ensure(w, s)) || (rc = spend_table_ensure(w, s)))
        return rc;
    SbArgs a;   // (the columns in SB_IN's and SB_OUT's order)
    a.in.nsks = cc.in<uint32_t>(h.nsks), a.in.ars = cc.in<uint32_t>(h.ars), a.in.rcvs = cc.in<uint32_t>(h.rcvs);
    a.in.note.ids = cc.in<uint32_t>(h.ids), a.in.note.pk_ds = cc.in<uint32_t>(h.pk_ds), a.in.note.rseeds = cc.in<uint32_t>(h.rseeds);
    a.in.aks = cc.in<uint32_t>(h.aks), a.in.note.values = cc.in<uint64_t>(h.values), a.in.note.positions = cc.in<uint64_t>(h.positions);
    a.in.note.diversifiers = cc.in(h.divs), a.in.note.leads = cc.in(h.leads);
    a.in.note.nks = nullptr;
    a.state = (SbState*)w.sb.state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.nft = (const JNiels*)w.nf_table.p;
    a.vcr = (const JNiels*)w.ob_table.p;
    a.sbt = (const JNiels*)w.sb_table.p;
    a.cvs = cc.out<uint32_t>(h.cvs), a.rks = cc.out<uint32_t>(h.rks), a.nfs = cc.out<uint32_t>(h.nfs);
    a.cmus = cc.out<uint32_t>(h.cmus), a.nks = cc.out<uint32_t>(h.nks), a.status = cc.out(h.status);
    return run_per_item(s, w.sb, cc, n, [&](size_t c) { a.n = (uint32_t)c, sb_enqueue(s, a); });
}

}  // namespace

extern "C" {

int masp_hip_redjubjub_sign_batch(masp_hip_ctx* ctx, size_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes,
                                  const uint8_t* kinds, const uint8_t* randoms, uint8_t* status, uint8_t* vks_out, uint8_t* sigs_out) {
    if (!ctx || n > SB_MAX_ITEMS) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) return MASP_HIP_OK;
    if (!sks || !sighashes || !kinds || !randoms || !status || !sigs_out) return MASP_HIP_E_INVALID_ARG;
    for (size_t i = 0; i < n; ++i)
        if (kinds[i] > 1) return MASP_HIP_E_INVALID_ARG;
    (void)spend_table();   // built outside the locks
    (void)output_table();
    WalletCall call(ctx);
    const RsHost h = {sks, alphas, sighashes, kinds, randoms, status, vks_out, sigs_out};
    return call.done(end_per_item(call.ctx->streams.vk[0], call.w.rs, RS_IN, run_sign(call.ctx, n, h)));
}

int masp_hip_redjubjub_sign_configure(masp_hip_ctx* ctx, size_t chunk_items) { return per_item_configure(ctx, &WalletState::rs, chunk_items, SB_CHUNK); }

int masp_hip_redjubjub_sign_last_timing(masp_hip_ctx* ctx, double ms[3]) { return per_item_last_timing(ctx, &WalletState::rs, ms); }

int masp_hip_sapling_build_spends(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                  const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                  const uint8_t* aks, const uint8_t* nsks, const uint8_t* ars, const uint8_t* rcvs, const uint64_t* positions,
                                  uint8_t* status, uint8_t* cvs_out, uint8_t* rks_out, uint8_t* nfs_out, uint8_t* cmus_out, uint8_t* nks_out) {
    if (!ctx || n > SB_MAX_ITEMS) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) return MASP_HIP_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !aks || !nsks || !ars || !rcvs || !positions ||
        !status || !cvs_out || !rks_out || !nfs_out)
        return MASP_HIP_E_INVALID_ARG;
    (void)pedersen_table_bytes();   // built outside the locks
    (void)nullifier_table();
    (void)output_table();
    (void)spend_table();
    WalletCall call(ctx);
    const SbHost h = {asset_identifiers, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, values, positions,
                      status,            cvs_out,      rks_out, nfs_out,  cmus_out, nks_out};
    return call.done(end_per_item(call.ctx->streams.vk[0], call.w.sb, SB_IN, run_build_spends(call.ctx, n, h)));
}

int masp_hip_build_spends_configure(masp_hip_ctx* ctx, size_t chunk_spends) { return per_item_configure(ctx, &WalletState::sb, chunk_spends, SB_CHUNK); }

int masp_hip_build_spends_last_timing(masp_hip_ctx* ctx, double ms[3]) { return per_item_last_timing(ctx, &WalletState::sb, ms); }

}  // extern "C"
#endif   // MASP_SB_KERNELS_ONLY
