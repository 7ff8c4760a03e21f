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
#include "internal.h"
#include "spend_table.h"

using namespace masp;

namespace {

constexpr size_t SB_MAX_ITEMS = (size_t)1 << 20;
// items per launch sequence.  Spends: 252 bytes in, 704 of state and 161 out a spend, 73 MB in all; signatures: 177 in, 132 of state, 97 out.
constexpr size_t SB_CHUNK = (size_t)1 << 16;

size_t chunk_cap(size_t configured, size_t n) {
    return std::min(configured ? configured : SB_CHUNK, (n + 63) / 64 * 64);   // every array of the input buffer starts on a multiple of 8 bytes
}

struct RsHost {
    const uint8_t *sks, *alphas, *sighashes, *kinds, *randoms;
    uint8_t *status, *vks, *sigs;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall and scrubs behind it
int run_sign(masp_hip_ctx* ctx, size_t n, const RsHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const size_t cap = chunk_cap(w.rs_chunk.load(), n);
    const size_t n_pad = (cap + SB_BLOCK - 1) / SB_BLOCK * SB_BLOCK;
    int rc;
    if ((rc = w.rs_in.reserve(177 * n_pad)) || (rc = w.rs_state.reserve(sizeof(RsState) * n_pad)) || (rc = w.rs_out.reserve(97 * n_pad)) ||
        (rc = w.rs_stage.reserve(144 * n_pad)))
        return rc;
    if ((rc = spend_table_ensure(w, s)) || (rc = output_table_ensure(w, s))) return rc;
    uint8_t* in = w.rs_in.p;
    uint8_t *d_sk = in, *d_al = in + 32 * n_pad, *d_rnd = in + 64 * n_pad, *d_sh = in + 144 * n_pad, *d_kind = in + 176 * n_pad;
    uint8_t *p_sk = w.rs_stage.p, *p_al = p_sk + 32 * n_pad, *p_rnd = p_sk + 64 * n_pad;   // the secrets' pinned staging
    uint8_t* out = w.rs_out.p;
    uint8_t *d_vk = out, *d_sig = out + 32 * n_pad, *d_status = out + 96 * n_pad;
    RsArgs a;
    a.in = {(const uint32_t*)d_sk, h.alphas ? (const uint32_t*)d_al : nullptr, (const uint32_t*)d_sh, d_kind, (const uint32_t*)d_rnd};
    a.state = (RsState*)w.rs_state.p;
    a.tab = {{(const JNiels*)w.sb_table.p, (const JNiels*)w.ob_table.p}};
    a.status = d_status;
    a.vks = (uint32_t*)d_vk;
    a.sigs = (uint32_t*)d_sig;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    for (size_t o = 0; o < n; o += cap) {
        const size_t c = std::min(cap, n - o);
        memcpy(p_sk, h.sks + 32 * o, 32 * c);
        if (h.alphas) memcpy(p_al, h.alphas + 32 * o, 32 * c);
        memcpy(p_rnd, h.randoms + 80 * o, 80 * c);
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(hipMemcpyAsync(d_sk, p_sk, 32 * c, hipMemcpyHostToDevice, s));
        if (h.alphas) HIP_TRY(hipMemcpyAsync(d_al, p_al, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rnd, p_rnd, 80 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_sh, h.sighashes + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_kind, h.kinds + o, c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(out, 0, 96 * n_pad, s));   // a refused item's outputs are zeros
        HIP_TRY(hipEventRecord(ev[1], s));
        a.n = (uint32_t)c;
        rs_enqueue(s, a);
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipMemcpyAsync(h.status + o, d_status, c, hipMemcpyDeviceToHost, s));
        if (h.vks) HIP_TRY(hipMemcpyAsync(h.vks + 32 * o, d_vk, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.sigs + 64 * o, d_sig, 64 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev[3], s));
        HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        if ((rc = add_elapsed(ev, 3, ms))) return rc;
    }
    w.rs_timing.store(ms);
    return MASP_HIP_OK;
}

// What a call leaves of its secrets, on success and on every error path, before the wallet lock is released: the uploaded inputs (the
// secret ones among them) and the per-item state on the device, the pinned staging on the host.  (A failed memset is not reported over the call's own result.)
void scrub(hipStream_t s, DevBuf<uint8_t>& in, DevBuf<uint8_t>& state, PinnedBuf<uint8_t>& stage) {
    if (in.p) (void)hipMemsetAsync(in.p, 0, in.cap, s);
    if (state.p) (void)hipMemsetAsync(state.p, 0, state.cap, s);
    (void)hipStreamSynchronize(s);
    if (stage.p) memset(stage.p, 0, stage.cap);
}

struct SbHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *aks, *nsks, *ars, *rcvs;
    const uint64_t *values, *positions;
    uint8_t *status, *cvs, *rks, *nfs, *cmus, *nks;
};

int run_build_spends(masp_hip_ctx* ctx, size_t n, const SbHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const size_t cap = chunk_cap(w.sb_chunk.load(), n);
    const size_t n_pad = (cap + SB_BLOCK - 1) / SB_BLOCK * SB_BLOCK;
    int rc;
    if ((rc = w.sb_in.reserve(252 * n_pad)) || (rc = w.sb_state.reserve(sizeof(SbState) * n_pad)) || (rc = w.sb_out.reserve(161 * n_pad)) ||
        (rc = w.sb_stage.reserve(96 * n_pad)))
        return rc;
    if ((rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s)) || (rc = output_table_ensure(w, s)) || (rc = spend_table_ensure(w, s)))
        return rc;
    uint8_t* in = w.sb_in.p;
    uint8_t *d_nsk = in, *d_ar = in + 32 * n_pad, *d_rcv = in + 64 * n_pad, *d_ids = in + 96 * n_pad, *d_pk = in + 128 * n_pad, *d_rs = in + 160 * n_pad,
            *d_ak = in + 192 * n_pad, *d_val = in + 224 * n_pad, *d_pos = in + 232 * n_pad, *d_div = in + 240 * n_pad, *d_lead = in + 251 * n_pad;
    uint8_t *p_nsk = w.sb_stage.p, *p_ar = p_nsk + 32 * n_pad, *p_rcv = p_nsk + 64 * n_pad;
    uint8_t* out = w.sb_out.p;
    uint8_t *d_cv = out, *d_rk = out + 32 * n_pad, *d_nf = out + 64 * n_pad, *d_cmu = out + 96 * n_pad, *d_nk = out + 128 * n_pad, *d_status = out + 160 * n_pad;
    SbArgs a;
    a.in.note = {(const uint32_t*)d_ids, (const uint64_t*)d_val, d_div, (const uint32_t*)d_pk, d_lead, (const uint32_t*)d_rs, nullptr, (const uint64_t*)d_pos};
    a.in.aks = (const uint32_t*)d_ak;
    a.in.nsks = (const uint32_t*)d_nsk;
    a.in.ars = (const uint32_t*)d_ar;
    a.in.rcvs = (const uint32_t*)d_rcv;
    a.state = (SbState*)w.sb_state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.nft = (const JNiels*)w.nf_table.p;
    a.vcr = (const JNiels*)w.ob_table.p;
    a.sbt = (const JNiels*)w.sb_table.p;
    a.status = d_status;
    a.cvs = (uint32_t*)d_cv;
    a.rks = (uint32_t*)d_rk;
    a.nfs = (uint32_t*)d_nf;
    a.cmus = (uint32_t*)d_cmu;
    a.nks = (uint32_t*)d_nk;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    for (size_t o = 0; o < n; o += cap) {
        const size_t c = std::min(cap, n - o);
        memcpy(p_nsk, h.nsks + 32 * o, 32 * c);
        memcpy(p_ar, h.ars + 32 * o, 32 * c);
        memcpy(p_rcv, h.rcvs + 32 * o, 32 * c);
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(hipMemcpyAsync(d_nsk, p_nsk, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ar, p_ar, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rcv, p_rcv, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ids, h.ids + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pk, h.pk_ds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rs, h.rseeds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ak, h.aks + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_val, h.values + o, 8 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pos, h.positions + o, 8 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_div, h.divs + 11 * o, 11 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_lead, h.leads + o, c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(out, 0, 160 * n_pad, s));   // a refused spend's outputs are zeros
        HIP_TRY(hipEventRecord(ev[1], s));
        a.n = (uint32_t)c;
        sb_enqueue(s, a);
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipMemcpyAsync(h.status + o, d_status, c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.cvs + 32 * o, d_cv, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.rks + 32 * o, d_rk, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.nfs + 32 * o, d_nf, 32 * c, hipMemcpyDeviceToHost, s));
        if (h.cmus) HIP_TRY(hipMemcpyAsync(h.cmus + 32 * o, d_cmu, 32 * c, hipMemcpyDeviceToHost, s));
        if (h.nks) HIP_TRY(hipMemcpyAsync(h.nks + 32 * o, d_nk, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev[3], s));
        HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        if ((rc = add_elapsed(ev, 3, ms))) return rc;
    }
    w.sb_timing.store(ms);
    return MASP_HIP_OK;
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
    const int rc = run_sign(call.ctx, n, h);
    scrub(call.ctx->streams.vk[0], call.w.rs_in, call.w.rs_state, call.w.rs_stage);   // (waits for the stream: nothing of this call stays in flight)
    return call.done(rc);
}

int masp_hip_redjubjub_sign_configure(masp_hip_ctx* ctx, size_t chunk_items) {
    if (!ctx || chunk_items > SB_CHUNK) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.rs_chunk.store(chunk_items);
    return MASP_HIP_OK;
}

int masp_hip_redjubjub_sign_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.rs_timing.load(ms);
    return MASP_HIP_OK;
}

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
    const int rc = run_build_spends(call.ctx, n, h);
    scrub(call.ctx->streams.vk[0], call.w.sb_in, call.w.sb_state, call.w.sb_stage);   // (waits for the stream: nothing of this call stays in flight)
    return call.done(rc);
}

int masp_hip_build_spends_configure(masp_hip_ctx* ctx, size_t chunk_spends) {
    if (!ctx || chunk_spends > SB_CHUNK) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.sb_chunk.store(chunk_spends);
    return MASP_HIP_OK;
}

int masp_hip_build_spends_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.sb_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
#endif   // MASP_SB_KERNELS_ONLY
