// Output descriptions without their proofs on the GPU: the C ABI entry point masp_hip_sapling_build_outputs (include/masp_hip.h), what
// SaplingOutputInfo::build of masp_primitives/src/transaction/components/sapling/builder.rs puts around an Output proof, cv, cmu, epk,
// enc_ciphertext and out_ciphertext, for n outputs at once.  The steps themselves are device/output_build.hpp; the kernels
// are wrappers around them, over a per-output state in global memory, cut as the nullifiers' are (k_nullifier.hip), so that no kernel holds
// two square roots or a square root next to a ladder:
//           k_ob_parse     gridDim.y = 4, one lane per (output, check): y = 0 the asset generator and [8] g, y = 1 g_d, y = 2 pk_d decodes,
//                          y = 3 rcm, esk (PRF^expand of the rseed for lead byte 2) and rcv's range;
//           k_ob_memo      the 512-byte memo rows into 16-byte columns, as k_ns_repitch does for the scans (not launched without memos);
//           k_ob_commit    eight lanes per output: the output's status from the six checks before, then the 280 Pedersen summands and the
//                          windows of [rcm] G_ncr, a share per lane, folded over __shfl_xor; the group's first lane writes cmu;
//           k_ob_cv        one lane per output: [value] [8] g on cv_mul64, + the windows of [rcv] G_vcr;
//           k_ob_ladder    gridDim.y = 2, one lane per (output, ladder): y = 0 epk = [esk] g_d, y = 1 the secret [8 esk] pk_d; the scalars
//                          differ per lane, so this is jj_mul;
//           k_ob_seal      one lane per output: the KDF, ChaCha20 blocks 0 to 10, 39 Poly1305 blocks, PRF^ock and the small AEAD; the two
//                          ciphertexts leave in 16-byte columns, lanes along the outputs, and the memo is read from such columns;
//           k_ob_rows      the columns into the 612- and 80-byte rows the caller gets, one lane per word of a row: the stores are
//                          consecutive words, the strided accesses are four-byte loads, once per output (KERNELS.md: why).
// An output whose status is set is skipped by everything behind k_ob_commit; its outputs stay the zeros they were set to.
#include "device/output_build.hpp"
#include "util.h"

namespace masp {

constexpr uint32_t OB_BLOCK = 64;   // a wave per workgroup, as the nullifiers: a few thousand outputs spread over the chip
constexpr int OB_LANES = 8;         // lanes per output in k_ob_commit

struct ObArgs {
    ObIn in;
    ObState* state;
    const JNiels *ped, *ncr, *vcr;   // the Pedersen Niels table, G_ncr's windows, G_vcr's windows
    const uint4* memo_rows;          // 32 columns a row as they come, or null: every memo is the empty one
    uint4* memo_cols;
    uint4* cols;                     // [c * n_pad + o], c < OB_COLS
    uint8_t* status;
    uint32_t *cvs, *cmus, *epks;     // 8 words an output
    uint32_t *encs, *couts;          // 153 and 20 words an output
    uint32_t n, n_pad;
};

__global__ __launch_bounds__(OB_BLOCK) void k_ob_parse(const ObArgs a) {
    const uint32_t i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    ob_parse(a.state[i], a.in, i, (int)blockIdx.y);
}

__global__ __launch_bounds__(OB_BLOCK) void k_ob_memo(const ObArgs a) {
    const uint32_t o = blockIdx.x * OB_BLOCK + threadIdx.x, c = blockIdx.y;
    if (o >= a.n) return;
    a.memo_cols[(size_t)c * a.n_pad + o] = a.memo_rows[(size_t)o * OB_MEMO_COLS + c];
}

// (a lane group is wholly inside the outputs or wholly outside, and an output's status is the same for its lanes: the lanes that fold are
// all there)
__global__ __launch_bounds__(OB_BLOCK) void k_ob_commit(const ObArgs a) {
    const uint32_t t = blockIdx.x * OB_BLOCK + threadIdx.x, g = t / OB_LANES, lane = t % OB_LANES;
    if (g >= a.n) return;
    ObState& st = a.state[g];
    const uint8_t status = ob_status(st);
    if (status != OB_OK) {
        if (lane == 0) a.status[g] = status;
        return;
    }
    const JExt cm = nf_fold<OB_LANES>(nf_commit_partial(st.nf, a.ped, a.ncr, lane, OB_LANES));
    if (lane != 0) return;
    uint32_t cmu[8];
    nf_commit_finish(st.nf, cm, cmu);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.cmus[8 * (size_t)g + k] = cmu[k];
    a.status[g] = OB_OK;
}

__global__ __launch_bounds__(OB_BLOCK) void k_ob_cv(const ObArgs a) {
    const uint32_t i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= a.n || a.status[i] != OB_OK) return;
    uint32_t cv[8];
    ob_value_commitment(cv, a.state[i], a.vcr, a.in.rcvs + 8 * (size_t)i);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.cvs[8 * (size_t)i + k] = cv[k];
}

__global__ __launch_bounds__(OB_BLOCK) void k_ob_ladder(const ObArgs a) {
    const uint32_t i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= a.n || a.status[i] != OB_OK) return;
    ob_ladder(a.state[i], a.epks + 8 * (size_t)i, (int)blockIdx.y);
}

__global__ __launch_bounds__(OB_BLOCK) void k_ob_seal(const ObArgs a) {
    const uint32_t i = blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= a.n || a.status[i] != OB_OK) return;
    ob_seal(a.state[i], a.in, i, a.cvs + 8 * (size_t)i, a.cmus + 8 * (size_t)i, a.epks + 8 * (size_t)i, a.memo_rows ? a.memo_cols + i : nullptr,
            a.n_pad, a.cols + i, a.n_pad);
}

// one lane per word of an output's 153 + 20: a wave stores 256 consecutive bytes
__global__ __launch_bounds__(256) void k_ob_rows(const ObArgs a) {
    constexpr uint32_t WORDS = OB_ENC_WORDS + OB_OUT_WORDS;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t o = (uint32_t)(t / WORDS), w = (uint32_t)(t % WORDS);
    if (o >= a.n || a.status[o] != OB_OK) return;
    const uint32_t* cols = (const uint32_t*)a.cols;
    if (w < OB_ENC_WORDS) {
        a.encs[(size_t)o * OB_ENC_WORDS + w] = cols[4 * ((size_t)(w >> 2) * a.n_pad + o) + (w & 3u)];
    } else {
        const uint32_t v = w - OB_ENC_WORDS;
        a.couts[(size_t)o * OB_OUT_WORDS + v] = cols[4 * ((size_t)(OB_ENC_COLS + (v >> 2)) * a.n_pad + o) + (v & 3u)];
    }
}

// the seven kernels over a.n >= 1 outputs on `s`
inline void ob_enqueue(hipStream_t s, const ObArgs& a) {
    const uint32_t nb = (a.n + OB_BLOCK - 1) / OB_BLOCK;
    MASP_LAUNCH(k_ob_parse, dim3(nb, 4), dim3(OB_BLOCK), 0, s, a);
    if (a.memo_rows) MASP_LAUNCH(k_ob_memo, dim3(nb, OB_MEMO_COLS), dim3(OB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_ob_commit, dim3((uint32_t)(((uint64_t)a.n * OB_LANES + OB_BLOCK - 1) / OB_BLOCK)), dim3(OB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_ob_cv, dim3(nb), dim3(OB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_ob_ladder, dim3(nb, 2), dim3(OB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_ob_seal, dim3(nb), dim3(OB_BLOCK), 0, s, a);
    MASP_LAUNCH(k_ob_rows, dim3((uint32_t)(((uint64_t)a.n * (OB_ENC_WORDS + OB_OUT_WORDS) + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace masp

#ifndef MASP_OB_KERNELS_ONLY   // (tests/native/output_build_dev.hip runs the kernels above without a context)
#include "internal.h"
#include "output_table.h"

using namespace masp;

namespace {

constexpr size_t OB_MAX_OUTPUTS = (size_t)1 << 20;
// outputs per launch sequence: 309 bytes in, 512 of memo twice, 592 of state, 704 of columns and 789 out an output, 225 MB in all
constexpr size_t OB_CHUNK = (size_t)1 << 16;

struct ObHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *esks, *rcvs, *memos, *ovks, *flags, *randoms;
    const uint64_t* values;
    uint8_t *status, *cvs, *cmus, *epks, *encs, *couts;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall
int run_build_outputs(masp_hip_ctx* ctx, size_t n, const ObHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const size_t configured = w.ob_chunk.load();
    const size_t cap = std::min(configured ? configured : OB_CHUNK, (n + 63) / 64 * 64);   // every array of the input buffer starts on a multiple of 8 bytes
    const size_t n_pad = (cap + OB_BLOCK - 1) / OB_BLOCK * OB_BLOCK;
    int rc;
    if ((rc = w.ob_in.reserve(309 * n_pad)) || (rc = w.ob_state.reserve(sizeof(ObState) * n_pad)) || (rc = w.ob_cols.reserve(16 * (size_t)OB_COLS * n_pad)) ||
        (rc = w.ob_out.reserve(789 * n_pad)) || (h.memos && (rc = w.ob_memo.reserve(2 * 512 * n_pad))))
        return rc;
    if ((rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s)) || (rc = output_table_ensure(w, s))) return rc;
    uint8_t* in = w.ob_in.p;
    uint8_t *d_ids = in, *d_pk = in + 32 * n_pad, *d_rs = in + 64 * n_pad, *d_esk = in + 96 * n_pad, *d_rcv = in + 128 * n_pad, *d_ovk = in + 160 * n_pad,
            *d_rnd = in + 192 * n_pad, *d_val = in + 288 * n_pad, *d_div = in + 296 * n_pad, *d_lead = in + 307 * n_pad, *d_flag = in + 308 * n_pad;
    uint8_t* out = w.ob_out.p;
    uint8_t *d_cv = out, *d_cmu = out + 32 * n_pad, *d_epk = out + 64 * n_pad, *d_enc = out + 96 * n_pad, *d_cout = out + 708 * n_pad, *d_status = out + 788 * n_pad;
    ObArgs a;
    a.in = {(const uint32_t*)d_ids, (const uint64_t*)d_val, d_div, (const uint32_t*)d_pk, d_lead, (const uint32_t*)d_rs,
            h.esks ? (const uint32_t*)d_esk : nullptr, (const uint32_t*)d_rcv, (const uint32_t*)d_ovk, h.flags ? d_flag : nullptr,
            h.randoms ? (const uint32_t*)d_rnd : nullptr};
    a.state = (ObState*)w.ob_state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.ncr = (const JNiels*)w.nf_table.p;
    a.vcr = (const JNiels*)w.ob_table.p;
    a.memo_rows = h.memos ? (const uint4*)w.ob_memo.p : nullptr;
    a.memo_cols = h.memos ? (uint4*)(w.ob_memo.p + 512 * n_pad) : nullptr;
    a.cols = (uint4*)w.ob_cols.p;
    a.status = d_status;
    a.cvs = (uint32_t*)d_cv;
    a.cmus = (uint32_t*)d_cmu;
    a.epks = (uint32_t*)d_epk;
    a.encs = (uint32_t*)d_enc;
    a.couts = (uint32_t*)d_cout;
    a.n_pad = (uint32_t)n_pad;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    for (size_t o = 0; o < n; o += cap) {
        const size_t c = std::min(cap, n - o);
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(hipMemcpyAsync(d_ids, h.ids + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pk, h.pk_ds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rs, h.rseeds + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        if (h.esks) HIP_TRY(hipMemcpyAsync(d_esk, h.esks + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rcv, h.rcvs + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ovk, h.ovks + 32 * o, 32 * c, hipMemcpyHostToDevice, s));
        if (h.randoms) HIP_TRY(hipMemcpyAsync(d_rnd, h.randoms + 96 * o, 96 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_val, h.values + o, 8 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_div, h.divs + 11 * o, 11 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_lead, h.leads + o, c, hipMemcpyHostToDevice, s));
        if (h.flags) HIP_TRY(hipMemcpyAsync(d_flag, h.flags + o, c, hipMemcpyHostToDevice, s));
        if (h.memos) HIP_TRY(hipMemcpyAsync(w.ob_memo.p, h.memos + 512 * o, 512 * c, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(out, 0, 788 * n_pad, s));   // a refused output's outputs are zeros
        HIP_TRY(hipEventRecord(ev[1], s));
        a.n = (uint32_t)c;
        ob_enqueue(s, a);
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipMemcpyAsync(h.status + o, d_status, c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.cvs + 32 * o, d_cv, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.cmus + 32 * o, d_cmu, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.epks + 32 * o, d_epk, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.encs + 612 * o, d_enc, 612 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.couts + 80 * o, d_cout, 80 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev[3], s));
        HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        if ((rc = add_elapsed(ev, 3, ms))) return rc;
    }
    w.ob_timing.store(ms);
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_build_outputs(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                   const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                   const uint8_t* esks, const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* ovk_flags,
                                   const uint8_t* out_randoms, uint8_t* status, uint8_t* cvs_out, uint8_t* cmus_out, uint8_t* epks_out,
                                   uint8_t* encs_out, uint8_t* couts_out) {
    if (!ctx || n > OB_MAX_OUTPUTS) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) return MASP_HIP_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !rcvs || !ovks || !status || !cvs_out || !cmus_out ||
        !epks_out || !encs_out || !couts_out)
        return MASP_HIP_E_INVALID_ARG;
    if (!esks && memchr(lead_bytes, 1, n)) return MASP_HIP_E_INVALID_ARG;              // a lead byte 1 needs its esk
    if (!out_randoms && ovk_flags && memchr(ovk_flags, 0, n)) return MASP_HIP_E_INVALID_ARG;   // an absent ovk needs its 96 bytes
    (void)pedersen_table_bytes();   // built outside the locks
    (void)nullifier_table();
    (void)output_table();
    WalletCall call(ctx);
    const ObHost h = {asset_identifiers, diversifiers, pk_ds,  lead_bytes, rseeds,   esks,     rcvs,     memos,    ovks,
                      ovk_flags,         out_randoms,  values, status,     cvs_out,  cmus_out, epks_out, encs_out, couts_out};
    const int rc = run_build_outputs(call.ctx, n, h);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[0]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_build_outputs_configure(masp_hip_ctx* ctx, size_t chunk_outputs) {
    if (!ctx || chunk_outputs > OB_CHUNK) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.ob_chunk.store(chunk_outputs);
    return MASP_HIP_OK;
}

int masp_hip_build_outputs_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.ob_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
#endif   // MASP_OB_KERNELS_ONLY
