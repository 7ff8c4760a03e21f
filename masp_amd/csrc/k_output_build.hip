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
#include "column_host.h"
#include "output_table.h"

using namespace masp;

namespace {

constexpr size_t OB_MAX_OUTPUTS = (size_t)1 << 20;
// outputs per launch sequence: 309 bytes in, 512 of memo twice, 592 of state, 704 of columns and 789 out an output, 225 MB in all
constexpr size_t OB_CHUNK = (size_t)1 << 16;
// ids, pk_ds, rseeds, esks, rcvs, ovks, out_randoms, values, diversifiers, lead bytes, ovk flags
constexpr ColumnWidths OB_IN{32, 32, 32, 32, 32, 32, 96, 8, 11, 1, 1};
constexpr ColumnWidths OB_OUT{32, 32, 32, 4 * OB_ENC_WORDS, 4 * OB_OUT_WORDS, 1};   // cvs, cmus, epks, enc_ciphertexts, out_ciphertexts, status
constexpr size_t OB_MEMO = 16 * OB_MEMO_COLS;
static_assert(OB_IN.total == 309 && OB_MEMO == 512 && sizeof(ObState) == 592 && 16 * OB_COLS == 704 && OB_OUT.total == 789, "OB_CHUNK's sizing");

struct ObHost {
    const uint8_t *ids, *divs, *pk_ds, *leads, *rseeds, *esks, *rcvs, *memos, *ovks, *flags, *randoms;
    const uint64_t* values;
    uint8_t *status, *cvs, *cmus, *epks, *encs, *couts;
};

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall and ends it (end_per_item)
int run_build_outputs(masp_hip_ctx* ctx, size_t n, const ObHost& h) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    ColumnCall cc(OB_IN, OB_OUT, column_chunk(w.ob.chunk.load(), OB_CHUNK, n));
    int rc;
    if ((rc = w.ob.reserve(cc, sizeof(ObState))) || (rc = w.ob_cols.reserve(16 * (size_t)OB_COLS * cc.n_pad)) ||
        (h.memos && (rc = w.ob_memo.reserve(2 * OB_MEMO * cc.n_pad))) || (rc = pedersen_table_ensure(w, s)) || (rc = nullifier_table_ensure(w, s)) ||
        (rc = output_table_ensure(w, s)))
        return rc;
    ObArgs a;   // (the columns in OB_IN's and OB_OUT's order; the memo rows go up behind them into a buffer of their own)
    a.in.ids = cc.in<uint32_t>(h.ids), a.in.pk_ds = cc.in<uint32_t>(h.pk_ds), a.in.rseeds = cc.in<uint32_t>(h.rseeds);
    a.in.esks = cc.in<uint32_t>(h.esks), a.in.rcvs = cc.in<uint32_t>(h.rcvs), a.in.ovks = cc.in<uint32_t>(h.ovks);
    a.in.out_randoms = cc.in<uint32_t>(h.randoms), a.in.values = cc.in<uint64_t>(h.values), a.in.diversifiers = cc.in(h.divs);
    a.in.leads = cc.in(h.leads), a.in.ovk_flags = cc.in(h.flags);
    a.memo_rows = cc.in_at<uint4>(w.ob_memo.p, OB_MEMO, h.memos);
    a.memo_cols = h.memos ? (uint4*)(w.ob_memo.p + OB_MEMO * cc.n_pad) : nullptr;
    a.state = (ObState*)w.ob.state.p;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.ncr = (const JNiels*)w.nf_table.p;
    a.vcr = (const JNiels*)w.ob_table.p;
    a.cols = (uint4*)w.ob_cols.p;
    a.cvs = cc.out<uint32_t>(h.cvs), a.cmus = cc.out<uint32_t>(h.cmus), a.epks = cc.out<uint32_t>(h.epks);
    a.encs = cc.out<uint32_t>(h.encs), a.couts = cc.out<uint32_t>(h.couts), a.status = cc.out(h.status);
    a.n_pad = (uint32_t)cc.n_pad;
    return run_per_item(s, w.ob, cc, n, [&](size_t c) { a.n = (uint32_t)c, ob_enqueue(s, a); });
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
    return call.done(end_per_item(call.ctx->streams.vk[0], call.w.ob, OB_IN, run_build_outputs(call.ctx, n, h)));
}

int masp_hip_build_outputs_configure(masp_hip_ctx* ctx, size_t chunk_outputs) { return per_item_configure(ctx, &WalletState::ob, chunk_outputs, OB_CHUNK); }

int masp_hip_build_outputs_last_timing(masp_hip_ctx* ctx, double ms[3]) { return per_item_last_timing(ctx, &WalletState::ob, ms); }

}  // extern "C"
#endif   // MASP_OB_KERNELS_ONLY
