// The consensus pre-checks of a block's bundles on the GPU: the C ABI entry point masp_hip_sapling_check_bundles (include/masp_hip.h), what
// BatchValidator::check_bundle (masp_proofs/src/sapling/verifier/batch.rs:78-193) decides per description before it queues anything, with the
// public inputs (verifier.rs:71-95, 120-128, 151-165) and the binding verification key (sapling/mod.rs:14-38) that validation then needs, for
// every bundle of a block in one call.  The per-item steps are device/bundle_check.hpp; the kernels are wrappers around them:
//           k_bc_points      one lane per Jubjub encoding (cv, rk, epk): decoding, the small-order test, the canonical (u, v);
//           k_bc_terms       one lane per value-balance entry: -sign(value) [|value|] [8] asset_generator(identifier);
//           k_bc_proof_read  gridDim.y = 3, one lane per proof point: `Proof::read` of A, B, C with the subgroup tests, a status byte each
//                            (the readers and tests of the Groth16 verifier, device/point_read.hpp and subgroup.hpp; nothing else is kept);
//           k_bc_rows        one lane per description: its status byte and its public-input row;
//           k_bc_bvk         one lane per bundle: the sum of its cv and terms, encoded, and the bundle's status.
// A wave per workgroup throughout: a block of a few thousand descriptions is a few hundred waves on 1 024 SIMDs.
#include "device/bundle_check.hpp"
#include "device/point_read.hpp"
#include "device/subgroup.hpp"
#include "util.h"

namespace masp {

constexpr uint32_t BC_BLOCK = 64;

__global__ __launch_bounds__(BC_BLOCK) void k_bc_points(const BcArgs a) {
    const uint32_t i = blockIdx.x * BC_BLOCK + threadIdx.x;
    if (i >= bc_n_points(a)) return;
    bc_point_lane(a, i);
}

__global__ __launch_bounds__(BC_BLOCK) void k_bc_terms(const BcArgs a) {
    const uint32_t i = blockIdx.x * BC_BLOCK + threadIdx.x;
    if (i >= a.n_balance) return;
    bc_term_lane(a, i);
}

// proofs: n x 192 bytes; status3[3 i + y]: 0, or the PT_* bits for which `Proof::read` refuses point y of proof i (y = 0 A, 1 B, 2 C; the
// identity is refused too).  Every lane writes a byte of its own.
__global__ __launch_bounds__(BC_BLOCK) void k_bc_proof_read(const uint8_t* __restrict__ proofs, uint32_t n, uint8_t* __restrict__ status3) {
    const uint32_t i = blockIdx.x * BC_BLOCK + threadIdx.x, what = blockIdx.y;
    if (i >= n) return;
    const uint8_t* pr = proofs + 192 * (size_t)i;
    int st;
    if (what == 1) {
        G2Affine q;
        st = g2_read_compressed(pr + 48, q);
        if (st == PT_OK && !g2_in_subgroup(q)) st = PT_NOT_IN_SUBGROUP;
    } else {
        G1Affine p;
        st = g1_read_compressed(pr + (what == 0 ? 0 : 144), p);
        if (st == PT_OK && !g1_in_subgroup(p)) st = PT_NOT_IN_SUBGROUP;
    }
    status3[3 * (size_t)i + what] = (uint8_t)st;
}

__global__ __launch_bounds__(BC_BLOCK) void k_bc_rows(const BcArgs a) {
    const uint32_t i = blockIdx.x * BC_BLOCK + threadIdx.x;
    if (i >= bc_n_descriptions(a)) return;
    bc_row_lane(a, i);
}

__global__ __launch_bounds__(BC_BLOCK) void k_bc_bvk(const BcArgs a) {
    const uint32_t i = blockIdx.x * BC_BLOCK + threadIdx.x;
    if (i >= a.n_bundles) return;
    bc_bvk_lane(a, i);
}

}  // namespace masp

#include <mutex>

#include "internal.h"

using namespace masp;

namespace {

constexpr size_t BC_MAX_ITEMS = (size_t)1 << 20;     // per kind: spends, converts, outputs, value-balance entries
constexpr size_t BC_MAX_BUNDLES = (size_t)1 << 22;
constexpr size_t BC_PROOF_CHUNK = (size_t)1 << 16;   // proofs per upload and launch, as masp_hip_verify_each: 12 MB of proof bytes at a time

inline dim3 bc_grid(size_t n, uint32_t y = 1) { return dim3((uint32_t)((n + BC_BLOCK - 1) / BC_BLOCK), y); }

// Everything of one call on the context's second verifier stream.  offsets: (n_bundles + 1) x 4.  Caller: ctx->mu shared, ctx->jj.mu held.
int run_check_bundles(masp_hip_ctx* ctx, const masp_hip_bundle_check& h, const std::vector<uint32_t>& offsets) {
    JubjubState& jj = ctx->jj;
    hipStream_t s = ctx->streams.vk[1];
    const size_t S = h.n_spends, C = h.n_converts, O = h.n_outputs, B = h.n_balance, N = h.n_bundles;
    const size_t P = 2 * S + C + 2 * O, D = S + C + O;
    // in: the encodings kind after kind, then the other arrays (every one starts on a multiple of 16 bytes)
    const size_t in_enc = 0, in_sa = in_enc + 32 * P, in_nf = in_sa + 32 * S, in_ca = in_nf + 32 * S, in_cmu = in_ca + 32 * C, in_asset = in_cmu + 32 * O,
                 in_value = in_asset + 32 * B, in_off = in_value + 16 * B, in_bytes = in_off + 16 * (N + 1);
    // between the kernels: words first, bytes behind
    const size_t w_uv = 0, w_term = w_uv + 64 * P, w_ps = w_term + sizeof(JExt) * B, w_pts = w_ps + 3 * D, w_ts = w_pts + P, w_bytes = w_ts + B;
    // out: rows and bvk (words), then the status bytes
    const size_t o_si = 0, o_ci = o_si + 32 * BC_SPEND_INPUTS * S, o_oi = o_ci + 32 * BC_CONVERT_INPUTS * C, o_bvk = o_oi + 32 * BC_OUTPUT_INPUTS * O,
                 o_st = o_bvk + 32 * N, o_bst = o_st + D, o_bytes = o_bst + N;
    int rc;
    if ((rc = jj.bc_in.reserve(in_bytes)) || (rc = jj.bc_work.reserve(w_bytes)) || (rc = jj.bc_out.reserve(o_bytes)) ||
        (rc = jj.bc_proofs.reserve(192 * std::min(BC_PROOF_CHUNK, std::max(std::max(S, C), O)))))
        return rc;
    uint8_t *in = jj.bc_in.p, *work = jj.bc_work.p, *out = jj.bc_out.p;
    BcArgs a;
    a.enc = (const uint32_t*)(in + in_enc);
    a.spend_anchor = (const uint32_t*)(in + in_sa);
    a.spend_nf = (const uint32_t*)(in + in_nf);
    a.convert_anchor = (const uint32_t*)(in + in_ca);
    a.output_cmu = (const uint32_t*)(in + in_cmu);
    a.asset = (const uint32_t*)(in + in_asset);
    a.value = (const uint32_t*)(in + in_value);
    a.offsets = (const uint32_t*)(in + in_off);
    a.proof_status = work + w_ps;
    a.pt_status = work + w_pts;
    a.pt_uv = (uint32_t*)(work + w_uv);
    a.term = (JExt*)(work + w_term);
    a.term_status = work + w_ts;
    a.status = out + o_st;
    a.spend_inputs = (uint32_t*)(out + o_si);
    a.convert_inputs = (uint32_t*)(out + o_ci);
    a.output_inputs = (uint32_t*)(out + o_oi);
    a.bvk = (uint32_t*)(out + o_bvk);
    a.bundle_status = out + o_bst;
    a.n_spends = (uint32_t)S;
    a.n_converts = (uint32_t)C;
    a.n_outputs = (uint32_t)O;
    a.n_balance = (uint32_t)B;
    a.n_bundles = (uint32_t)N;
    Event ev[6];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    auto put = [&](size_t at, const void* src, size_t bytes) {
        return bytes ? HIP_RC(hipMemcpyAsync(in + at, src, bytes, hipMemcpyHostToDevice, s)) : MASP_HIP_OK;
    };
    auto get = [&](void* dst, size_t at, size_t bytes) {
        return bytes ? HIP_RC(hipMemcpyAsync(dst, out + at, bytes, hipMemcpyDeviceToHost, s)) : MASP_HIP_OK;
    };
    HIP_TRY(hipEventRecord(ev[0], s));
    if ((rc = put(in_enc, h.spend_cv, 32 * S)) || (rc = put(in_enc + 32 * S, h.spend_rk, 32 * S)) || (rc = put(in_enc + 64 * S, h.convert_cv, 32 * C)) ||
        (rc = put(in_enc + 64 * S + 32 * C, h.output_cv, 32 * O)) || (rc = put(in_enc + 64 * S + 32 * C + 32 * O, h.output_epk, 32 * O)) ||
        (rc = put(in_sa, h.spend_anchor, 32 * S)) || (rc = put(in_nf, h.spend_nullifier, 32 * S)) || (rc = put(in_ca, h.convert_anchor, 32 * C)) ||
        (rc = put(in_cmu, h.output_cmu, 32 * O)) || (rc = put(in_asset, h.balance_asset, 32 * B)) || (rc = put(in_value, h.balance_value, 16 * B)) ||
        (rc = put(in_off, offsets.data(), 16 * (N + 1))))
        return rc;
    HIP_TRY(hipEventRecord(ev[1], s));
    if (P) MASP_LAUNCH(k_bc_points, bc_grid(P), dim3(BC_BLOCK), 0, s, a);
    if (B) MASP_LAUNCH(k_bc_terms, bc_grid(B), dim3(BC_BLOCK), 0, s, a);
    HIP_TRY(hipEventRecord(ev[2], s));
    bool first_part_timed = false;
    const uint8_t* proofs[3] = {h.spend_zkproof, h.convert_zkproof, h.output_zkproof};
    const size_t n_proofs[3] = {S, C, O}, base[3] = {0, S, S + C};
    for (int kind = 0; kind < 3; ++kind)
        for (size_t lo = 0; lo < n_proofs[kind]; lo += BC_PROOF_CHUNK) {
            const size_t m = std::min(BC_PROOF_CHUNK, n_proofs[kind] - lo);
            HIP_TRY(hipEventRecord(ev[3], s));
            HIP_TRY(hipMemcpyAsync(jj.bc_proofs.p, proofs[kind] + 192 * lo, 192 * m, hipMemcpyHostToDevice, s));
            HIP_TRY(hipEventRecord(ev[4], s));
            MASP_LAUNCH(k_bc_proof_read, bc_grid(m, 3), dim3(BC_BLOCK), 0, s, (const uint8_t*)jj.bc_proofs.p, (uint32_t)m, work + w_ps + 3 * (base[kind] + lo));
            HIP_TRY(hipEventRecord(ev[5], s));
            HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the proof bytes and records these events again
            if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;
            if (!first_part_timed && (rc = add_elapsed(ev, 2, ms))) return rc;
            first_part_timed = true;
            if ((rc = add_elapsed(ev + 3, 2, ms))) return rc;
        }
    HIP_TRY(hipEventRecord(ev[3], s));
    if (D) MASP_LAUNCH(k_bc_rows, bc_grid(D), dim3(BC_BLOCK), 0, s, a);
    MASP_LAUNCH(k_bc_bvk, bc_grid(N), dim3(BC_BLOCK), 0, s, a);
    HIP_TRY(hipEventRecord(ev[4], s));
    if ((rc = get(h.spend_status, o_st, S)) || (rc = get(h.convert_status, o_st + S, C)) || (rc = get(h.output_status, o_st + S + C, O)) ||
        (rc = get(h.spend_inputs, o_si, 32 * BC_SPEND_INPUTS * S)) || (rc = get(h.convert_inputs, o_ci, 32 * BC_CONVERT_INPUTS * C)) ||
        (rc = get(h.output_inputs, o_oi, 32 * BC_OUTPUT_INPUTS * O)) || (rc = get(h.bvk, o_bvk, 32 * N)) || (rc = get(h.bundle_status, o_bst, N)))
        return rc;
    HIP_TRY(hipEventRecord(ev[5], s));
    HIP_TRY(hipStreamSynchronize(s));
    if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the bytes read back mean nothing
    if (!first_part_timed && (rc = add_elapsed(ev, 2, ms))) return rc;
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, ev[3], ev[4]));
    ms[1] += t;
    HIP_TRY(hipEventElapsedTime(&t, ev[4], ev[5]));
    ms[2] += t;
    jj.bc_timing.store(ms);
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_check_bundles(masp_hip_ctx* ctx, const masp_hip_bundle_check* args) {
    if (!ctx || !args) return MASP_HIP_E_INVALID_ARG;
    const masp_hip_bundle_check& h = *args;
    if (h.n_bundles == 0) return MASP_HIP_OK;
    if (h.n_bundles > BC_MAX_BUNDLES || h.n_spends > BC_MAX_ITEMS || h.n_converts > BC_MAX_ITEMS || h.n_outputs > BC_MAX_ITEMS || h.n_balance > BC_MAX_ITEMS ||
        !h.counts || !h.bvk || !h.bundle_status)
        return MASP_HIP_E_INVALID_ARG;
    if ((h.n_spends && (!h.spend_cv || !h.spend_anchor || !h.spend_nullifier || !h.spend_rk || !h.spend_zkproof || !h.spend_status || !h.spend_inputs)) ||
        (h.n_converts && (!h.convert_cv || !h.convert_anchor || !h.convert_zkproof || !h.convert_status || !h.convert_inputs)) ||
        (h.n_outputs && (!h.output_cv || !h.output_cmu || !h.output_epk || !h.output_zkproof || !h.output_status || !h.output_inputs)) ||
        (h.n_balance && (!h.balance_asset || !h.balance_value)))
        return MASP_HIP_E_INVALID_ARG;
    // where each bundle's items start: the running sums of the counts' columns, which must end at the four totals
    std::vector<uint32_t> offsets(4 * (h.n_bundles + 1));
    uint64_t run[4] = {0, 0, 0, 0};
    for (size_t b = 0; b <= h.n_bundles; ++b)
        for (int k = 0; k < 4; ++k) {
            if (run[k] > BC_MAX_ITEMS) return MASP_HIP_E_INVALID_ARG;
            offsets[4 * b + k] = (uint32_t)run[k];
            if (b < h.n_bundles) run[k] += h.counts[4 * b + k];
        }
    if (run[0] != h.n_spends || run[1] != h.n_converts || run[2] != h.n_outputs || run[3] != h.n_balance) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::SHARED);   // concurrent with provers and verifiers
    std::lock_guard<std::mutex> jlock(call.ctx->jj.mu);
    const int rc = run_check_bundles(call.ctx, h, offsets);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[1]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_check_bundles_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->jj.bc_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
