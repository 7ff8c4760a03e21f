// A conversion tree's leaves on the GPU: the C ABI entry point masp_hip_sapling_allowed_conversions (include/masp_hip.h),
// AllowedConversion::from(I128Sum) and AllowedConversion::cmu of masp_primitives/src/convert.rs for many conversions at once.
// The steps themselves are device/conversion.hpp; the kernels are wrappers around them:
//           k_cv_terms     one lane per term: the asset generator (the family's one square root), the sign and the low 64 bits of |v|, the
//                          64-bit multiplication; the signed point and a status byte go to global memory;
//           k_cv_generator L lanes per conversion: the conversion's status from its terms' bytes, then the terms' points, a share per lane,
//                          folded over __shfl_xor; the group's first lane encodes the generator;
//           k_cv_leaf      L lanes per conversion: the 88 Pedersen summands over the generator's 256 bits, a share per lane, folded the same
//                          way; the first lane writes cmu.
// One inversion a kernel, as in the nullifiers' (with both in one kernel the compiler kept 384 bytes of scratch a lane instead of 256, and the
// group's lanes needed the first lane's eight words handed round; cut, they read them from global memory).  A refused conversion leaves
// k_cv_generator as a whole group and is skipped by k_cv_leaf; its outputs stay the zeros they were set to.  The term kernel does not
// depend on L.  There is no reduction across lane groups: one very long conversion is a serial loop of its L lanes.
#include "device/conversion.hpp"
#include "util.h"

namespace masp {

constexpr uint32_t CV_BLOCK = 64;   // a wave per workgroup, as the nullifiers': a few thousand conversions spread over the chip
// Below this many conversions a call runs the lane groups of eight.  Measured on an MI355X (tools/conversion_bench.py, conversions of three
// terms: profiles/conversion_bench.json, its four sizes and the sweep between 4 096 and 65 536), the three kernels' time with
// eight lanes against one: 1.26 / 1.53 ms at 256 conversions, 1.30 / 1.51 at 4 096, 1.42 / 1.49 at 8 192, 1.48 / 1.52 at 16 384, and then
// 2.35 / 2.07 at 32 768, 3.74 / 3.05 at 65 536 and 49.7 / 40.9 at 2^20: the crossover lies between 16 384 and 32 768, half the nullifiers'
// 65 536 (the chain here is 3 + 88 additions, not 343, and the term kernel does not depend on the width).
constexpr size_t CV_WIDE_BELOW = 32768;

struct CvArgs {
    const uint32_t* ids;        // 8 words a term
    const uint32_t* values;     // 4 words a term
    const uint64_t* offsets;    // n_conv + 1, as the caller's: the chunk's first term is offsets[0]
    JExt* points;               // a term's signed point
    uint8_t* term_status;
    const JNiels* ped;          // the Pedersen Niels table (pedersen_table.h)
    uint8_t* status;
    uint32_t* gens;             // 8 words a conversion
    uint32_t* cmus;             // 8 words a conversion
    uint32_t n_conv, n_terms;
};

__global__ __launch_bounds__(CV_BLOCK) void k_cv_terms(const CvArgs a) {
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x;
    if (t >= a.n_terms) return;
    JExt p;
    a.term_status[t] = cv_term(p, a.ids + 8 * (size_t)t, a.values + 4 * (size_t)t);
    a.points[t] = p;
}

// the sum of the L partial sums of a lane group (L a power of two, groups aligned in the wave), in every lane of the group
template <int L>
__device__ __forceinline__ JExt cv_fold(JExt r) {
    for (int m = 1; m < L; m <<= 1) {
        JExt o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o.U.v[k] = __shfl_xor(r.U.v[k], m);
            o.V.v[k] = __shfl_xor(r.V.v[k], m);
            o.Z.v[k] = __shfl_xor(r.Z.v[k], m);
            o.T.v[k] = __shfl_xor(r.T.v[k], m);
        }
        r = jj_add(r, o);
    }
    return r;
}

// (a lane group is wholly inside the conversions or wholly outside, and a conversion's status is the same for its lanes: the lanes that
// fold are all there)
template <int L>
__global__ __launch_bounds__(CV_BLOCK) void k_cv_generator(const CvArgs a) {
    static_assert(L == 1 || L == 8, "lanes per conversion");
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x, g = t / L, lane = t % L;
    if (g >= a.n_conv) return;
    const uint64_t base = a.offsets[0], begin = a.offsets[g] - base, end = a.offsets[g + 1] - base;
    uint32_t mask = cv_status_partial(a.term_status, begin, end, lane, L);
    for (int m = 1; m < L; m <<= 1) mask |= __shfl_xor(mask, m);
    const uint8_t status = cv_status_of(mask);
    if (lane == 0) a.status[g] = status;
    if (status != CV_OK) return;
    const JExt gen = cv_fold<L>(cv_sum_partial(a.points, begin, end, lane, L));
    if (lane != 0) return;
    uint32_t w[8];
    jj_encode(w, gen);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.gens[8 * (size_t)g + k] = w[k];
}

template <int L>
__global__ __launch_bounds__(CV_BLOCK) void k_cv_leaf(const CvArgs a) {
    static_assert(L == 1 || L == 8, "lanes per conversion");
    const uint32_t t = blockIdx.x * CV_BLOCK + threadIdx.x, g = t / L, lane = t % L;
    if (g >= a.n_conv || a.status[g] != CV_OK) return;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = a.gens[8 * (size_t)g + k];   // (the same eight words for the group's lanes: one request)
    const JExt cm = cv_fold<L>(cv_hash_partial(w, a.ped, lane, L));
    if (lane != 0) return;
    uint32_t cmu[8];
    cv_cmu(cmu, cm);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.cmus[8 * (size_t)g + k] = cmu[k];
}

// the three kernels over a.n_conv >= 1 conversions on `s`; lanes: 1 or 8
inline void cv_enqueue(hipStream_t s, const CvArgs& a, int lanes) {
    if (a.n_terms) MASP_LAUNCH(k_cv_terms, dim3((a.n_terms + CV_BLOCK - 1) / CV_BLOCK), dim3(CV_BLOCK), 0, s, a);
    if (lanes == 8) {
        const uint32_t nb8 = (uint32_t)(((uint64_t)a.n_conv * 8 + CV_BLOCK - 1) / CV_BLOCK);
        MASP_LAUNCH(k_cv_generator<8>, dim3(nb8), dim3(CV_BLOCK), 0, s, a);
        MASP_LAUNCH(k_cv_leaf<8>, dim3(nb8), dim3(CV_BLOCK), 0, s, a);
    } else {
        const uint32_t nb = (a.n_conv + CV_BLOCK - 1) / CV_BLOCK;
        MASP_LAUNCH(k_cv_generator<1>, dim3(nb), dim3(CV_BLOCK), 0, s, a);
        MASP_LAUNCH(k_cv_leaf<1>, dim3(nb), dim3(CV_BLOCK), 0, s, a);
    }
}

}  // namespace masp

#ifndef MASP_CV_KERNELS_ONLY   // (tests/native/conversion_dev.hip runs the kernels above for both lane widths without a context)
#include "internal.h"
#include "pedersen_table.h"

using namespace masp;

namespace {

constexpr size_t CV_MAX_CONV = (size_t)1 << 22, CV_MAX_TERMS = (size_t)1 << 24;
// conversions and terms per launch sequence: a term is 48 bytes in and 129 of point and status, a conversion 8 in and 65 out
constexpr size_t CV_CHUNK_CONV = (size_t)1 << 19, CV_CHUNK_TERMS = (size_t)1 << 20;

struct CvHost {
    const uint64_t* offsets;
    const uint8_t *ids, *values;
    uint8_t *status, *gens, *cmus;
};

// the chunks of a call, cut at conversion boundaries: chunk k holds the conversions cuts[k] .. cuts[k + 1] - 1, at most max_conv of
// them with at most max_terms terms together.  false: one conversion alone has more than max_terms terms.
bool cv_cut(std::vector<size_t>& cuts, size_t n_conv, const uint64_t* off, size_t max_conv, size_t max_terms) {
    cuts.assign(1, 0);
    for (size_t c = 0; c < n_conv; ++c) {
        if (off[c + 1] - off[c] > max_terms) return false;
        const size_t first = cuts.back();
        if (c - first == max_conv || off[c + 1] - off[first] > max_terms) cuts.push_back(c);
    }
    cuts.push_back(n_conv);
    return true;
}

// everything of one call on the context's first verifier stream, chunk after chunk; the caller is a WalletCall
int run_conversions(masp_hip_ctx* ctx, const std::vector<size_t>& cuts, const CvHost& h, int lanes) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    size_t cap_c = 0, cap_t = 0;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        cap_c = std::max(cap_c, cuts[k + 1] - cuts[k]);
        cap_t = std::max(cap_t, (size_t)(h.offsets[cuts[k + 1]] - h.offsets[cuts[k]]));
    }
    cap_c = (cap_c + 63) / 64 * 64;   // every array of a buffer starts on a multiple of 8 bytes
    cap_t = (cap_t + 63) / 64 * 64;
    int rc;
    if ((rc = w.cv_in.reserve(8 * (cap_c + 8) + 48 * cap_t)) || (rc = w.cv_terms.reserve(sizeof(JExt) * cap_t + cap_t)) ||
        (rc = w.cv_out.reserve(65 * cap_c)))
        return rc;
    if ((rc = pedersen_table_ensure(w, s))) return rc;
    uint8_t *d_off = w.cv_in.p, *d_ids = d_off + 8 * (cap_c + 8), *d_val = d_ids + 32 * cap_t;
    uint8_t *d_gen = w.cv_out.p, *d_cmu = d_gen + 32 * cap_c, *d_status = d_gen + 64 * cap_c;
    CvArgs a;
    a.ids = (const uint32_t*)d_ids;
    a.values = (const uint32_t*)d_val;
    a.offsets = (const uint64_t*)d_off;
    a.points = (JExt*)w.cv_terms.p;
    a.term_status = w.cv_terms.p + sizeof(JExt) * cap_t;
    a.ped = (const JNiels*)w.nsc_table.p;
    a.status = d_status;
    a.gens = (uint32_t*)d_gen;
    a.cmus = (uint32_t*)d_cmu;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    double ms[3] = {0, 0, 0};
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const size_t c0 = cuts[k], c = cuts[k + 1] - c0;
        const size_t t0 = (size_t)h.offsets[c0], t = (size_t)h.offsets[c0 + c] - t0;
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(hipMemcpyAsync(d_off, h.offsets + c0, 8 * (c + 1), hipMemcpyHostToDevice, s));
        if (t) {
            HIP_TRY(hipMemcpyAsync(d_ids, h.ids + 32 * t0, 32 * t, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_val, h.values + 16 * t0, 16 * t, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemsetAsync(d_gen, 0, 64 * cap_c, s));   // a refused conversion's outputs are zeros
        HIP_TRY(hipEventRecord(ev[1], s));
        a.n_conv = (uint32_t)c;
        a.n_terms = (uint32_t)t;
        cv_enqueue(s, a, lanes);
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipMemcpyAsync(h.status + c0, d_status, c, hipMemcpyDeviceToHost, s));
        if (h.gens) HIP_TRY(hipMemcpyAsync(h.gens + 32 * c0, d_gen, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.cmus + 32 * c0, d_cmu, 32 * c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev[3], s));
        HIP_TRY(hipStreamSynchronize(s));   // the next chunk overwrites the buffers
        if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
        if ((rc = add_elapsed(ev, 3, ms))) return rc;
    }
    w.cv_timing.store(ms);
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_sapling_allowed_conversions(masp_hip_ctx* ctx, size_t n_conv, const uint64_t* term_offsets, size_t n_terms,
                                         const uint8_t* identifiers, const uint8_t* values, uint8_t* status, uint8_t* generators_out,
                                         uint8_t* cmus_out) {
    if (!ctx || n_conv > CV_MAX_CONV || n_terms > CV_MAX_TERMS) return MASP_HIP_E_INVALID_ARG;
    if (n_conv == 0) return MASP_HIP_OK;
    if (!term_offsets || !status || !cmus_out || (n_terms && (!identifiers || !values))) return MASP_HIP_E_INVALID_ARG;
    if (term_offsets[0] != 0 || term_offsets[n_conv] != n_terms) return MASP_HIP_E_INVALID_ARG;
    for (size_t c = 0; c < n_conv; ++c)
        if (term_offsets[c] > term_offsets[c + 1]) return MASP_HIP_E_INVALID_ARG;
    WalletState& cfg = FIRST_DEVICE(ctx)->wallet;
    const size_t max_conv = cfg.cv_chunk_conv.load(), max_terms = cfg.cv_chunk_terms.load();
    std::vector<size_t> cuts;
    if (!cv_cut(cuts, n_conv, term_offsets, max_conv ? max_conv : CV_CHUNK_CONV, max_terms ? max_terms : CV_CHUNK_TERMS))
        return MASP_HIP_E_INVALID_ARG;
    const int forced = cfg.cv_lanes.load();
    const int lanes = forced ? forced : n_conv < CV_WIDE_BELOW ? 8 : 1;
    (void)pedersen_table_bytes();   // built outside the locks
    WalletCall call(ctx);
    const CvHost h = {term_offsets, identifiers, values, status, generators_out, cmus_out};
    const int rc = run_conversions(call.ctx, cuts, h, lanes);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[0]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_allowed_conversions_configure(masp_hip_ctx* ctx, int lanes_per_conversion, size_t chunk_conversions, size_t chunk_terms) {
    if (!ctx || (lanes_per_conversion != 0 && lanes_per_conversion != 1 && lanes_per_conversion != 8) || chunk_conversions > CV_CHUNK_CONV ||
        chunk_terms > CV_CHUNK_TERMS)
        return MASP_HIP_E_INVALID_ARG;
    WalletState& w = FIRST_DEVICE(ctx)->wallet;
    w.cv_lanes.store(lanes_per_conversion);
    w.cv_chunk_conv.store(chunk_conversions);
    w.cv_chunk_terms.store(chunk_terms);
    return MASP_HIP_OK;
}

int masp_hip_allowed_conversions_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.cv_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
#endif   // MASP_CV_KERNELS_ONLY
