// Test-only shim over the allowed conversions' device code: masp_amd/csrc/device/conversion.hpp on the host (the header is __host__
// __device__), step by step with the points handed out, and the product's own kernels (masp_amd/csrc/k_conversion.hip, its kernel half) on
// the GPU for either number of lanes per conversion, without a context.  The table is the product's (pedersen_table.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_CV_KERNELS_ONLY
#include "../../masp_amd/csrc/k_conversion.hip"
#include "../../masp_amd/csrc/pedersen_table.h"

using namespace masp;

namespace {

struct DevMem {
    std::vector<void*> all;
    ~DevMem() {
        for (void* p : all) (void)hipFree(p);
    }
    template <class T>
    T* put(const void* src, size_t bytes, bool& ok) {
        void* p = nullptr;
        ok = ok && hipMalloc(&p, bytes ? bytes : 1) == hipSuccess;
        if (ok) all.push_back(p);
        if (ok && src && bytes) ok = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && !src) ok = hipMemset(p, 0, bytes ? bytes : 1) == hipSuccess;
        return (T*)p;
    }
};

// offsets[0] = 0, non-decreasing, offsets[n_conv] = n_terms: what the product's entry point checks before its kernels run
bool offsets_ok(uint32_t n_conv, const uint64_t* off, uint32_t n_terms) {
    if (off[0] != 0 || off[n_conv] != n_terms) return false;
    for (uint32_t c = 0; c < n_conv; ++c)
        if (off[c] > off[c + 1]) return false;
    return true;
}

}  // namespace

extern "C" {

// the steps of device/conversion.hpp over n_conv conversions with `lanes` lanes per conversion, the lanes' masks OR-ed and their partial
// sums folded one after the other.  trace (may be NULL), 64 bytes a conversion: repr(generator point) 32 | repr(cm) 32 (zeros for a
// conversion with a status)
int cvd_steps_host(uint32_t n_conv, const uint64_t* offsets, uint32_t n_terms, const uint8_t* ids, const uint8_t* values, uint32_t lanes,
                   uint8_t* status, uint8_t* gens, uint8_t* cmus, uint8_t* trace) {
    if (lanes == 0 || lanes > 10 || !offsets_ok(n_conv, offsets, n_terms)) return -1;
    std::vector<uint32_t> idw(8 * (size_t)n_terms + 1), vw(4 * (size_t)n_terms + 1);
    if (n_terms) {
        memcpy(idw.data(), ids, 32 * (size_t)n_terms);
        memcpy(vw.data(), values, 16 * (size_t)n_terms);
    }
    const JNiels* ped = (const JNiels*)pedersen_table_bytes().data();
    std::vector<JExt> points(n_terms + 1);
    std::vector<uint8_t> term_status(n_terms + 1);
    for (uint32_t t = 0; t < n_terms; ++t) term_status[t] = cv_term(points[t], idw.data() + 8 * (size_t)t, vw.data() + 4 * (size_t)t);
    memset(gens, 0, 32 * (size_t)n_conv);
    memset(cmus, 0, 32 * (size_t)n_conv);
    if (trace) memset(trace, 0, 64 * (size_t)n_conv);
    for (uint32_t c = 0; c < n_conv; ++c) {
        const uint64_t begin = offsets[c], end = offsets[c + 1];
        uint32_t mask = 0;
        for (uint32_t l = 0; l < lanes; ++l) mask |= cv_status_partial(term_status.data(), begin, end, l, lanes);
        status[c] = cv_status_of(mask);
        if (status[c] != CV_OK) continue;
        JExt gen = cv_sum_partial(points.data(), begin, end, 0, lanes);
        for (uint32_t l = 1; l < lanes; ++l) gen = jj_add(gen, cv_sum_partial(points.data(), begin, end, l, lanes));
        uint32_t w[8], u[8];
        jj_encode(w, gen);
        memcpy(gens + 32 * (size_t)c, w, 32);
        JExt cm = cv_hash_partial(w, ped, 0, lanes);
        for (uint32_t l = 1; l < lanes; ++l) cm = jj_add(cm, cv_hash_partial(w, ped, l, lanes));
        cv_cmu(u, cm);
        memcpy(cmus + 32 * (size_t)c, u, 32);
        if (trace) {
            memcpy(trace + 64 * (size_t)c, w, 32);
            jj_encode(w, cm);
            memcpy(trace + 64 * (size_t)c + 32, w, 32);
        }
    }
    return 0;
}

// the product's three kernels over n_conv >= 1 conversions with lanes = 1 or 8 per conversion, on the null stream
int cvd_run_gpu(uint32_t n_conv, const uint64_t* offsets, uint32_t n_terms, const uint8_t* ids, const uint8_t* values, int lanes,
                uint8_t* status, uint8_t* gens, uint8_t* cmus) {
    if (n_conv == 0 || (lanes != 1 && lanes != 8) || !offsets_ok(n_conv, offsets, n_terms)) return -1;
    const std::vector<uint8_t>& ped = pedersen_table_bytes();
    DevMem m;
    bool ok = true;
    CvArgs a;
    a.ids = m.put<uint32_t>(ids, 32 * (size_t)n_terms, ok);
    a.values = m.put<uint32_t>(values, 16 * (size_t)n_terms, ok);
    a.offsets = m.put<uint64_t>(offsets, 8 * ((size_t)n_conv + 1), ok);
    a.points = m.put<JExt>(nullptr, sizeof(JExt) * (size_t)n_terms, ok);
    a.term_status = m.put<uint8_t>(nullptr, n_terms, ok);
    a.ped = m.put<JNiels>(ped.data(), ped.size(), ok);
    a.status = m.put<uint8_t>(nullptr, n_conv, ok);
    a.gens = m.put<uint32_t>(nullptr, 32 * (size_t)n_conv, ok);
    a.cmus = m.put<uint32_t>(nullptr, 32 * (size_t)n_conv, ok);
    a.n_conv = n_conv;
    a.n_terms = n_terms;
    if (!ok) return -2;
    launch_error().clear();
    cv_enqueue(nullptr, a, lanes);
    if (!launch_error().empty() || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(status, a.status, n_conv, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gens, a.gens, 32 * (size_t)n_conv, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cmus, a.cmus, 32 * (size_t)n_conv, hipMemcpyDeviceToHost) != hipSuccess)
        return -4;
    return 0;
}

}  // extern "C"
