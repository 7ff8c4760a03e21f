// Test-only shim over the note nullifiers' device code: masp_amd/csrc/device/nullifier.hpp on the host (the header is __host__ __device__),
// step by step with the state handed out, and the product's own kernels (masp_amd/csrc/k_nullifier.hip, its kernel half) on the GPU for
// either number of lanes per note, without a context.  The tables are the product's (nullifier_table.h, pedersen_table.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_NF_KERNELS_ONLY
#include "../../masp_amd/csrc/k_nullifier.hip"
#include "../../masp_amd/csrc/nullifier_table.h"

using namespace masp;

namespace {

// the eight arrays as they come, copied where the device code reads words
struct Inputs {
    std::vector<uint32_t> ids, pk_ds, rseeds, nks;
    std::vector<uint64_t> values, positions;
    const uint8_t *divs, *leads;
    Inputs(size_t n, const uint8_t* ids_, const uint64_t* values_, const uint8_t* divs_, const uint8_t* pk_ds_, const uint8_t* leads_,
           const uint8_t* rseeds_, const uint8_t* nks_, const uint64_t* positions_)
        : ids(8 * n), pk_ds(8 * n), rseeds(8 * n), nks(8 * n), values(n), positions(n), divs(divs_), leads(leads_) {
        memcpy(ids.data(), ids_, 32 * n);
        memcpy(pk_ds.data(), pk_ds_, 32 * n);
        memcpy(rseeds.data(), rseeds_, 32 * n);
        memcpy(nks.data(), nks_, 32 * n);
        memcpy(values.data(), values_, 8 * n);
        memcpy(positions.data(), positions_, 8 * n);
    }
    NfIn in() const { return {ids.data(), values.data(), divs, pk_ds.data(), leads, rseeds.data(), nks.data(), positions.data()}; }
};

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
        if (ok && src) ok = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && !src) ok = hipMemset(p, 0, bytes ? bytes : 1) == hipSuccess;
        return (T*)p;
    }
};

}  // namespace

extern "C" {

// [k] G from the fixed-base table: which = 0 G_ncr (63 windows: k below 2^252), 1 G_nf (16 windows: k below 2^64) -> the point's encoding
int nfd_table_mul_host(int which, const uint8_t k32[32], uint8_t out32[32]) {
    uint32_t k[8], w[8];
    memcpy(k, k32, 32);
    const JNiels* t = nullifier_table().data();
    const JExt p = which == 0 ? nf_table_sum(jj_identity(), t, NF_NCR_WINDOWS, k, 0, 1) : nf_table_sum(jj_identity(), t + NF_NCR_TABLE, NF_POS_WINDOWS, k, 0, 1);
    jj_encode(w, p);
    memcpy(out32, w, 32);
    return 0;
}

// the steps of device/nullifier.hpp over n notes with `lanes` lanes per note, the partial sums folded one after the other.
// trace (may be NULL), 208 bytes a note: msg 104 | rcm 32 | repr(cm) 32 | repr(rho) 32 | bad 8 (what the steps left in the state; cm and
// rho of a note with a status are zeros)
int nfd_steps_host(uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds, const uint8_t* leads,
                   const uint8_t* rseeds, const uint8_t* nks, const uint64_t* positions, uint32_t lanes, uint8_t* status, uint8_t* cmus,
                   uint8_t* nfs, uint8_t* trace) {
    if (lanes == 0 || lanes > 64) return -1;
    const Inputs I(n, ids, values, divs, pk_ds, leads, rseeds, nks, positions);
    const NfIn in = I.in();
    const JNiels* ped = (const JNiels*)pedersen_table_bytes().data();
    const JNiels* tab = nullifier_table().data();
    std::vector<NfState> state(n);
    memset((void*)state.data(), 0, sizeof(NfState) * n);
    memset(cmus, 0, 32 * (size_t)n);
    memset(nfs, 0, 32 * (size_t)n);
    if (trace) memset(trace, 0, 208 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        NfState& st = state[i];
        nf_parse(st, in, i, 0);
        nf_parse(st, in, i, 1);
        nf_key(st, in, i, 0);
        nf_key(st, in, i, 1);
        status[i] = nf_status(st);
        uint8_t* tr = trace ? trace + 208 * (size_t)i : nullptr;
        if (tr) {
            memcpy(tr, st.msg, 104);
            memcpy(tr + 104, st.rcm, 32);
            memcpy(tr + 200, st.bad, 8);
        }
        if (status[i] != NF_OK) continue;
        JExt cm = nf_commit_partial(st, ped, tab, 0, lanes);
        for (uint32_t l = 1; l < lanes; ++l) cm = jj_add(cm, nf_commit_partial(st, ped, tab, l, lanes));
        uint32_t w[8];
        nf_commit_finish(st, cm, w);
        memcpy(cmus + 32 * (size_t)i, w, 32);
        JExt rho = nf_rho_partial(st, tab + NF_NCR_TABLE, in.positions[i], 0, lanes);
        for (uint32_t l = 1; l < lanes; ++l) rho = jj_add(rho, nf_rho_partial(st, tab + NF_NCR_TABLE, in.positions[i], l, lanes));
        nf_finish(w, rho, in.nks + 8 * (size_t)i);
        memcpy(nfs + 32 * (size_t)i, w, 32);
        if (tr) {
            jj_encode(w, st.cm);
            memcpy(tr + 136, w, 32);
            jj_encode(w, rho);
            memcpy(tr + 168, w, 32);
        }
    }
    return 0;
}

// the product's four kernels over n >= 1 notes with lanes = 1 or 8 per note, on the null stream
int nfd_run_gpu(uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds, const uint8_t* leads,
                const uint8_t* rseeds, const uint8_t* nks, const uint64_t* positions, int lanes, uint8_t* status, uint8_t* cmus, uint8_t* nfs) {
    if (n == 0 || (lanes != 1 && lanes != 8)) return -1;
    const std::vector<uint8_t>& ped = pedersen_table_bytes();
    const std::vector<JNiels>& tab = nullifier_table();
    DevMem m;
    bool ok = true;
    NfArgs a;
    a.in.ids = m.put<uint32_t>(ids, 32 * (size_t)n, ok);
    a.in.values = m.put<uint64_t>(values, 8 * (size_t)n, ok);
    a.in.diversifiers = m.put<uint8_t>(divs, 11 * (size_t)n, ok);
    a.in.pk_ds = m.put<uint32_t>(pk_ds, 32 * (size_t)n, ok);
    a.in.leads = m.put<uint8_t>(leads, n, ok);
    a.in.rseeds = m.put<uint32_t>(rseeds, 32 * (size_t)n, ok);
    a.in.nks = m.put<uint32_t>(nks, 32 * (size_t)n, ok);
    a.in.positions = m.put<uint64_t>(positions, 8 * (size_t)n, ok);
    a.state = m.put<NfState>(nullptr, sizeof(NfState) * (size_t)n, ok);
    a.ped = m.put<JNiels>(ped.data(), ped.size(), ok);
    a.tab = m.put<JNiels>(tab.data(), sizeof(JNiels) * tab.size(), ok);
    a.status = m.put<uint8_t>(nullptr, n, ok);
    a.cmus = m.put<uint32_t>(nullptr, 32 * (size_t)n, ok);
    a.nfs = m.put<uint32_t>(nullptr, 32 * (size_t)n, ok);
    a.n = n;
    if (!ok) return -2;
    launch_error().clear();
    nf_enqueue(nullptr, a, lanes);
    if (!launch_error().empty() || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(status, a.status, n, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(cmus, a.cmus, 32 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(nfs, a.nfs, 32 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return -4;
    return 0;
}

}  // extern "C"
