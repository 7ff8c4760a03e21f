// Test-only unit over the kernels that write and read a CRS: the parameter-generation kernels of masp_amd/csrc/device/setup.hpp, the base
// import of the MSM tables (k_msm_import, device/msm.hpp) and the loader's single-point imports (k_g1_import_one / k_g2_import_one through
// their launch_* wrappers: the product's translation unit k_groth16.hip is included whole).  Every entry point below launches ONE of them,
// unchanged and with the product's launch geometry, on inputs the test sets directly (tests/test_gpu_setup_stages.py); sd_fixed_mul_*
// first builds the table it reads with k_setup_fixed_table, as masp_hip_generate_parameters does.
// Everything that crosses this boundary is canonical: scalars 32 bytes little-endian (converted to and from Montgomery form on the host,
// where a kernel wants that), G1 96 and G2 192 bytes of bellman uncompressed form.  Every buffer a kernel writes is filled with the byte
// 0xA5 beforehand and has GUARD poisoned slots behind its end, which come back raw.  An index that would leave a buffer is refused here
// (-1), before any launch; n = 0 returns at once.  Non-zero on a HIP error; every function synchronises its stream exactly once.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/k_groth16.hip"
#include "../../masp_amd/csrc/device/msm.hpp"
#include "../../masp_amd/csrc/device/setup.hpp"

using namespace masp;

namespace {

constexpr int POISON = 0xA5;
constexpr uint32_t GUARD = 4;  // poisoned slots behind the end of every output
constexpr uint32_t TAB = 32 * 255;

// device buffers of one call, released when it returns
struct Scope {
    std::vector<void*> bufs;
    hipStream_t s = nullptr;
    bool ok = true;
    Scope() { ok = hipStreamCreate(&s) == hipSuccess; }
    ~Scope() {
        for (void* p : bufs) (void)hipFree(p);
        if (s) (void)hipStreamDestroy(s);
    }
    template <class T>
    T* alloc(size_t n) {
        void* p = nullptr;
        if (!ok || hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        bufs.push_back(p);
        return (T*)p;
    }
    template <class T>
    T* poisoned(size_t n) {
        T* d = alloc<T>(n);
        if (d && hipMemsetAsync(d, POISON, sizeof(T) * (n ? n : 1), s) != hipSuccess) ok = false;
        return d;
    }
    template <class T>
    T* upload(const T* h, size_t n) {
        T* d = alloc<T>(n);
        if (d && n && hipMemcpyAsync(d, h, sizeof(T) * n, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
        return d;
    }
    template <class T>
    void download(T* h, const T* d, size_t n) {
        if (ok && n && hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s) != hipSuccess) ok = false;
    }
    int finish() {
        if (!ok) return -2;
        if (hipStreamSynchronize(s) != hipSuccess) return -3;
        if (launch_status() != MASP_HIP_OK || hipGetLastError() != hipSuccess) return -4;
        return 0;
    }
};

// 32 little-endian bytes -> Fr, Montgomery if asked; false if not below r
bool fr_in(const uint8_t* b, bool mont, Fr& out) {
    const Fr v = fe_load_le<FrCfg>(b);
    if (fe_canonical_ge_mod(v)) return false;
    out = mont ? fe_to_mont(v) : v;
    return true;
}
bool fr_vec_in(const uint8_t* b, size_t n, bool mont, std::vector<Fr>& out) {
    out.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (!fr_in(b + 32 * i, mont, out[i])) return false;
    return true;
}
// n Montgomery results -> canonical bytes; the GUARD slots behind them raw
void fr_vec_out(const std::vector<Fr>& v, size_t n, uint8_t* out, uint8_t* guard) {
    for (size_t i = 0; i < n; ++i) fe_store_le(fe_from_mont(v[i]), out + 32 * i);
    memcpy(guard, v.data() + n, sizeof(Fr) * GUARD);
}
// runs `launch` over a poisoned Fr output of n + GUARD slots and brings it back
template <class L>
int fr_kernel(Scope& sc, uint32_t n, uint8_t* out, uint8_t* guard, L launch) {
    Fr* d_out = sc.poisoned<Fr>((size_t)n + GUARD);
    if (!sc.ok) return -2;
    launch(d_out);
    std::vector<Fr> h((size_t)n + GUARD);
    sc.download(h.data(), d_out, h.size());
    const int rc = sc.finish();
    if (rc) return rc;
    fr_vec_out(h, n, out, guard);
    return 0;
}

// a row or table entry as it came back: 1 every byte the poison, 2 every byte zero, 0 anything else (then `out` holds its wire form)
template <class A>
int raw_state(const A& p) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(&p);
    bool poison = true, zero = true;
    for (size_t k = 0; k < sizeof(A); ++k) {
        poison = poison && b[k] == POISON;
        zero = zero && b[k] == 0;
    }
    return poison ? 1 : zero ? 2 : 0;
}
void point_out(const G1Affine& p, uint8_t* out) { g1_write_uncompressed(p, out); }
void point_out(const G2Affine& p, uint8_t* out) { g2_write_uncompressed(p, out); }
int point_in(const uint8_t* in, G1Affine& p) { return g1_read_uncompressed(in, p); }
int point_in(const uint8_t* in, G2Affine& p) { return g2_read_uncompressed(in, p); }
template <class A>
void points_out(const A* p, size_t n, size_t width, uint8_t* out, uint8_t* state) {
    for (size_t i = 0; i < n; ++i) {
        state[i] = (uint8_t)raw_state(p[i]);
        if (state[i] == 1)
            memset(out + width * i, 0, width);
        else
            point_out(p[i], out + width * i);
    }
}

template <class O, int BYTES>
int fixed_table(const uint8_t* gen, uint8_t* out, uint8_t* state) {
    const ApiLaunchScope api_scope;
    Affine<O> g;
    if (point_in(gen, g) != PT_OK) return -1;
    Scope sc;
    Affine<O>* d_tab = sc.poisoned<Affine<O>>(TAB + GUARD);
    if (!sc.ok) return -2;
    MASP_LAUNCH((k_setup_fixed_table<O>), dim3(1), dim3(64), 0, sc.s, g, d_tab);
    std::vector<Affine<O>> h(TAB + GUARD);
    sc.download(h.data(), d_tab, h.size());
    const int rc = sc.finish();
    if (rc) return rc;
    points_out(h.data(), h.size(), BYTES, out, state);
    return 0;
}
template <class O, int BYTES>
int fixed_mul(const uint8_t* gen, const uint8_t* scalars32, uint32_t n, int mont, uint8_t* out, uint8_t* guard) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    Affine<O> g;
    std::vector<Fr> k;
    if (point_in(gen, g) != PT_OK || !fr_vec_in(scalars32, n, mont != 0, k)) return -1;
    Scope sc;
    Affine<O>* d_tab = sc.poisoned<Affine<O>>(TAB);
    const Fr* d_k = sc.upload(k.data(), n);
    uint8_t* d_out = sc.poisoned<uint8_t>((size_t)BYTES * (n + GUARD));
    if (!sc.ok) return -2;
    MASP_LAUNCH((k_setup_fixed_table<O>), dim3(1), dim3(64), 0, sc.s, g, d_tab);
    MASP_LAUNCH((k_setup_fixed_mul<O, BYTES>), dim3((n + 63) / 64), dim3(64), 0, sc.s, d_tab, d_k, n, mont, d_out);
    sc.download(out, d_out, (size_t)BYTES * n);
    sc.download(guard, d_out + (size_t)BYTES * n, (size_t)BYTES * GUARD);
    return sc.finish();
}
template <class O, int BYTES>
int msm_import(const uint8_t* raw, uint32_t n, uint8_t* out, uint8_t* state, int* status) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    Scope sc;
    const uint8_t* d_raw = sc.upload(raw, (size_t)BYTES * n);
    TabRow<O>* d_tab = sc.poisoned<TabRow<O>>((size_t)n + GUARD);
    int zero = 0;
    int* d_status = sc.upload(&zero, 1);
    if (!sc.ok) return -2;
    MASP_LAUNCH((k_msm_import<O, BYTES>), dim3((n + 63) / 64), dim3(64), 0, sc.s, d_raw, d_tab, n, d_status);
    std::vector<TabRow<O>> h((size_t)n + GUARD);
    sc.download(h.data(), d_tab, h.size());
    sc.download(status, d_status, 1);
    const int rc = sc.finish();
    if (rc) return rc;
    for (size_t i = 0; i < h.size(); ++i) points_out(&h[i].p, 1, BYTES, out + (size_t)BYTES * i, state + i);
    return 0;
}
template <class A, int BYTES, class L>
int import_one(const uint8_t* raw, uint8_t* out, uint8_t* state, int* status, L launch) {
    const ApiLaunchScope api_scope;
    Scope sc;
    const uint8_t* d_raw = sc.upload(raw, BYTES);
    A* d_out = sc.poisoned<A>(1 + GUARD);
    int zero = 0;
    int* d_status = sc.upload(&zero, 1);
    if (!sc.ok) return -2;
    launch(sc.s, d_raw, d_out, d_status);
    A h[1 + GUARD];
    sc.download(h, d_out, 1 + GUARD);
    sc.download(status, d_status, 1);
    const int rc = sc.finish();
    if (rc) return rc;
    points_out(h, 1 + GUARD, BYTES, out, state);
    return 0;
}

}  // namespace

extern "C" {

uint32_t sd_guard_slots(void) { return GUARD; }

// k_setup_lagrange: lag[k] for k < nrows
int sd_lagrange(uint32_t nrows, const uint8_t* omega32, const uint8_t* tau32, const uint8_t* z_over_m32, uint8_t* out, uint8_t* guard) {
    if (nrows == 0) return 0;
    const ApiLaunchScope api_scope;
    Fr omega, tau, zm;
    if (!fr_in(omega32, true, omega) || !fr_in(tau32, true, tau) || !fr_in(z_over_m32, true, zm)) return -1;
    Scope sc;
    return fr_kernel(sc, nrows, out, guard,
                     [&](Fr* d_out) { MASP_LAUNCH(k_setup_lagrange, dim3((nrows + 127) / 128), dim3(128), 0, sc.s, d_out, nrows, omega, tau, zm); });
}
// k_setup_qap over a CSC matrix of nv columns (colptr[nv + 1], rowidx / coef32 of colptr[nv] entries) and lag32 of n_lag values
int sd_qap(const uint32_t* colptr, const uint32_t* rowidx, const uint8_t* coef32, const uint8_t* lag32, uint32_t n_lag, uint32_t nv, uint32_t n_inputs,
           uint32_t n_constraints, int is_a, uint8_t* out, uint8_t* guard) {
    if (nv == 0) return 0;
    if (colptr[0] != 0) return -1;
    for (uint32_t v = 0; v < nv; ++v)
        if (colptr[v + 1] < colptr[v]) return -1;
    const uint32_t nnz = colptr[nv];
    for (uint32_t t = 0; t < nnz; ++t)
        if (rowidx[t] >= n_lag) return -1;
    if (is_a && (uint64_t)n_constraints + (nv < n_inputs ? nv : n_inputs) > n_lag) return -1;
    const ApiLaunchScope api_scope;
    std::vector<Fr> coef, lag;
    if (!fr_vec_in(coef32, nnz, true, coef) || !fr_vec_in(lag32, n_lag, true, lag)) return -1;
    Scope sc;
    const uint32_t* d_colptr = sc.upload(colptr, (size_t)nv + 1);
    const uint32_t* d_rowidx = sc.upload(rowidx, nnz);
    const Fr* d_coef = sc.upload(coef.data(), nnz);
    const Fr* d_lag = sc.upload(lag.data(), n_lag);
    return fr_kernel(sc, nv, out, guard, [&](Fr* d_out) {
        MASP_LAUNCH(k_setup_qap, dim3((nv + 127) / 128), dim3(128), 0, sc.s, d_colptr, d_rowidx, d_coef, d_lag, nv, n_inputs, n_constraints, is_a, d_out);
    });
}
// k_setup_lc
int sd_lc(const uint8_t* at32, const uint8_t* bt32, const uint8_t* ct32, uint32_t n, const uint8_t* alpha32, const uint8_t* beta32, const uint8_t* scale32,
          uint8_t* out, uint8_t* guard) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    std::vector<Fr> at, bt, ct;
    Fr alpha, beta, scale;
    if (!fr_vec_in(at32, n, true, at) || !fr_vec_in(bt32, n, true, bt) || !fr_vec_in(ct32, n, true, ct) || !fr_in(alpha32, true, alpha) ||
        !fr_in(beta32, true, beta) || !fr_in(scale32, true, scale))
        return -1;
    Scope sc;
    const Fr* d_at = sc.upload(at.data(), n);
    const Fr* d_bt = sc.upload(bt.data(), n);
    const Fr* d_ct = sc.upload(ct.data(), n);
    return fr_kernel(sc, n, out, guard,
                     [&](Fr* d_out) { MASP_LAUNCH(k_setup_lc, dim3((n + 255) / 256), dim3(256), 0, sc.s, d_at, d_bt, d_ct, n, alpha, beta, scale, d_out); });
}
// k_setup_nonzero: flags[n], then GUARD bytes raw
int sd_nonzero(const uint8_t* x32, uint32_t n, uint8_t* flags) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    std::vector<Fr> x;
    if (!fr_vec_in(x32, n, true, x)) return -1;
    Scope sc;
    const Fr* d_x = sc.upload(x.data(), n);
    uint8_t* d_flags = sc.poisoned<uint8_t>((size_t)n + GUARD);
    if (!sc.ok) return -2;
    MASP_LAUNCH(k_setup_nonzero, dim3((n + 255) / 256), dim3(256), 0, sc.s, d_x, n, d_flags);
    sc.download(flags, d_flags, (size_t)n + GUARD);
    return sc.finish();
}
// k_setup_gather: out[k] = src[idx[k]]
int sd_gather(const uint8_t* src32, uint32_t n_src, const uint32_t* idx, uint32_t n, uint8_t* out, uint8_t* guard) {
    if (n == 0) return 0;
    for (uint32_t k = 0; k < n; ++k)
        if (idx[k] >= n_src) return -1;
    const ApiLaunchScope api_scope;
    std::vector<Fr> src;
    if (!fr_vec_in(src32, n_src, true, src)) return -1;
    Scope sc;
    const Fr* d_src = sc.upload(src.data(), n_src);
    const uint32_t* d_idx = sc.upload(idx, n);
    return fr_kernel(sc, n, out, guard,
                     [&](Fr* d_out) { MASP_LAUNCH(k_setup_gather, dim3((n + 255) / 256), dim3(256), 0, sc.s, d_src, d_idx, n, d_out); });
}
// k_setup_h_scalars: out[i] = tau^i c
int sd_h_scalars(const uint8_t* tau32, const uint8_t* c32, uint32_t n, uint8_t* out, uint8_t* guard) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    Fr tau, c;
    if (!fr_in(tau32, true, tau) || !fr_in(c32, true, c)) return -1;
    Scope sc;
    return fr_kernel(sc, n, out, guard,
                     [&](Fr* d_out) { MASP_LAUNCH(k_setup_h_scalars, dim3((n + 255) / 256), dim3(256), 0, sc.s, tau, c, n, d_out); });
}
// k_setup_fixed_table: out / state for 32 * 255 + GUARD entries (state 1: the entry still holds the poison)
int sd_fixed_table_g1(const uint8_t* gen96, uint8_t* out96, uint8_t* state) { return fixed_table<FpOps, 96>(gen96, out96, state); }
int sd_fixed_table_g2(const uint8_t* gen192, uint8_t* out192, uint8_t* state) { return fixed_table<Fp2Ops, 192>(gen192, out192, state); }
// k_setup_fixed_mul over the table of gen: n points as bytes, then GUARD points' worth of bytes raw
int sd_fixed_mul_g1(const uint8_t* gen96, const uint8_t* scalars32, uint32_t n, int mont, uint8_t* out96, uint8_t* guard) {
    return fixed_mul<FpOps, 96>(gen96, scalars32, n, mont, out96, guard);
}
int sd_fixed_mul_g2(const uint8_t* gen192, const uint8_t* scalars32, uint32_t n, int mont, uint8_t* out192, uint8_t* guard) {
    return fixed_mul<Fp2Ops, 192>(gen192, scalars32, n, mont, out192, guard);
}
// k_msm_import: the first n + GUARD rows' points as bytes with a state each (1 poison, 2 all zero), and the status word
int sd_msm_import_g1(const uint8_t* raw96, uint32_t n, uint8_t* out96, uint8_t* state, int* status) {
    return msm_import<FpOps, 96>(raw96, n, out96, state, status);
}
int sd_msm_import_g2(const uint8_t* raw192, uint32_t n, uint8_t* out192, uint8_t* state, int* status) {
    return msm_import<Fp2Ops, 192>(raw192, n, out192, state, status);
}
// k_g1_import_one / k_g2_import_one through the loader's wrappers: 1 + GUARD slots
int sd_import_one_g1(const uint8_t* raw96, uint8_t* out96, uint8_t* state, int* status) {
    return import_one<G1Affine, 96>(raw96, out96, state, status, launch_g1_import_one);
}
int sd_import_one_g2(const uint8_t* raw192, uint8_t* out192, uint8_t* state, int* status) {
    return import_one<G2Affine, 192>(raw192, out192, state, status, launch_g2_import_one);
}

}  // extern "C"
