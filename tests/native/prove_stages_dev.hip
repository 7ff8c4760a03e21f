// Test-only unit over the prover's witness-to-quotient kernels (masp_amd/csrc/device/r1cs.hpp and the bit-reversal / pointwise kernels
// of device/ntt.hpp): each launched on its own through the product's OWN launch wrapper — this unit includes k_ntt.hip — so that
// tests/test_gpu_prove_stages.py can compare every stage, grid geometry included, with Python big integers.
// Scalars cross this boundary as canonical little-endian 32-byte values; where a kernel takes or leaves Montgomery residues the unit
// converts on the host (field.hpp's conversions are __host__ __device__), except where the conversion IS the kernel under test
// (to_mont, split_forms: raw residues out) or the kernel's operands are plain by contract (the scale of ab_eval / fr_scale_sub /
// fr_scale).  Every strided output is filled with a marker byte first, so that the test sees what a kernel wrote between rows.
// Every _gpu function checks its sizes before it launches, returns non-zero on a HIP error and synchronises its stream exactly once.
#include "../../masp_amd/csrc/k_ntt.hip"

#include <cstring>
#include <vector>

using namespace masp;

namespace {

// device buffers of one call, released when it returns (as in verify_dev.hip)
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
    T* filled(size_t n, uint8_t marker) {
        T* d = alloc<T>(n);
        if (d && hipMemsetAsync(d, marker, sizeof(T) * (n ? n : 1), s) != hipSuccess) ok = false;
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
    // the call's one synchronisation; also what a launch left behind
    int finish() {
        if (!ok) return -2;
        if (hipStreamSynchronize(s) != hipSuccess) return -3;
        if (launch_status() != MASP_HIP_OK || hipGetLastError() != hipSuccess) return -4;
        return 0;
    }
};

static_assert(sizeof(Fr) == 32, "Fr is eight 32-bit limbs, little-endian: the canonical wire form");
const int E_SIZES = -6;  // the sizes given would make a kernel read or write outside its buffers

// n scalars as the caller's bytes hold them (which outlive the call's one synchronisation)
Fr* up_raw(Scope& sc, const uint8_t* in, size_t n) { return (Fr*)sc.upload(in, 32 * n); }
void down_raw(Scope& sc, uint8_t* out, const Fr* d, size_t n) { sc.download(out, (const uint8_t*)d, 32 * n); }
std::vector<Fr> mont(const uint8_t* in, size_t n) {
    std::vector<Fr> v(n);
    if (n) memcpy(v.data(), in, 32 * n);
    for (Fr& x : v) x = fe_to_mont(x);
    return v;
}
void canonical_in_place(uint8_t* io, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        Fr x;
        memcpy(&x, io + 32 * i, 32);
        x = fe_from_mont(x);
        memcpy(io + 32 * i, &x, 32);
    }
}
Fr one_raw(const uint8_t* in) {
    Fr x;
    memcpy(&x, in, 32);
    return x;
}

}  // namespace

extern "C" {

// k_fr_to_mont: x np rows of n, x_stride apart (np * x_stride elements given) -> y np x n RAW Montgomery residues, *flag the range flag
int pst_to_mont_gpu(const uint8_t* x, uint64_t x_stride, uint32_t n, uint32_t np, uint8_t* y, int* flag) {
    if (n == 0 || np == 0 || x_stride < n) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const Fr* d_x = up_raw(sc, x, (size_t)np * x_stride);
    Fr* d_y = sc.filled<Fr>((size_t)np * n, 0x5A);
    int* d_flag = sc.filled<int>(1, 0);
    if (!sc.ok) return -1;
    launch_fr_to_mont(sc.s, d_x, (size_t)x_stride, d_y, n, np, d_flag);
    down_raw(sc, y, d_y, (size_t)np * n);
    sc.download(flag, d_flag, 1);
    return sc.finish();
}

// k_fr_split_forms: as above with the elements from mont_from on arriving as Montgomery residues; x (np * x_stride elements, the gaps
// included) comes back as the kernel left it
int pst_split_forms_gpu(uint8_t* x, uint64_t x_stride, uint32_t n, uint32_t mont_from, uint32_t np, uint8_t* y, int* flag) {
    if (n == 0 || np == 0 || x_stride < n) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    Fr* d_x = up_raw(sc, x, (size_t)np * x_stride);
    Fr* d_y = sc.filled<Fr>((size_t)np * n, 0x5A);
    int* d_flag = sc.filled<int>(1, 0);
    if (!sc.ok) return -1;
    launch_fr_split_forms(sc.s, d_x, (size_t)x_stride, d_y, n, mont_from, np, d_flag);
    down_raw(sc, y, d_y, (size_t)np * n);
    down_raw(sc, x, d_x, (size_t)np * x_stride);
    sc.download(flag, d_flag, 1);
    return sc.finish();
}

// k_r1cs_eval: three CSR matrices (rowptr n_constraints + 1, col / coef rowptr[n_constraints] canonical), each with its row order and
// n_long; w np assignments of n_inputs + n_aux canonical values -> out[i] np x (n_constraints + n_inputs) canonical, i < n_mat.
// Coefficients and assignments go through launch_fr_to_mont as the loader and enqueue_proofs send them; with n_mat = 2 the third
// matrix's pointers are null, as enqueue_proofs passes them.  *flag: the range flag of the assignments' conversion.
int pst_r1cs_eval_gpu(uint32_t n_inputs, uint32_t n_aux, uint32_t n_constraints, const uint32_t* const* rowptr, const uint32_t* const* col,
                      const uint8_t* const* coef, const uint32_t* const* order, const uint32_t* n_long, const uint8_t* w, uint32_t np,
                      uint32_t n_mat, uint8_t* const* out, int* flag) {
    const uint32_t n_vars = n_inputs + n_aux, nrows = n_constraints + n_inputs;
    if (n_mat < 2 || n_mat > 3 || np == 0 || n_inputs == 0 || n_constraints == 0) return E_SIZES;
    for (int i = 0; i < 3; ++i) {  // what the kernel indexes with: checked here, on the host
        if (rowptr[i][0] != 0 || n_long[i] > n_constraints) return E_SIZES;
        std::vector<bool> seen(n_constraints, false);
        for (uint32_t r = 0; r < n_constraints; ++r) {
            if (rowptr[i][r + 1] < rowptr[i][r] || order[i][r] >= n_constraints || seen[order[i][r]]) return E_SIZES;
            seen[order[i][r]] = true;
        }
        for (uint32_t t = 0; t < rowptr[i][n_constraints]; ++t)
            if (col[i][t] >= n_vars) return E_SIZES;
    }
    const ApiLaunchScope api_scope;
    Scope sc;
    R1csMatrices M;
    Fr* d_out[3] = {nullptr, nullptr, nullptr};
    int* d_flag = sc.filled<int>(2, 0);  // [0] the assignments', [1] the coefficients'
    for (uint32_t i = 0; i < 3; ++i) {
        if (i >= n_mat) {
            M.rowptr[i] = M.order[i] = M.col[i] = nullptr;
            M.coef[i] = nullptr;
            M.out[i] = nullptr;
            M.n_long[i] = 0;
            continue;
        }
        const uint32_t nnz = rowptr[i][n_constraints];
        const Fr* d_raw = up_raw(sc, coef[i], nnz);
        Fr* d_coef = sc.alloc<Fr>(nnz);
        M.rowptr[i] = sc.upload(rowptr[i], (size_t)n_constraints + 1);
        M.order[i] = sc.upload(order[i], n_constraints);
        M.col[i] = sc.upload(col[i], nnz);
        M.coef[i] = d_coef;
        M.out[i] = sc.filled<Fr>((size_t)np * nrows, 0x5A);
        M.n_long[i] = n_long[i];
        d_out[i] = sc.alloc<Fr>((size_t)np * nrows);
        if (!sc.ok) return -1;
        if (nnz) launch_fr_to_mont(sc.s, d_raw, (size_t)0, d_coef, nnz, 1, d_flag + 1);
    }
    const Fr* d_w = up_raw(sc, w, (size_t)np * n_vars);
    Fr* d_wm = sc.alloc<Fr>((size_t)np * n_vars);
    if (!sc.ok) return -1;
    launch_fr_to_mont(sc.s, d_w, (size_t)n_vars, d_wm, n_vars, np, d_flag);
    launch_r1cs_eval(sc.s, M, d_wm, n_vars, n_constraints, n_inputs, np, n_mat);
    int hflag[2] = {0, 0};
    for (uint32_t i = 0; i < n_mat; ++i) {
        launch_fr_from_mont(sc.s, M.out[i], d_out[i], np * nrows);
        down_raw(sc, out[i], d_out[i], (size_t)np * nrows);
    }
    sc.download(hflag, d_flag, 2);
    const int rc = sc.finish();
    if (rc) return rc;
    if (hflag[1]) return E_SIZES;  // a coefficient that is not canonical
    *flag = hflag[0];
    return 0;
}

// k_gather_scalars: src np rows, src_stride apart; idx n indices below src_stride -> dst np rows, dst_stride apart (0: n), raw copies
int pst_gather_scalars_gpu(const uint8_t* src, uint64_t src_stride, const uint32_t* idx, uint32_t n, uint32_t np, uint8_t* dst, uint64_t dst_stride,
                           uint8_t marker) {
    const size_t ds = dst_stride ? (size_t)dst_stride : (size_t)n;
    if (n == 0 || np == 0 || ds < n) return E_SIZES;
    for (uint32_t k = 0; k < n; ++k)
        if (idx[k] >= src_stride) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const Fr* d_src = up_raw(sc, src, (size_t)np * src_stride);
    const uint32_t* d_idx = sc.upload(idx, n);
    Fr* d_dst = sc.filled<Fr>(np * ds, marker);
    if (!sc.ok) return -1;
    launch_gather_scalars(sc.s, d_src, (size_t)src_stride, d_idx, n, d_dst, np, (size_t)dst_stride);
    down_raw(sc, dst, d_dst, np * ds);
    return sc.finish();
}

// k_ntt_load_bitrev (montgomery_in = 0: the kernel converts) / k_ntt_copy_bitrev (1: x sent in Montgomery form): x np rows of
// nrows <= 2^logm, x_stride apart -> y np x 2^logm canonical, y[rev(k)] = x[k], 0 from nrows on.  y starts as marker bytes: the zeros
// are the kernel's.
int pst_bitrev_gpu(int montgomery_in, const uint8_t* x, uint64_t x_stride, uint32_t nrows, uint32_t logm, uint32_t np, uint8_t* y, uint8_t marker) {
    if (logm == 0 || logm > 20 || np == 0 || nrows > (1u << logm) || x_stride < nrows || x_stride == 0) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm;
    const std::vector<Fr> hx = montgomery_in ? mont(x, (size_t)np * x_stride) : std::vector<Fr>();
    const Fr* d_x = montgomery_in ? sc.upload(hx.data(), hx.size()) : up_raw(sc, x, (size_t)np * x_stride);
    Fr* d_y = sc.filled<Fr>(np * m, marker);
    if (!sc.ok) return -1;
    if (montgomery_in)
        launch_ntt_copy_bitrev(sc.s, d_x, (size_t)x_stride, nrows, d_y, logm, np);
    else
        launch_ntt_load_bitrev(sc.s, d_x, (size_t)x_stride, nrows, d_y, logm, np);
    down_raw(sc, y, d_y, np * m);
    const int rc = sc.finish();
    if (rc) return rc;
    canonical_in_place(y, np * m);
    return 0;
}

// k_ntt_scale_bitrev (b == null): y[rev(k)] = a[k] * scale[k];  k_ntt_ab_bitrev (scale == null): y[rev(k)] = a[k] * b[k]
// (a, b np x 2^logm, scale 2^logm, all sent in Montgomery form; y np x 2^logm canonical)
int pst_mul_bitrev_gpu(const uint8_t* a, const uint8_t* b, const uint8_t* scale, uint32_t logm, uint32_t np, uint8_t* y) {
    if (logm == 0 || logm > 20 || np == 0 || !a || !b == !scale) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm;
    const std::vector<Fr> ha = mont(a, np * m), hb = b ? mont(b, np * m) : mont(scale, m);
    const Fr* d_a = sc.upload(ha.data(), ha.size());
    const Fr* d_b = sc.upload(hb.data(), hb.size());
    Fr* d_y = sc.filled<Fr>(np * m, 0x5A);
    if (!sc.ok) return -1;
    if (b)
        launch_ntt_ab_bitrev(sc.s, d_a, d_b, d_y, logm, np);
    else
        launch_ntt_scale_bitrev(sc.s, d_a, d_b, d_y, logm, np);
    down_raw(sc, y, d_y, np * m);
    const int rc = sc.finish();
    if (rc) return rc;
    canonical_in_place(y, np * m);
    return 0;
}

// k_ntt_ab_eval: y_p[k] = a_p[k] * b_p[k] * scale   (a, b np x n sent in Montgomery form, scale plain: y np rows, y_stride apart, as left)
int pst_ab_eval_gpu(const uint8_t* a, const uint8_t* b, const uint8_t* scale, uint32_t n, uint32_t np, uint8_t* y, uint64_t y_stride, uint8_t marker) {
    if (n == 0 || np == 0 || y_stride < n) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const std::vector<Fr> ha = mont(a, (size_t)np * n), hb = mont(b, (size_t)np * n);
    const Fr* d_a = sc.upload(ha.data(), ha.size());
    const Fr* d_b = sc.upload(hb.data(), hb.size());
    Fr* d_y = sc.filled<Fr>(np * (size_t)y_stride, marker);
    if (!sc.ok) return -1;
    launch_ntt_ab_eval(sc.s, d_a, d_b, one_raw(scale), d_y, n, np, (size_t)y_stride);
    down_raw(sc, y, d_y, np * (size_t)y_stride);
    return sc.finish();
}

// k_fr_scale_sub (c != null): y_p[k] = x_p[k] * scale[k] - c_p[k] * cscale;  k_fr_scale (c == null): y_p[k] = x_p[k] * scale[k]
// (x, c np x n sent in Montgomery form, scale n and cscale plain: y np rows, y_stride apart (0: n), as left)
int pst_fr_scale_gpu(const uint8_t* x, const uint8_t* scale, const uint8_t* c, const uint8_t* cscale, uint32_t n, uint32_t np, uint8_t* y,
                     uint64_t y_stride, uint8_t marker) {
    const size_t ys = y_stride ? (size_t)y_stride : (size_t)n;
    if (n == 0 || np == 0 || ys < n || (c && !cscale)) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const std::vector<Fr> hx = mont(x, (size_t)np * n), hc = c ? mont(c, (size_t)np * n) : std::vector<Fr>();
    const Fr* d_x = sc.upload(hx.data(), hx.size());
    const Fr* d_s = up_raw(sc, scale, n);
    const Fr* d_c = c ? sc.upload(hc.data(), hc.size()) : nullptr;
    Fr* d_y = sc.filled<Fr>(np * ys, marker);
    if (!sc.ok) return -1;
    if (c)
        launch_fr_scale_sub(sc.s, d_x, d_s, d_c, one_raw(cscale), d_y, n, np, (size_t)y_stride);
    else
        launch_fr_scale(sc.s, d_x, d_s, d_y, n, np, (size_t)y_stride);
    down_raw(sc, y, d_y, np * ys);
    return sc.finish();
}

}  // extern "C"
