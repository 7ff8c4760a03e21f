// Test-only unit over the evaluation-form quotient's three kernels (masp_amd/csrc/device/ntt.hpp: k_ntt_dif_top, k_ntt_mid,
// k_ntt_dit_top_ab), each launched on its own through the product's OWN launch wrapper — this unit includes k_ntt.hip — and over the two
// whole chains, the three kernels and the seven launches they replace, so that tests/test_gpu_quotient_fused.py can compare every kernel
// with Python big integers and the chains with each other.  The tables are built here as NttDomain::init builds them, with the product's
// launch_fr_powers / launch_fr_powers_bitrev.
// Scalars cross this boundary as canonical little-endian 32-byte values (the unit converts on the host; field.hpp's conversions are
// __host__ __device__).  Every strided output is filled with a marker byte first.  Every _gpu function checks its sizes before it
// launches, returns non-zero on a HIP error and synchronises its stream exactly once.
#include "../../masp_amd/csrc/k_ntt.hip"

#include <cstring>
#include <vector>

using namespace masp;

namespace {

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
    int finish() {
        if (!ok) return -2;
        if (hipStreamSynchronize(s) != hipSuccess) return -3;
        if (launch_status() != MASP_HIP_OK || hipGetLastError() != hipSuccess) return -4;
        return 0;
    }
};

static_assert(sizeof(Fr) == 32, "Fr is eight 32-bit limbs, little-endian: the canonical wire form");
const int E_SIZES = -6;  // the sizes given would make a kernel read or write outside its buffers

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
Fr fr_limbs(const uint32_t* limbs) {
    Fr v;
    for (int i = 0; i < 8; ++i) v.v[i] = limbs[i];
    return v;
}

// a domain's tables, as NttDomain::init (masp_amd/csrc/internal.h) builds them
struct Tables {
    Fr *tw_fwd = nullptr, *tw_inv = nullptr, *coset_scale = nullptr, *coset_scale_rev = nullptr;
    Fr e_scale;
    bool build(Scope& sc, uint32_t logm) {
        const size_t m = (size_t)1 << logm, half = m / 2;
        Fr omega = fr_limbs(FrCfg::ROOT_OF_UNITY);
        for (uint32_t i = logm; i < 32; ++i) omega = fe_sqr(omega);
        const Fr omega_inv = fe_inv(omega), one = fe_one<FrCfg>(), g = fr_limbs(FrCfg::GEN);
        Fr mm = fe_zero<FrCfg>();
        mm.v[0] = (uint32_t)m;
        const Fr minv = fe_inv(fe_to_mont(mm));
        uint32_t e[2] = {(uint32_t)m, 0};
        e_scale = fe_from_mont(fe_inv(fe_sub(fe_pow(g, e, 2), one)));
        tw_fwd = sc.alloc<Fr>(half);
        tw_inv = sc.alloc<Fr>(half);
        coset_scale = sc.alloc<Fr>(m);
        coset_scale_rev = sc.alloc<Fr>(m);
        if (!sc.ok) return false;
        launch_fr_powers(sc.s, tw_fwd, (uint32_t)half, omega, one, 0);
        launch_fr_powers(sc.s, tw_inv, (uint32_t)half, omega_inv, one, 0);
        launch_fr_powers(sc.s, coset_scale, (uint32_t)m, g, minv, 0);
        launch_fr_powers_bitrev(sc.s, coset_scale_rev, logm, g, minv);
        return true;
    }
};
// NttDomain::passes
void passes(hipStream_t s, Fr* data, const Fr* tw, uint32_t logm, uint32_t np) {
    for (uint32_t s0 = 0; s0 < logm;) {
        const uint32_t nst = std::min<uint32_t>(NTT_LT, logm - s0);
        launch_ntt_pass(s, data, tw, logm, s0, nst, np);
        s0 += nst;
    }
}
bool sizes_ok(uint32_t logm, uint32_t q) { return ntt_fused_ok(logm) && q >= 1 && q <= 64; }

}  // namespace

extern "C" {

// the product's own predicate for the three-kernel schedule (enqueue_quotient_eval runs the separate passes where it is false)
int qf_fused_ok(uint32_t logm) { return ntt_fused_ok(logm) ? 1 : 0; }
uint32_t qf_tile_log() { return (uint32_t)NTT_LT; }

// launch_fr_powers_bitrev: table[i] = scale * base^rev(i), i < 2^logn, canonical in and out
int qf_powers_bitrev_gpu(uint32_t logn, const uint8_t* base, const uint8_t* scale, uint8_t* table) {
    if (logn == 0 || logn > 20) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t n = (size_t)1 << logn;
    Fr* d = sc.filled<Fr>(n, 0x5A);
    if (!sc.ok) return -1;
    launch_fr_powers_bitrev(sc.s, d, logn, mont(base, 1)[0], mont(scale, 1)[0]);
    sc.download(table, (const uint8_t*)d, 32 * n);
    const int rc = sc.finish();
    if (rc) return rc;
    canonical_in_place(table, n);
    return 0;
}

// k_ntt_dif_top: a, b q rows of nrows <= 2^logm values each, in_stride apart (q * in_stride elements given) -> y: [a | b], 2 q x 2^logm
int qf_dif_top_gpu(const uint8_t* a, const uint8_t* b, uint64_t in_stride, uint32_t nrows, uint32_t logm, uint32_t q, uint8_t* y, uint8_t marker) {
    if (!sizes_ok(logm, q) || nrows == 0 || nrows > (1u << logm) || in_stride < nrows) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm;
    Tables T;
    if (!T.build(sc, logm)) return -1;
    const std::vector<Fr> ha = mont(a, (size_t)q * in_stride), hb = mont(b, (size_t)q * in_stride);
    const Fr* d_a = sc.upload(ha.data(), ha.size());
    const Fr* d_b = sc.upload(hb.data(), hb.size());
    Fr* d_y = sc.filled<Fr>(2 * q * m, marker);
    if (!sc.ok) return -1;
    launch_ntt_dif_top(sc.s, d_a, d_b, (size_t)in_stride, nrows, d_y, T.tw_inv, logm, q);
    sc.download(y, (const uint8_t*)d_y, 32 * 2 * q * m);
    const int rc = sc.finish();
    if (rc) return rc;
    canonical_in_place(y, 2 * q * m);
    return 0;
}

// k_ntt_mid, in place on np transforms of 2^logm
int qf_mid_gpu(uint8_t* x, uint32_t logm, uint32_t np) {
    if (!sizes_ok(logm, np)) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm;
    Tables T;
    if (!T.build(sc, logm)) return -1;
    const std::vector<Fr> hx = mont(x, np * m);
    Fr* d_x = sc.upload(hx.data(), hx.size());
    if (!sc.ok) return -1;
    launch_ntt_mid(sc.s, d_x, T.tw_inv, T.coset_scale_rev, T.tw_fwd, logm, np);
    sc.download(x, (const uint8_t*)d_x, 32 * np * m);
    const int rc = sc.finish();
    if (rc) return rc;
    canonical_in_place(x, np * m);
    return 0;
}

// k_ntt_dit_top_ab: x = [a | b], 2 q x 2^logm -> y q rows of 2^logm, y_stride apart, as the kernel left them (canonical by contract)
int qf_dit_top_ab_gpu(const uint8_t* x, uint32_t logm, uint32_t q, uint8_t* y, uint64_t y_stride, uint8_t marker) {
    if (!sizes_ok(logm, q) || y_stride < ((uint64_t)1 << logm)) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm;
    Tables T;
    if (!T.build(sc, logm)) return -1;
    const std::vector<Fr> hx = mont(x, 2 * q * m);
    const Fr* d_x = sc.upload(hx.data(), hx.size());
    Fr* d_y = sc.filled<Fr>(q * (size_t)y_stride, marker);
    if (!sc.ok) return -1;
    launch_ntt_dit_top_ab(sc.s, d_x, q * m, T.tw_fwd, T.e_scale, d_y, (size_t)y_stride, logm, q);
    sc.download(y, (const uint8_t*)d_y, 32 * q * (size_t)y_stride);
    return sc.finish();
}

// Both whole chains of enqueue_quotient_eval over the same inputs (a, b: q rows of nrows RAW Montgomery residues below r, in_stride apart):
// y_fused — the three kernels on one work buffer — and y_separate — copy_bitrev x 2, the inverse passes, scale_bitrev, the forward
// passes, ab_eval — each q rows of 2^logm, y_stride apart, as the kernels left them.
int qf_chains_gpu(const uint8_t* a, const uint8_t* b, uint64_t in_stride, uint32_t nrows, uint32_t logm, uint32_t q, uint8_t* y_fused,
                  uint8_t* y_separate, uint64_t y_stride, uint8_t marker) {
    if (!sizes_ok(logm, q) || nrows == 0 || nrows > (1u << logm) || in_stride < nrows || y_stride < ((uint64_t)1 << logm)) return E_SIZES;
    const ApiLaunchScope api_scope;
    Scope sc;
    const size_t m = (size_t)1 << logm, part = q * m;
    Tables T;
    if (!T.build(sc, logm)) return -1;
    const Fr* d_a = (const Fr*)sc.upload(a, 32 * (size_t)q * in_stride);
    const Fr* d_b = (const Fr*)sc.upload(b, 32 * (size_t)q * in_stride);
    Fr* x0 = sc.alloc<Fr>(2 * part);
    Fr* x1 = sc.alloc<Fr>(2 * part);
    Fr* d_f = sc.filled<Fr>(q * (size_t)y_stride, marker);
    Fr* d_s = sc.filled<Fr>(q * (size_t)y_stride, marker);
    if (!sc.ok) return -1;
    launch_ntt_dif_top(sc.s, d_a, d_b, (size_t)in_stride, nrows, x0, T.tw_inv, logm, q);
    launch_ntt_mid(sc.s, x0, T.tw_inv, T.coset_scale_rev, T.tw_fwd, logm, 2 * q);
    launch_ntt_dit_top_ab(sc.s, x0, part, T.tw_fwd, T.e_scale, d_f, (size_t)y_stride, logm, q);
    launch_ntt_copy_bitrev(sc.s, d_a, (size_t)in_stride, nrows, x0, logm, q);
    launch_ntt_copy_bitrev(sc.s, d_b, (size_t)in_stride, nrows, x0 + part, logm, q);
    passes(sc.s, x0, T.tw_inv, logm, 2 * q);
    launch_ntt_scale_bitrev(sc.s, x0, T.coset_scale, x1, logm, 2 * q);
    passes(sc.s, x1, T.tw_fwd, logm, 2 * q);
    launch_ntt_ab_eval(sc.s, x1, x1 + part, T.e_scale, d_s, (uint32_t)m, q, (size_t)y_stride);
    sc.download(y_fused, (const uint8_t*)d_f, 32 * q * (size_t)y_stride);
    sc.download(y_separate, (const uint8_t*)d_s, 32 * q * (size_t)y_stride);
    return sc.finish();
}

}  // extern "C"
