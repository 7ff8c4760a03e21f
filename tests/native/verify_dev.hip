// Test-only unit over the device half of the GPU batch verifier (masp_amd/csrc/device/pairing.hpp, device/subgroup.hpp): each of its
// kernels launched on its own, with the product's geometry, so that tests/test_gpu_verify_stages.py can compare every stage with big
// integers.  Everything that crosses this boundary is canonical bytes in the bellman wire formats, never Montgomery residues:
//   Fp      48 bytes big-endian;            Fp12  12 Fp in the flat order a.a.a, a.a.b, a.b.a, ... of masp_host::bls::Fp12
//   G1      96 bytes uncompressed (x | y);  G2    192 bytes uncompressed (x.c1 | x.c0 | y.c1 | y.c0);  identity 0x40 then zeros
// The _host functions are wrappers over masp_amd/csrc/host/pairing.h and touch no GPU.  Every _gpu function returns non-zero on a HIP
// error and synchronises its stream exactly once.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/device/pairing.hpp"
#include "../../masp_amd/csrc/host/pairing.h"
#include "../../masp_amd/csrc/host/pairing_prog.h"
#include "../../masp_amd/csrc/verify_launch.h"

using namespace masp;
namespace hb = masp_host::bls;

namespace {

// ---- bytes <-> device types (on the host: field.hpp's conversions are __host__ __device__) ----
Fp fp_of_be(const uint8_t* in) { return fe_to_mont(fe_load_be<FpCfg>(in)); }
void fp_to_be(const Fp& mont, uint8_t* out) { fe_store_be(fe_from_mont(mont), out); }
G1Affine g1_of_wire(const uint8_t* in) {  // an entry with the infinity flag, or of zeros only, is the identity (x = y = 0)
    if (in[0] & 0x40) return {fe_zero<FpCfg>(), fe_zero<FpCfg>()};
    return {fp_of_be(in), fp_of_be(in + 48)};
}
G2Affine g2_of_wire(const uint8_t* in) {
    if (in[0] & 0x40) return {Fp2Ops::zero(), Fp2Ops::zero()};
    return {{fp_of_be(in + 48), fp_of_be(in)}, {fp_of_be(in + 144), fp_of_be(in + 96)}};
}

// ---- bytes <-> host types ----
void hfp12_to_be(const hb::Fp12& f, uint8_t* out) {
    const hb::Fp* c = &f.a.a.a;  // 12 packed residues (static_assert below)
    for (int i = 0; i < 12; ++i) {
        uint64_t v[6];
        c[i].canon(v);
        for (int k = 0; k < 48; ++k) out[48 * i + k] = (uint8_t)(v[5 - k / 8] >> (8 * (7 - k % 8)));
    }
}
static_assert(sizeof(hb::Fp12) == 12 * 48, "Fp12 is 12 packed Montgomery residues");
bool hfp12_of_be(hb::Fp12& f, const uint8_t* in) {
    hb::Fp* c = &f.a.a.a;
    for (int i = 0; i < 12; ++i)
        if (!hb::Fp::from_be(c[i], in + 48 * i)) return false;
    return true;
}

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

bool raise_lds() {
    return hipFuncSetAttribute((const void*)k_miller_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_fp12_product, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
}

__global__ void __launch_bounds__(64) k_xyzz_export(const G1Xyzz* __restrict__ p, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g1_write_uncompressed(xyzz_to_affine<FpOps, true>(p[i]), out + 96 * (size_t)i);
}

}  // namespace

extern "C" {

// proofs n x 192, z n x 16 -> status n ints, za n x 96, b n x 192, zc n x 96 (affine)
int vfy_prepare_gpu(const uint8_t* proofs, const uint8_t* z, uint32_t n, int* status, uint8_t* za, uint8_t* b, uint8_t* zc) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    Scope sc;
    const uint8_t* d_proofs = sc.upload(proofs, 192 * (size_t)n);
    const uint8_t* d_z = sc.upload(z, 16 * (size_t)n);
    G1Affine* d_za = sc.alloc<G1Affine>(n);
    G2Affine* d_b = sc.alloc<G2Affine>(n);
    G1Xyzz* d_zc = sc.alloc<G1Xyzz>(n);
    int* d_status = sc.alloc<int>(n);
    uint8_t* d_zc96 = sc.alloc<uint8_t>(96 * (size_t)n);
    if (!sc.ok) return -1;
    // b and za of a proof whose point does not decode are whatever the buffer held: zeros here, so that a run repeats
    if (hipMemsetAsync(d_status, 0, sizeof(int) * n, sc.s) != hipSuccess || hipMemsetAsync(d_za, 0, sizeof(G1Affine) * n, sc.s) != hipSuccess ||
        hipMemsetAsync(d_b, 0, sizeof(G2Affine) * n, sc.s) != hipSuccess || hipMemsetAsync(d_zc, 0, sizeof(G1Xyzz) * n, sc.s) != hipSuccess)
        return -1;
    MASP_LAUNCH(k_verify_prepare, dim3((n + 63) / 64, 5), dim3(64), 0, sc.s, d_proofs, d_z, n, d_za, d_b, d_zc, d_status);
    MASP_LAUNCH(k_xyzz_export, dim3((n + 63) / 64), dim3(64), 0, sc.s, d_zc, n, d_zc96);
    std::vector<G1Affine> h_za(n);
    std::vector<G2Affine> h_b(n);
    sc.download(status, d_status, n);
    sc.download(h_za.data(), d_za, n);
    sc.download(h_b.data(), d_b, n);
    sc.download(zc, d_zc96, 96 * (size_t)n);
    const int rc = sc.finish();
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        g1_write_uncompressed(h_za[i], za + 96 * (size_t)i);
        g2_write_uncompressed(h_b[i], b + 192 * (size_t)i);
    }
    return 0;
}

// points n x 96 (affine; an entry of zeros only is the identity) -> their sum, 96 bytes
int vfy_g1_sum_gpu(const uint8_t* points96, uint32_t n, uint8_t* out96) {
    const ApiLaunchScope api_scope;
    std::vector<G1Xyzz> h(n);
    for (uint32_t i = 0; i < n; ++i) h[i] = xyzz_from_affine(g1_of_wire(points96 + 96 * (size_t)i));
    Scope sc;
    const G1Xyzz* d_zc = sc.upload(h.data(), n);
    uint8_t* d_sum = sc.alloc<uint8_t>(96);
    if (!sc.ok) return -1;
    MASP_LAUNCH(k_g1_sum_export, dim3(1), dim3(256), 0, sc.s, d_zc, n, d_sum);
    sc.download(out96, d_sum, 96);
    return sc.finish();
}

// pairs (p n x 96, q n x 192) -> n Miller values of 12 Fp
int vfy_miller_gpu(const uint8_t* p96, const uint8_t* q192, uint32_t n, uint8_t* out) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    const ProgramTable pr = pairing_program_table();   // what masp_hip_vk_prepare uploads
    const uint32_t lds = pr.n_slots * 48;
    if (lds > 64 * 1024 || !raise_lds()) return -5;
    std::vector<G1Affine> hp(n);
    std::vector<G2Affine> hq(n);
    for (uint32_t i = 0; i < n; ++i) {
        hp[i] = g1_of_wire(p96 + 96 * (size_t)i);
        hq[i] = g2_of_wire(q192 + 192 * (size_t)i);
    }
    Scope sc;
    const uint32_t* d_ops = sc.upload(pr.ops.data(), pr.ops.size());
    const uint32_t* d_steps = sc.upload(pr.steps.data(), pr.steps.size());
    const G1Affine* d_p = sc.upload(hp.data(), n);
    const G2Affine* d_q = sc.upload(hq.data(), n);
    Fp* d_f = sc.alloc<Fp>(12 * (size_t)n);
    if (!sc.ok) return -1;
    MASP_LAUNCH(k_miller_pairs, dim3(n), dim3(64), lds, sc.s, pr.dev(0, d_ops, d_steps), pr.dev(1, d_ops, d_steps), pr.n_slots, d_p, d_q, d_f);
    std::vector<Fp> hf(12 * (size_t)n);
    sc.download(hf.data(), d_f, hf.size());
    const int rc = sc.finish();
    if (rc) return rc;
    for (size_t i = 0; i < hf.size(); ++i) fp_to_be(hf[i], out + 48 * i);
    return 0;
}

// n values of 12 Fp -> their product, by the schedule masp_hip_verify_batch runs (verify_launch.h)
int vfy_fp12_product_gpu(const uint8_t* vals, uint32_t n, uint8_t* out) {
    if (n == 0) return -1;
    const ApiLaunchScope api_scope;
    const ProgramTable pr = pairing_program_table();   // what masp_hip_vk_prepare uploads
    const uint32_t lds = pr.n_slots * 48;
    if (lds > 64 * 1024 || !raise_lds()) return -5;
    std::vector<Fp> hf(12 * (size_t)n);
    for (size_t i = 0; i < hf.size(); ++i) hf[i] = fp_of_be(vals + 48 * i);
    Scope sc;
    const uint32_t* d_ops = sc.upload(pr.ops.data(), pr.ops.size());
    const uint32_t* d_steps = sc.upload(pr.steps.data(), pr.steps.size());
    Fp* d_f = sc.upload(hf.data(), hf.size());
    if (!sc.ok) return -1;
    launch_fp12_product(sc.s, pr.dev(2, d_ops, d_steps), pr.n_slots, lds, d_f, n);
    Fp r[12];
    sc.download(r, d_f, 12);
    const int rc = sc.finish();
    if (rc) return rc;
    for (int i = 0; i < 12; ++i) fp_to_be(r[i], out + 48 * i);
    return 0;
}

// ---- host/pairing.h, no GPU ----
int vfy_miller_host(const uint8_t* p96, const uint8_t* q192, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        hb::G1A P;
        hb::G2A Q;
        if (!hb::g1_uncompressed(P, p96 + 96 * (size_t)i) || !hb::g2_uncompressed(Q, q192 + 192 * (size_t)i)) return -1;
        hfp12_to_be(hb::miller(P, Q), out + 576 * (size_t)i);
    }
    return 0;
}
int vfy_fp12_mul_host(const uint8_t* a, const uint8_t* b, uint8_t* out) {
    hb::Fp12 x, y;
    if (!hfp12_of_be(x, a) || !hfp12_of_be(y, b)) return -1;
    hfp12_to_be(x * y, out);
    return 0;
}
// 1 if f^((p^12 - 1)/r) is one, 0 if not, < 0 if the bytes are not canonical
int vfy_final_exp_is_one_host(const uint8_t* f) {
    hb::Fp12 x;
    if (!hfp12_of_be(x, f)) return -1;
    return hb::final_exp(x) == hb::Fp12::one() ? 1 : 0;
}
int vfy_final_exp_eq_host(const uint8_t* a, const uint8_t* b) {
    hb::Fp12 x, y;
    if (!hfp12_of_be(x, a) || !hfp12_of_be(y, b)) return -1;
    return hb::final_exp(x) == hb::final_exp(y) ? 1 : 0;
}

}  // extern "C"
