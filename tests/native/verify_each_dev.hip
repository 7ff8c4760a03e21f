// Test-only unit over the device half of masp_hip_verify_each (masp_amd/csrc/device/pairing.hpp): k_final_exp and k_verify_acc launched
// on their own, with the product's tables (masp_amd/csrc/verify_launch.h) and geometry, so that tests/test_gpu_verify_each_stages.py can
// compare each with big integers and with the host's final exponentiation.  As in verify_dev.hip everything that crosses this boundary
// is canonical bytes: Fp 48 bytes big-endian, Fp12 12 Fp in the flat order of masp_host::bls::Fp12, G1 96 bytes uncompressed (identity:
// 0x40 then zeros).  Every _gpu function returns non-zero on a HIP error and synchronises its stream exactly once.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/device/pairing.hpp"
#include "../../masp_amd/csrc/host/groth16_vk.h"
#include "../../masp_amd/csrc/host/pairing.h"
#include "../../masp_amd/csrc/verify_launch.h"

using namespace masp;
namespace hb = masp_host::bls;

namespace {

Fp fp_of_be(const uint8_t* in) { return fe_to_mont(fe_load_be<FpCfg>(in)); }
void fp_to_be(const Fp& mont, uint8_t* out) { fe_store_be(fe_from_mont(mont), out); }

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
    int finish() {
        if (!ok) return -2;
        if (hipStreamSynchronize(s) != hipSuccess) return -3;
        if (launch_status() != MASP_HIP_OK || hipGetLastError() != hipSuccess) return -4;
        return 0;
    }
};

}  // namespace

extern "C" {

// n values of 12 Fp -> their final exponentiations (zeros where the verdict is 0 for want of an inverse) and verdicts (1: the power is one)
int ve_final_exp_gpu(const uint8_t* vals, uint32_t n, uint8_t* out, uint8_t* verdict) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    const FinalExpTables ft = final_exp_tables();
    const uint32_t lds = ft.n_slots * 48;
    if (lds > 64 * 1024 || hipFuncSetAttribute((const void*)k_final_exp, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) != hipSuccess) return -5;
    std::vector<Fp> hf(12 * (size_t)n);
    for (size_t i = 0; i < hf.size(); ++i) hf[i] = fp_of_be(vals + 48 * i);
    Scope sc;
    const uint32_t* d_ops = sc.upload(ft.ops.data(), ft.ops.size());
    const uint32_t* d_steps = sc.upload(ft.steps.data(), ft.steps.size());
    const uint32_t* d_sched = sc.upload(ft.sched.data(), ft.sched.size());
    const Fp* d_consts = sc.upload(ft.consts, 15);
    const Fp* d_f = sc.upload(hf.data(), hf.size());
    Fp* d_out = sc.alloc<Fp>(12 * (size_t)n);
    uint8_t* d_verdict = sc.alloc<uint8_t>(n);
    if (!sc.ok) return -1;
    PairingProgramDev progs[6];
    for (int i = 0; i < 6; ++i) progs[i] = ft.dev(i, d_ops, d_steps);
    const PairingProgramDev* d_progs = sc.upload(progs, 6);
    if (!sc.ok) return -1;
    const FinalExpDev fe = {d_progs, d_sched, (uint32_t)ft.sched.size(), ft.n_slots, d_consts};
    MASP_LAUNCH(k_final_exp, dim3(n), dim3(64), lds, sc.s, fe, d_f, 1u, (const Fp*)nullptr, (const uint8_t*)nullptr, d_out, d_verdict);
    sc.download(hf.data(), d_out, hf.size());
    sc.download(verdict, d_verdict, n);
    const int rc = sc.finish();
    if (rc) return rc;
    for (size_t i = 0; i < hf.size(); ++i) fp_to_be(hf[i], out + 48 * i);
    return 0;
}

// ic: (n_public + 1) x 96 (IC_0 .. IC_n_public); inputs: n x n_public x 32 little-endian; status: n ints as k_verify_decode leaves them
// -> neg_acc: n x 96, -(IC_0 + sum_j x_ij IC_j) (the identity where pre is not 0), pre: n bytes
int ve_acc_gpu(const uint8_t* ic96, uint32_t n_public, const uint8_t* inputs, const int* status, uint32_t n, uint8_t* neg_acc, uint8_t* pre) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    masp_host::PreparedVk vk;
    vk.ic.resize(n_public + 1);
    for (uint32_t j = 0; j <= n_public; ++j)
        if (!hb::g1_uncompressed(vk.ic[j], ic96 + 96 * (size_t)j)) return -1;
    vk.build_tables();
    const std::vector<G1Affine> ic = ic_table(vk);
    Scope sc;
    const G1Affine* d_ic = sc.upload(ic.data(), ic.size());
    const uint8_t* d_inputs = sc.upload(inputs, 32 * (size_t)n_public * n);
    const int* d_status = sc.upload(status, n);
    G1Affine* d_pp = sc.alloc<G1Affine>(3 * (size_t)n);
    uint8_t* d_pre = sc.alloc<uint8_t>(n);
    if (!sc.ok) return -1;
    MASP_LAUNCH(k_verify_acc, dim3((n + 63) / 64), dim3(64), 0, sc.s, d_inputs, n, n_public, d_ic, d_ic + 1, d_status, d_pp, d_pre);
    std::vector<G1Affine> hp(3 * (size_t)n);
    sc.download(hp.data(), d_pp, hp.size());
    sc.download(pre, d_pre, n);
    const int rc = sc.finish();
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) g1_write_uncompressed(hp[3 * (size_t)i + 1], neg_acc + 96 * (size_t)i);
    return 0;
}

// ---- host/pairing.h, no GPU ----
// f^(3 (p^12 - 1) / r) by bls::final_exp; -1 if a coefficient is not canonical
int ve_final_exp_host(const uint8_t* in, uint8_t* out) {
    hb::Fp12 f;
    hb::Fp* c = &f.a.a.a;
    for (int i = 0; i < 12; ++i)
        if (!hb::Fp::from_be(c[i], in + 48 * i)) return -1;
    const hb::Fp12 r = hb::final_exp(f);
    const hb::Fp* g = &r.a.a.a;
    for (int i = 0; i < 12; ++i) {
        uint64_t v[6];
        g[i].canon(v);
        for (int k = 0; k < 48; ++k) out[48 * i + k] = (uint8_t)(v[5 - k / 8] >> (8 * (7 - k % 8)));
    }
    return 0;
}

}  // extern "C"
