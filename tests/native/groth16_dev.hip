// Test-only unit over the proof-assembly kernels (masp_amd/csrc/device/groth16.hpp): the product's translation unit k_groth16.hip is
// included whole, so the kernels and their launch_* wrappers are the product's, and every entry point below launches ONE of them on
// inputs the test sets directly (tests/test_gpu_groth16_stages.py).  g16_fixed_g1 / _g2 first build the tables they read with
// launch_fixed_table_*, as the loader does; the tables have entry points of their own.
// Everything that crosses this boundary is canonical bytes: G1 96 and G2 192 bytes of bellman uncompressed form (the identity 0x40 then
// zeros), scalars 32 bytes little-endian, Fp 48 bytes big-endian.  An input that stands for an MSM result or an assembly piece comes with
// a z (Fp for G1; c0 | c1 for G2, never zero) and is uploaded as (x z^2, y z^3, z^2, z^3): such values are never normalised in the
// product.  The identity is uploaded as the all-zero struct.  Results go back as affine bytes, so they are compared as group elements.
// Every buffer a kernel writes is filled with the byte 0xA5 beforehand and has poisoned slots behind its end; for every XYZZ slot that
// comes back there is a state byte: 0 converted, 1 still the poison, 2 neither (a coordinate that is no reduced residue: not converted).
// Every _gpu-side function returns non-zero on a HIP error and synchronises its stream exactly once.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/k_groth16.hip"

using namespace masp;

namespace {

constexpr int POISON = 0xA5;
constexpr uint32_t TAB = 32 * 255;  // entries of one fixed-base table
constexpr uint32_t GUARD = 6;       // poisoned XYZZ slots behind the end of part / part2 / a table

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

// ---- wire bytes -> what the kernels read ----
__device__ void note_status(int st, int* status) {
    if (st & ~PT_INFINITY) atomicOr(status, st);
}
// affine points `stride` bytes apart (the verifying key's members, the bases of the tables, the rows k_g1_subgroup_flag walks)
__global__ void __launch_bounds__(64) k_g16_g1_affine_in(const uint8_t* __restrict__ raw, uint32_t n, uint8_t* __restrict__ out, size_t stride, int* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine a;
    note_status(g1_read_uncompressed(raw + 96 * (size_t)i, a), status);
    *reinterpret_cast<G1Affine*>(out + (size_t)i * stride) = a;
}
__global__ void __launch_bounds__(64) k_g16_g2_affine_in(const uint8_t* __restrict__ raw, uint32_t n, G2Affine* __restrict__ out, int* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G2Affine a;
    note_status(g2_read_uncompressed(raw + 192 * (size_t)i, a), status);
    out[i] = a;
}
// (x z^2, y z^3, z^2, z^3); the identity as the all-zero struct
__global__ void __launch_bounds__(64) k_g16_g1_in(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ z, uint32_t n, G1Xyzz* __restrict__ out, int* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine a;
    note_status(g1_read_uncompressed(raw + 96 * (size_t)i, a), status);
    G1Xyzz p = xyzz_from_affine(a);
    if (!xyzz_is_inf(p)) {
        const Fp zc = fe_load_be<FpCfg>(z + 48 * (size_t)i);
        if (fe_is_zero(zc) || fe_canonical_ge_mod(zc)) atomicOr(status, PT_NOT_CANONICAL);
        const Fp zm = fe_to_mont(zc);
        p.ZZ = fe_sqr_nc(zm);
        p.ZZZ = fe_mul_nc(p.ZZ, zm);
        p.X = fe_mul_nc(a.x, p.ZZ);
        p.Y = fe_mul_nc(a.y, p.ZZZ);
    }
    out[i] = p;
}
__global__ void __launch_bounds__(64) k_g16_g2_in(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ z, uint32_t n, G2Xyzz* __restrict__ out, int* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G2Affine a;
    note_status(g2_read_uncompressed(raw + 192 * (size_t)i, a), status);
    G2Xyzz p = xyzz_from_affine(a);
    if (!xyzz_is_inf(p)) {
        const Fp z0 = fe_load_be<FpCfg>(z + 96 * (size_t)i), z1 = fe_load_be<FpCfg>(z + 96 * (size_t)i + 48);
        if ((fe_is_zero(z0) && fe_is_zero(z1)) || fe_canonical_ge_mod(z0) || fe_canonical_ge_mod(z1)) atomicOr(status, PT_NOT_CANONICAL);
        const Fp2 zm = {fe_to_mont(z0), fe_to_mont(z1)};
        p.ZZ = Fp2Ops::sqr(zm);
        p.ZZZ = Fp2Ops::mul(p.ZZ, zm);
        p.X = Fp2Ops::mul(a.x, p.ZZ);
        p.Y = Fp2Ops::mul(a.y, p.ZZZ);
    }
    out[i] = p;
}

// ---- what the kernels left -> wire bytes + a state byte per slot ----
// 1: every byte is the poison; 2: a word that is no limb of a reduced residue; 0: a point to convert
template <class X>
__device__ int slot_state(const X& p) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&p);
    bool all_poison = true;
    for (uint32_t k = 0; k < sizeof(X) / 4; ++k) all_poison = all_poison && w[k] == 0xA5A5A5A5u;
    if (all_poison) return 1;
    const Fp* f = reinterpret_cast<const Fp*>(&p);
    for (uint32_t k = 0; k < sizeof(X) / sizeof(Fp); ++k)
        if (fe_canonical_ge_mod(f[k])) return 2;
    return 0;
}
__global__ void __launch_bounds__(64) k_g16_g1_out(const G1Xyzz* __restrict__ p, uint32_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Xyzz v = p[i];
    const int st = slot_state(v);
    state[i] = (uint8_t)st;
    if (st == 0)
        g1_write_uncompressed(xyzz_to_affine(v), out + 96 * (size_t)i);
    else
        for (int k = 0; k < 96; ++k) out[96 * (size_t)i + k] = 0;
}
__global__ void __launch_bounds__(64) k_g16_g2_out(const G2Xyzz* __restrict__ p, uint32_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G2Xyzz v = p[i];
    const int st = slot_state(v);
    state[i] = (uint8_t)st;
    if (st == 0)
        g2_write_uncompressed(xyzz_to_affine(v), out + 192 * (size_t)i);
    else
        for (int k = 0; k < 192; ++k) out[192 * (size_t)i + k] = 0;
}
// one lane per scalar through the product's endo_split
__global__ void __launch_bounds__(64) k_g16_endo_split(const uint8_t* __restrict__ k32, uint32_t n, uint8_t* __restrict__ q16, uint8_t* __restrict__ rem16) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr k = fe_load_le<FrCfg>(k32 + 32 * (size_t)i);
    uint32_t q[4], rem[4];
    endo_split(k.v, q, rem);
    for (int j = 0; j < 16; ++j) {
        q16[16 * (size_t)i + j] = (uint8_t)(q[j >> 2] >> (8 * (j & 3)));
        rem16[16 * (size_t)i + j] = (uint8_t)(rem[j >> 2] >> (8 * (j & 3)));
    }
}

dim3 lanes(uint32_t n) { return dim3((n + 63) / 64); }

G1Xyzz* g1_in(Scope& sc, const uint8_t* raw, const uint8_t* z, uint32_t n, size_t slots, int* d_status) {
    G1Xyzz* d = sc.poisoned<G1Xyzz>(slots);
    const uint8_t* d_raw = sc.upload(raw, 96 * (size_t)n);
    const uint8_t* d_z = sc.upload(z, 48 * (size_t)n);
    if (sc.ok && n) MASP_LAUNCH(k_g16_g1_in, lanes(n), dim3(64), 0, sc.s, d_raw, d_z, n, d, d_status);
    return d;
}
G2Xyzz* g2_in(Scope& sc, const uint8_t* raw, const uint8_t* z, uint32_t n, size_t slots, int* d_status) {
    G2Xyzz* d = sc.poisoned<G2Xyzz>(slots);
    const uint8_t* d_raw = sc.upload(raw, 192 * (size_t)n);
    const uint8_t* d_z = sc.upload(z, 96 * (size_t)n);
    if (sc.ok && n) MASP_LAUNCH(k_g16_g2_in, lanes(n), dim3(64), 0, sc.s, d_raw, d_z, n, d, d_status);
    return d;
}
// n affine G1 points back to back
G1Affine* g1_affine_in(Scope& sc, const uint8_t* raw, uint32_t n, int* d_status) {
    G1Affine* d = sc.poisoned<G1Affine>(n);
    const uint8_t* d_raw = sc.upload(raw, 96 * (size_t)n);
    if (sc.ok && n) MASP_LAUNCH(k_g16_g1_affine_in, lanes(n), dim3(64), 0, sc.s, d_raw, n, reinterpret_cast<uint8_t*>(d), sizeof(G1Affine), d_status);
    return d;
}
G2Affine* g2_affine_in(Scope& sc, const uint8_t* raw, uint32_t n, int* d_status) {
    G2Affine* d = sc.poisoned<G2Affine>(n);
    const uint8_t* d_raw = sc.upload(raw, 192 * (size_t)n);
    if (sc.ok && n) MASP_LAUNCH(k_g16_g2_affine_in, lanes(n), dim3(64), 0, sc.s, d_raw, n, d, d_status);
    return d;
}
int* status_word(Scope& sc) {
    int* d = sc.alloc<int>(1);
    if (d && hipMemsetAsync(d, 0, sizeof(int), sc.s) != hipSuccess) sc.ok = false;
    return d;
}
void g1_out(Scope& sc, const G1Xyzz* d, uint32_t n, uint8_t* out, uint8_t* state) {
    uint8_t* d_out = sc.alloc<uint8_t>(96 * (size_t)n);
    uint8_t* d_state = sc.alloc<uint8_t>(n);
    if (!sc.ok) return;
    MASP_LAUNCH(k_g16_g1_out, lanes(n), dim3(64), 0, sc.s, d, n, d_out, d_state);
    sc.download(out, d_out, 96 * (size_t)n);
    sc.download(state, d_state, n);
}
void g2_out(Scope& sc, const G2Xyzz* d, uint32_t n, uint8_t* out, uint8_t* state) {
    uint8_t* d_out = sc.alloc<uint8_t>(192 * (size_t)n);
    uint8_t* d_state = sc.alloc<uint8_t>(n);
    if (!sc.ok) return;
    MASP_LAUNCH(k_g16_g2_out, lanes(n), dim3(64), 0, sc.s, d, n, d_out, d_state);
    sc.download(out, d_out, 192 * (size_t)n);
    sc.download(state, d_state, n);
}
// finish() and then the verdict of the input conversions: -6 if a point or a z was not canonical
int finish_checked(Scope& sc, const int* d_status) {
    int st = 0;
    sc.download(&st, d_status, 1);
    const int rc = sc.finish();
    return rc ? rc : st ? -6 : 0;
}

}  // namespace

extern "C" {

uint32_t g16_guard_slots(void) { return GUARD; }
// the distance of the rows k_g1_subgroup_flag walks in the loader (Circuit::a / b1 tables)
uint32_t g16_tab_row_stride(void) { return (uint32_t)sizeof(TabRow<FpOps>); }

// k_fixed_table_xyzz<FpOps>: npts bases -> npts tables of 32 x 255 entries + GUARD slots, as affine bytes and state bytes
int g16_fixed_table_g1(const uint8_t* pts96, uint32_t npts, uint8_t* out96, uint8_t* state) {
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    const G1Affine* d_pts = g1_affine_in(sc, pts96, npts, d_status);
    const uint32_t slots = npts * TAB + GUARD;
    G1Xyzz* d_tabs = sc.poisoned<G1Xyzz>(slots);
    if (!sc.ok) return -1;
    launch_fixed_table_g1(sc.s, d_pts, d_tabs, npts);
    g1_out(sc, d_tabs, slots, out96, state);
    return finish_checked(sc, d_status);
}
int g16_fixed_table_g2(const uint8_t* pts192, uint32_t npts, uint8_t* out192, uint8_t* state) {
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    const G2Affine* d_pts = g2_affine_in(sc, pts192, npts, d_status);
    const uint32_t slots = npts * TAB + GUARD;
    G2Xyzz* d_tabs = sc.poisoned<G2Xyzz>(slots);
    if (!sc.ok) return -1;
    launch_fixed_table_g2(sc.s, d_pts, d_tabs, npts);
    g2_out(sc, d_tabs, slots, out192, state);
    return finish_checked(sc, d_status);
}

// k_groth16_fixed_g1 over the tables of pts96 = delta1 | alpha1 | beta1; rs: np rows of rs_stride words (r in words 0..7, s in 8..15)
// -> part (6 np + GUARD slots)
int g16_fixed_g1(const uint8_t* pts96, const uint8_t* rs, uint32_t rs_stride, uint32_t np, uint8_t* out96, uint8_t* state) {
    if (np == 0 || rs_stride < 16) return -1;
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    const G1Affine* d_pts = g1_affine_in(sc, pts96, 3, d_status);
    G1Xyzz* d_tabs = sc.poisoned<G1Xyzz>(3 * (size_t)TAB);
    const uint32_t* d_rs = reinterpret_cast<const uint32_t*>(sc.upload(rs, 4 * (size_t)rs_stride * np));
    const uint32_t slots = 6 * np + GUARD;
    G1Xyzz* d_part = sc.poisoned<G1Xyzz>(slots);
    if (!sc.ok) return -1;
    launch_fixed_table_g1(sc.s, d_pts, d_tabs, 3);
    launch_groth16_fixed_g1(sc.s, d_tabs, d_rs, rs_stride, d_part, np);
    g1_out(sc, d_part, slots, out96, state);
    return finish_checked(sc, d_status);
}
// k_groth16_fixed_g2 over the table of pt192 = delta2 -> part2 (np + GUARD slots)
int g16_fixed_g2(const uint8_t* pt192, const uint8_t* rs, uint32_t rs_stride, uint32_t np, uint8_t* out192, uint8_t* state) {
    if (np == 0 || rs_stride < 16) return -1;
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    const G2Affine* d_pt = g2_affine_in(sc, pt192, 1, d_status);
    G2Xyzz* d_tab = sc.poisoned<G2Xyzz>(TAB);
    const uint32_t* d_rs = reinterpret_cast<const uint32_t*>(sc.upload(rs, 4 * (size_t)rs_stride * np));
    const uint32_t slots = np + GUARD;
    G2Xyzz* d_part2 = sc.poisoned<G2Xyzz>(slots);
    if (!sc.ok) return -1;
    launch_fixed_table_g2(sc.s, d_pt, d_tab, 1);
    launch_groth16_fixed_g2(sc.s, d_tab, d_rs, rs_stride, d_part2, np);
    g2_out(sc, d_part2, slots, out192, state);
    return finish_checked(sc, d_status);
}

// n scalars of 32 bytes -> q and rem of 16 bytes each, little-endian (the product's endo_split, one lane per scalar)
int g16_endo_split(const uint8_t* k32, uint32_t n, uint8_t* q16, uint8_t* rem16) {
    if (n == 0) return 0;
    const ApiLaunchScope api_scope;
    Scope sc;
    const uint8_t* d_k = sc.upload(k32, 32 * (size_t)n);
    uint8_t* d_q = sc.poisoned<uint8_t>(16 * (size_t)n);
    uint8_t* d_rem = sc.poisoned<uint8_t>(16 * (size_t)n);
    if (!sc.ok) return -1;
    MASP_LAUNCH(k_g16_endo_split, lanes(n), dim3(64), 0, sc.s, d_k, n, d_q, d_rem);
    sc.download(q16, d_q, 16 * (size_t)n);
    sc.download(rem16, d_rem, 16 * (size_t)n);
    return sc.finish();
}

// k_groth16_var_mul: msm96 / z48 = 4 np slots H, L, A, B1 -> part (6 np + GUARD slots)
int g16_var_mul(int which, const uint8_t* msm96, const uint8_t* z48, const uint8_t* rs, uint32_t rs_stride, uint32_t np, int endo, uint8_t* out96,
                uint8_t* state) {
    if (np == 0 || rs_stride < 16 || which < 0 || which > 2) return -1;
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    const G1Xyzz* d_msm = g1_in(sc, msm96, z48, 4 * np, 4 * (size_t)np, d_status);
    const uint32_t* d_rs = reinterpret_cast<const uint32_t*>(sc.upload(rs, 4 * (size_t)rs_stride * np));
    const uint32_t slots = 6 * np + GUARD;
    G1Xyzz* d_part = sc.poisoned<G1Xyzz>(slots);
    if (!sc.ok) return -1;
    launch_groth16_var_mul(sc.s, which, d_msm, d_rs, rs_stride, d_part, np, endo != 0);
    g1_out(sc, d_part, slots, out96, state);
    return finish_checked(sc, d_status);
}

// k_g1_subgroup_flag over n affine points stride_bytes apart (0: n = 1, the loader's form for a member of the verifying key); the flag
// holds flag_in beforehand
int g16_subgroup_flag(const uint8_t* pts96, uint32_t n, uint32_t stride_bytes, int flag_in, int* flag_out) {
    if ((stride_bytes == 0 && n > 1) || (stride_bytes != 0 && stride_bytes < sizeof(G1Affine)) || stride_bytes % 4) return -1;
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    uint8_t* d_rows = sc.poisoned<uint8_t>((size_t)stride_bytes * n + sizeof(G1Affine));
    const uint8_t* d_raw = sc.upload(pts96, 96 * (size_t)n);
    int* d_flag = sc.upload(&flag_in, 1);
    if (!sc.ok) return -1;
    if (n) MASP_LAUNCH(k_g16_g1_affine_in, lanes(n), dim3(64), 0, sc.s, d_raw, n, d_rows, (size_t)stride_bytes, d_status);
    launch_g1_subgroup_flag(sc.s, d_rows, stride_bytes, n, d_flag);
    sc.download(flag_out, d_flag, 1);
    return finish_checked(sc, d_status);
}

// The four finishing kernels on one set of inputs.  mode 0: k_groth16_finish_b, 1: _finish_ac, 2: _finish_ac_early, 3: _finish_c_late.
// vk: alpha_g1 and beta_g2 (its other members hold the poison: no finishing kernel reads them); part: 6 np slots, part2: np, msm1: 4 np
// (H, L, A, B1), msm2: np (B2), each with its z.  -> the proof bytes (192 (np + 1): one proof's worth of poison behind the end) and part
// as the kernel left it (6 np + GUARD slots).
int g16_finish(int mode, const uint8_t* alpha96, const uint8_t* beta2_192, const uint8_t* part96, const uint8_t* part_z, const uint8_t* part2_192,
               const uint8_t* part2_z, const uint8_t* msm1_96, const uint8_t* msm1_z, const uint8_t* msm2_192, const uint8_t* msm2_z, uint32_t np,
               uint8_t* proof, uint8_t* part_out96, uint8_t* part_state) {
    if (np == 0 || mode < 0 || mode > 3) return -1;
    const ApiLaunchScope api_scope;
    Scope sc;
    int* d_status = status_word(sc);
    VkDevice* d_vk = sc.poisoned<VkDevice>(1);
    const uint8_t* d_alpha = sc.upload(alpha96, 96);
    const uint8_t* d_beta2 = sc.upload(beta2_192, 192);
    const uint32_t slots = 6 * np + GUARD;
    G1Xyzz* d_part = g1_in(sc, part96, part_z, 6 * np, slots, d_status);
    const G2Xyzz* d_part2 = g2_in(sc, part2_192, part2_z, np, np, d_status);
    const G1Xyzz* d_msm1 = g1_in(sc, msm1_96, msm1_z, 4 * np, 4 * (size_t)np, d_status);
    const G2Xyzz* d_msm2 = g2_in(sc, msm2_192, msm2_z, np, np, d_status);
    uint8_t* d_proof = sc.poisoned<uint8_t>(192 * ((size_t)np + 1));
    if (!sc.ok) return -1;
    MASP_LAUNCH(k_g16_g1_affine_in, dim3(1), dim3(64), 0, sc.s, d_alpha, 1u, reinterpret_cast<uint8_t*>(&d_vk->alpha_g1), sizeof(G1Affine), d_status);
    MASP_LAUNCH(k_g16_g2_affine_in, dim3(1), dim3(64), 0, sc.s, d_beta2, 1u, &d_vk->beta_g2, d_status);
    if (mode == 0)
        launch_groth16_finish_b(sc.s, d_vk, d_part2, d_msm2, d_proof, np);
    else if (mode == 1)
        launch_groth16_finish_ac(sc.s, d_vk, d_part, d_msm1, d_proof, np);
    else if (mode == 2)
        launch_groth16_finish_ac_early(sc.s, d_vk, d_part, d_msm1, d_proof, np);
    else
        launch_groth16_finish_c_late(sc.s, d_part, d_msm1, d_proof, np);
    sc.download(proof, d_proof, 192 * ((size_t)np + 1));
    g1_out(sc, d_part, slots, part_out96, part_state);
    return finish_checked(sc, d_status);
}

}  // extern "C"
