// TEST-ONLY shim: compiles masp_amd/csrc/device/{field,curve,io}.hpp for the *host* so the exact
// source the HIP kernels use can be checked on a machine without a GPU (tests/test_device_math_host.py), and runs the
// device-only forms (lane pairs, quads, octs, the register-argument calls, the batch inversion) on the GPU
// (tests/test_device_ops.py).  Built with the product's flags (tests/device_shim.py).  It is never part of the product library.
#include <vector>

#include "../../masp_amd/csrc/device/io.hpp"
#include "../../masp_amd/csrc/device/oct.hpp"
#include "../../masp_amd/csrc/device/msm_tree.hpp"
#include "../../tools/fp28.hpp"   // (an experiment kept with its checks: see the header)
using namespace masp;

// ---- the same field functions ON THE DEVICE (their device overloads are hand-written carry chains / inline asm that the host
// build above never compiles): n lanes, lane i computes op(a_i, b_i).  op: 0 add 1 sub 2 mul 4 neg 5 sqr 8 dbl.  Returns 0, or a
// HIP error code.
template <class C>
__global__ void k_field_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = 4 * C::N;
    if (op >= 16) {
        // RAW limbs in, raw limbs out (Fp only): the Montgomery products on operands anywhere in [0, 2p) — what the lazily
        // reduced chains of the bucket tree feed them, and the shapes that stress the carry-free top-limb terms (field.hpp,
        // MASP_MACNC).  16 mul, 17 mul_lazy (left in [0, 2p)), 18 sqr, 19 mul2(a, b, b, a), 20 mul_lazy(mul_lazy(a, b), b)
        if constexpr (C::N == 12) {
            const Fe<C> x = fe_load_le<C>(a + (size_t)B * i), y = fe_load_le<C>(b + (size_t)B * i);
            Fe<C> r;
            switch (op) {
                case 16: r = fe_mul(x, y); break;
                case 17: r = fe_mul_lazy(x, y); break;
                case 18: r = fe_sqr(x); break;
                case 19: r = fe_mul2(x, y, y, x); break;
                default: r = fe_mul_lazy(fe_mul_lazy(x, y), y);
            }
            fe_store_le(r, out + (size_t)B * i);
        }
        return;
    }
    Fe<C> x = fe_to_mont(fe_load_le<C>(a + (size_t)B * i)), y = fe_to_mont(fe_load_le<C>(b + (size_t)B * i)), r;
    switch (op) {
        case 0: r = fe_add(x, y); break;
        case 1: r = fe_sub(x, y); break;
        case 2: r = fe_mul(x, y); break;
        case 4: r = fe_neg(x); break;
        case 8: r = fe_dbl(x); break;
        default: r = fe_sqr(x);
    }
    fe_store_le(fe_from_mont(r), out + (size_t)B * i);
}

// ---- the 28-bit-limb form (device/fp28.hpp): raw limbs in and out, 56 bytes per element (an Fp operand / result uses the first
// 48).  op: 0 mul 1 sqr 2 canon 3 sub_lazy 4 neg 5 from_fp 6 from_fp_lazy 7 to_fp 8 Ops::add 9 Ops::sub 10 Ops::dbl
// 11 canon(sub_lazy(sub_lazy(sqr(a), b), b)) 12 is_zero(a) | eq(a, b) << 1
MASP_HD void fp28_test_op(int op, const uint8_t* pa, const uint8_t* pb, uint8_t* po) {
    F28 a, b, r = fp28_zero();
    Fp fa, fr;
    for (int i = 0; i < 14; ++i) {
        a.v[i] = (uint32_t)pa[4 * i] | (uint32_t)pa[4 * i + 1] << 8 | (uint32_t)pa[4 * i + 2] << 16 | (uint32_t)pa[4 * i + 3] << 24;
        b.v[i] = (uint32_t)pb[4 * i] | (uint32_t)pb[4 * i + 1] << 8 | (uint32_t)pb[4 * i + 2] << 16 | (uint32_t)pb[4 * i + 3] << 24;
    }
    for (int i = 0; i < 12; ++i) fa.v[i] = a.v[i];
    bool is_fp = false;
    switch (op) {
        case 0: r = fp28_mul(a, b); break;
        case 1: r = fp28_sqr(a); break;
        case 2: r = fp28_canon(a); break;
        case 3: r = fp28_sub_lazy(a, b); break;
        case 4: r = fp28_neg(a); break;
        case 5: r = fp28_from_fp(fa); break;
        case 6: r = fp28_from_fp_lazy(fa); break;
        case 7: fr = fp28_to_fp(a); is_fp = true; break;
        case 8: r = Fp28Ops::add(a, b); break;
        case 9: r = Fp28Ops::sub(a, b); break;
        case 10: r = Fp28Ops::dbl(a); break;
        case 11: r = fp28_canon(fp28_sub_lazy(fp28_sub_lazy(fp28_sqr(a), b), b)); break;
        default: r.v[0] = (fp28_is_zero(a) ? 1u : 0u) | (fp28_eq(a, b) ? 2u : 0u); break;
    }
    if (is_fp) {
        for (int i = 0; i < 12; ++i) r.v[i] = fr.v[i];
        r.v[12] = r.v[13] = 0;
    }
    for (int i = 0; i < 14; ++i)
        for (int k = 0; k < 4; ++k) po[4 * i + k] = (uint8_t)(r.v[i] >> (8 * k));
}
__global__ void k_fp28_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fp28_test_op(op, a + 56 * (size_t)i, b + 56 * (size_t)i, out + 56 * (size_t)i);
}

// ---- checked device runs: every HIP call checked, the first error code returned, every buffer freed on every path ----------
struct DevRun {
    int err = 0;
    std::vector<void*> bufs;
    ~DevRun() {
        for (void* p : bufs) (void)hipFree(p);
    }
    void check(hipError_t e) {
        if (e != hipSuccess && !err) err = (int)e;
    }
    bool ok() const { return err == 0; }
    // zero-filled device buffer of `bytes`
    template <class T = uint8_t>
    T* alloc(size_t bytes) {
        void* p = nullptr;
        if (err) return nullptr;
        check(hipMalloc(&p, bytes ? bytes : 1));
        if (err) return nullptr;
        bufs.push_back(p);
        check(hipMemset(p, 0, bytes ? bytes : 1));
        return (T*)p;
    }
    // `bytes` from the host into a zero-filled buffer of max(bytes, cap)
    template <class T = uint8_t>
    T* up(const void* h, size_t bytes, size_t cap = 0) {
        T* p = alloc<T>(cap > bytes ? cap : bytes);
        if (!err && bytes) check(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
        return p;
    }
    void launched() { check(hipGetLastError()); }
    int back(void* h, const void* d, size_t bytes) {
        if (!err) check(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
        check(hipGetLastError());
        return err;
    }
};

extern "C" {
// op: 0 add 1 sub 2 mul 3 inv 4 neg 5 sqr 6 inv (binary gcd) 7 inv (Fermat); canonical little-endian in/out; which: 0 Fp (48 B), 1 Fr (32 B)
int mh_field_op(int which, int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    if (which == 0) {
        Fp x = fe_to_mont(fe_load_le<FpCfg>(a)), y = fe_to_mont(fe_load_le<FpCfg>(b)), r;
        switch (op) {
            case 0: r = fe_add(x, y); break;
            case 1: r = fe_sub(x, y); break;
            case 2: r = fe_mul(x, y); break;
            case 3: r = fe_inv(x); break;
            case 4: r = fe_neg(x); break;
            case 6: r = fe_inv_bingcd(x); break;
            case 7: r = fe_inv_fermat(x); break;
            default: r = fe_sqr(x);
        }
        fe_store_le(fe_from_mont(r), out);
    } else {
        Fr x = fe_to_mont(fe_load_le<FrCfg>(a)), y = fe_to_mont(fe_load_le<FrCfg>(b)), r;
        switch (op) {
            case 0: r = fe_add(x, y); break;
            case 1: r = fe_sub(x, y); break;
            case 2: r = fe_mul(x, y); break;
            case 3: r = fe_inv(x); break;
            case 4: r = fe_neg(x); break;
            case 6: r = fe_inv_bingcd(x); break;
            case 7: r = fe_inv_fermat(x); break;
            default: r = fe_sqr(x);
        }
        fe_store_le(fe_from_mont(r), out);
    }
    return 0;
}
// sum_i [k_i] P_i with the XYZZ formulas; mode 0: scalar-mul each then xyzz_add; mode 1: signed madd chain
// (k_i interpreted as small counts: adds P_i k_i[0] times, negated if k_i[1] != 0)
int mh_g1_lincomb(const uint8_t* pts96, const uint8_t* scalars32, int n, int mode, uint8_t* out96, uint8_t* out48) {
    G1Xyzz acc = xyzz_inf<FpOps>();
    for (int i = 0; i < n; ++i) {
        G1Affine p;
        int st = g1_read_uncompressed(pts96 + 96 * i, p);
        if (st & ~PT_INFINITY) return -1;
        if (mode == 0) {
            Fr k = fe_load_le<FrCfg>(scalars32 + 32 * i);
            G1Xyzz t = xyzz_mul_scalar(xyzz_from_affine(p), k.v);
            xyzz_add(acc, t);
        } else {
            int cnt = scalars32[32 * i];
            bool neg = scalars32[32 * i + 1] != 0;
            for (int c = 0; c < cnt; ++c) xyzz_madd(acc, p, neg);
        }
    }
    G1Affine r = xyzz_to_affine(acc);
    g1_write_uncompressed(r, out96);
    g1_write_compressed(r, out48);
    return 0;
}
int mh_g2_lincomb(const uint8_t* pts192, const uint8_t* scalars32, int n, int mode, uint8_t* out192, uint8_t* out96) {
    G2Xyzz acc = xyzz_inf<Fp2Ops>();
    for (int i = 0; i < n; ++i) {
        G2Affine p;
        int st = g2_read_uncompressed(pts192 + 192 * i, p);
        if (st & ~PT_INFINITY) return -1;
        if (mode == 0) {
            Fr k = fe_load_le<FrCfg>(scalars32 + 32 * i);
            G2Xyzz t = xyzz_mul_scalar(xyzz_from_affine(p), k.v);
            xyzz_add(acc, t);
        } else {
            int cnt = scalars32[32 * i];
            bool neg = scalars32[32 * i + 1] != 0;
            for (int c = 0; c < cnt; ++c) xyzz_madd(acc, p, neg);
        }
    }
    G2Affine r = xyzz_to_affine(acc);
    g2_write_uncompressed(r, out192);
    g2_write_compressed(r, out96);
    return 0;
}

int mh_field_ops_gpu(int which, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const size_t bytes = (size_t)(which == 0 ? 48 : 32) * n;
    DevRun d;
    const uint8_t *da = d.up(a, bytes), *db = d.up(b, bytes);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    if (which == 0)
        hipLaunchKernelGGL((k_field_ops<FpCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, n);
    else
        hipLaunchKernelGGL((k_field_ops<FrCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, n);
    d.launched();
    return d.back(out, dout, bytes);
}
int mh_fp28_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    for (int i = 0; i < n; ++i) fp28_test_op(op, a + 56 * (size_t)i, b + 56 * (size_t)i, out + 56 * (size_t)i);
    return 0;
}
int mh_fp28_ops_gpu(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const size_t bytes = (size_t)56 * n;
    DevRun d;
    const uint8_t *da = d.up(a, bytes), *db = d.up(b, bytes);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    hipLaunchKernelGGL(k_fp28_ops, dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, n);
    d.launched();
    return d.back(out, dout, bytes);
}
}

// ================================================================================================================================
// The layers above the base-field ops, op by op (tests/test_device_ops.py).  Canonical little-endian bytes in and out (Montgomery
// form inside), raw limbs where an op is lazy.  A stored Fp2 is c0 | c1 (96 bytes).  Each `*_op` below is the per-element body
// shared by the host loop and the device kernel; the lane-group kernels (pairs, quads, octs) run whole groups on inputs padded to
// whole waves and mask only the store.
// ================================================================================================================================
template <class C>
MASP_HD Fe<C> ld_m(const uint8_t* p) {
    return fe_to_mont(fe_load_le<C>(p));
}
template <class C>
MASP_HD void st_m(const Fe<C>& a, uint8_t* p) {
    fe_store_le(fe_from_mont(a), p);
}
MASP_HD void ld_t(Fp& r, const uint8_t* p) { r = ld_m<FpCfg>(p); }
MASP_HD void ld_t(Fp2& r, const uint8_t* p) {
    r.c0 = ld_m<FpCfg>(p);
    r.c1 = ld_m<FpCfg>(p + 48);
}
MASP_HD void st_t(const Fp& a, uint8_t* p) { st_m(a, p); }
MASP_HD void st_t(const Fp2& a, uint8_t* p) {
    st_m(a.c0, p);
    st_m(a.c1, p + 48);
}
static inline uint32_t pad_lanes(uint32_t lanes) { return (lanes + 255u) & ~255u; }   // whole waves for blocks of 64 and of 256

// ---- A. inversions and the power.  op: 0 fe_inv_bingcd 1 fe_inv_bingcd_nc 2 fe_inv 3 fe_inv_fermat 4 fe_pow(a, e[0 .. ne))
template <class C>
MASP_HD void inv_op(int op, const uint8_t* a, const uint32_t* e, int ne, uint8_t* out) {
    const Fe<C> x = ld_m<C>(a);
    Fe<C> r;
    switch (op) {
        case 0: r = fe_inv_bingcd(x); break;
        case 1: r = fe_inv_bingcd_nc(x); break;
        case 2: r = fe_inv(x); break;
        case 3: r = fe_inv_fermat(x); break;
        default: r = fe_pow(x, e, ne);
    }
    st_m(r, out);
}
template <class C>
__global__ void k_inv_ops(int op, const uint8_t* a, const uint32_t* e, int ne, uint8_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) inv_op<C>(op, a + 4 * C::N * (size_t)i, e, ne, out + 4 * C::N * (size_t)i);
}

// ---- B. the register-argument products, RAW limbs in and out.  op: 0 fe_mul_nc 1 fe_sqr_nc 2 fe_mul 3 fe_sqr 4 fe_mul_ref
template <class C>
__global__ void k_cold_products(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int B = 4 * C::N;
    const Fe<C> x = fe_load_le<C>(a + (size_t)B * i), y = fe_load_le<C>(b + (size_t)B * i);
    Fe<C> r;
    switch (op) {
        case 0: r = fe_mul_nc(x, y); break;
        case 1: r = fe_sqr_nc(x); break;
        case 2: r = fe_mul(x, y); break;
        case 3: r = fe_sqr(x); break;
        default: r = fe_mul_ref(x, y);
    }
    fe_store_le(r, out + (size_t)B * i);
}

// ---- C. Fp2Ops.  op: 0 add 1 sub 2 neg 3 dbl 4 mul 5 sqr 6 inv 7 inv_lone 8 inv_gcd 9 flags: is_zero(a) | eq(a, b) << 1 (raw word)
// 10 mul_lazy
MASP_HD void fp2_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    Fp2 x, y, r;
    ld_t(x, a);
    ld_t(y, b);
    switch (op) {
        case 0: r = Fp2Ops::add(x, y); break;
        case 1: r = Fp2Ops::sub(x, y); break;
        case 2: r = Fp2Ops::neg(x); break;
        case 3: r = Fp2Ops::dbl(x); break;
        case 4: r = Fp2Ops::mul(x, y); break;
        case 5: r = Fp2Ops::sqr(x); break;
        case 6: r = Fp2Ops::inv(x); break;
        case 7: r = Fp2Ops::inv_lone(x); break;
        case 8: r = Fp2Ops::inv_gcd(x); break;
        case 10: r = Fp2Ops::mul_lazy(x, y); break;
        default: {
            r = Fp2Ops::zero();
            r.c0.v[0] = (Fp2Ops::is_zero(x) ? 1u : 0u) | (Fp2Ops::eq(x, y) ? 2u : 0u);
            fe_store_le(r.c0, out);
            fe_store_le(r.c1, out + 48);
            return;
        }
    }
    st_t(r, out);
}
__global__ void k_fp2_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fp2_op(op, a + 96 * (size_t)i, b + 96 * (size_t)i, out + 96 * (size_t)i);
}
// Fp2PairOps / Fp2PairCold: lane 2 g + h holds half h of element g and stores its own half (48 bytes at lane * 48).
// op: 0 mul 1 mul_lazy 2 sqr 3 one 4 flags (raw word, as above) 5 inv_gcd 6 Fp2PairCold::mul 7 Fp2PairCold::sqr
__global__ void k_fp2pair_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, uint32_t n) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, g = lane >> 1, h = lane & 1u;
    const Fp x = ld_m<FpCfg>(a + 96 * (size_t)g + 48 * h), y = ld_m<FpCfg>(b + 96 * (size_t)g + 48 * h);
    Fp r;
    bool raw = false;
    switch (op) {
        case 0: r = Fp2PairOps::mul(x, y); break;
        case 1: r = Fp2PairOps::mul_lazy(x, y); break;
        case 2: r = Fp2PairOps::sqr(x); break;
        case 3: r = Fp2PairOps::one(); break;
        case 4: {
            const bool z = Fp2PairOps::is_zero(x), e = Fp2PairOps::eq(x, y);
            r = fe_zero<FpCfg>();
            r.v[0] = (z ? 1u : 0u) | (e ? 2u : 0u);
            raw = true;
            break;
        }
        case 5: r = Fp2PairOps::inv_gcd(x); break;
        case 6: r = Fp2PairCold::mul(x, y); break;
        default: r = Fp2PairCold::sqr(x);
    }
    if (g < n) {
        if (raw)
            fe_store_le(r, out + 48 * (size_t)lane);
        else
            st_m(r, out + 48 * (size_t)lane);
    }
}

// ---- D, E, F. the group law over a field-ops policy O.  A stored point is X | Y | ZZ | ZZZ (4 elements of the base field); lane
// part `part` of a group reads part `part` of every element.  b's X, Y double as the affine operand of the mixed forms.
// op: 0 xyzz_madd 1 xyzz_madd(negate) 2 xyzz_madd_nc 3 xyzz_madd_nc(negate) 4 xyzz_add 5 xyzz_add_nc 6 xyzz_dbl(acc)
// 7 xyzz_dbl_affine(b) 8 xyzz_to_affine<O, false>(acc) 9 xyzz_to_affine<O, true>(acc) (x, y in X, Y; ZZ = ZZZ = 0) 10 xyzz_mul_scalar(acc, k)
enum { PT_ALL = 0, PT_NO_AFFINE = 1, PT_COOP = 2 };   // the forms O has: every one / all but to_affine (no inversion) / 5, 6, 10
template <class O>
MASP_HD void pt_load(Xyzz<O>& p, const uint8_t* src, uint32_t part) {
    constexpr size_t EB = sizeof(typename O::Base::T), TB = sizeof(typename O::T);
    ld_t(p.X, src + 0 * EB + TB * part);
    ld_t(p.Y, src + 1 * EB + TB * part);
    ld_t(p.ZZ, src + 2 * EB + TB * part);
    ld_t(p.ZZZ, src + 3 * EB + TB * part);
}
template <class O>
MASP_HD void pt_store(const Xyzz<O>& p, uint8_t* dst) {
    constexpr size_t TB = sizeof(typename O::T);
    st_t(p.X, dst);
    st_t(p.Y, dst + TB);
    st_t(p.ZZ, dst + 2 * TB);
    st_t(p.ZZZ, dst + 3 * TB);
}
template <class O, int FORMS>
MASP_HD Xyzz<O> pt_op(int op, const Xyzz<O>& a, const Xyzz<O>& b, const uint8_t* k) {
    Xyzz<O> r = a;
    if (op == 5) {
        xyzz_add_nc(r, b);
    } else if (op == 6) {
        r = xyzz_dbl(a);
    } else if (op == 10) {
        const Fr s = fe_load_le<FrCfg>(k);
        r = xyzz_mul_scalar(a, s.v);
    } else if constexpr (FORMS != PT_COOP) {
        Affine<O> ba;
        ba.x = b.X;
        ba.y = b.Y;
        if (op <= 1) {
            xyzz_madd(r, ba, op == 1);
        } else if (op <= 3) {
            xyzz_madd_nc(r, ba, op == 3);
        } else if (op == 4) {
            xyzz_add(r, b);
        } else if (op == 7) {
            r = xyzz_dbl_affine(ba);
        } else if constexpr (FORMS == PT_ALL) {
            const Affine<O> t = op == 8 ? xyzz_to_affine<O, false>(a) : xyzz_to_affine<O, true>(a);
            r.X = t.x;
            r.Y = t.y;
            r.ZZ = O::zero();
            r.ZZZ = O::zero();
        }
    }
    return r;
}
// lane = group * O::LANES + lig stores its whole result (4 elements of its own part) at lane * 4 * sizeof(T): the pair forms store both
// halves, the replicated forms (quads, octs) every copy
template <class O, int FORMS>
__global__ void k_pt_ops(int op, const uint8_t* acc, const uint8_t* b, const uint8_t* k, uint8_t* out, uint32_t n) {
    constexpr size_t EB = sizeof(typename O::Base::T), TB = sizeof(typename O::T);
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, g = lane / O::LANES, part = lane % O::PARTS;
    Xyzz<O> pa, pb;
    pt_load(pa, acc + 4 * EB * (size_t)g, part);
    pt_load(pb, b + 4 * EB * (size_t)g, part);
    const Xyzz<O> r = pt_op<O, FORMS>(op, pa, pb, k + 32 * (size_t)g);
    if (g < n) pt_store(r, out + 4 * TB * (size_t)lane);
}

// ---- G. the grid-wide batch inversion as MsmTreeWs::batch_invert (msm_tree_impl.hpp) launches it, BINV_C / BINV_MID given
template <class O>
static int binv_run(const uint8_t* in, uint32_t n, uint32_t binv_c, uint32_t binv_mid, uint8_t* out) {
    typedef typename O::T F;
    constexpr uint32_t LN = O::LANES;
    const size_t bytes = (size_t)n * LN * sizeof(F);
    DevRun d;
    const F* din = d.up<F>(in, bytes);
    F *dout = d.alloc<F>(bytes), *bpre = d.alloc<F>(bytes), *btot = d.alloc<F>(bytes), *bitot = d.alloc<F>(bytes), *bpre2 = d.alloc<F>(bytes);
    if (!d.ok()) return d.err;
    if (n <= 4 * binv_mid) {
        const uint32_t M = std::min<uint32_t>(n, binv_mid);
        hipLaunchKernelGGL((k_binv_mid<O>), dim3((M * LN + 63) / 64), dim3(64), 0, 0, din, n, M, bpre, dout);
        d.launched();
    } else {
        const uint32_t M1 = (n + binv_c - 1) / binv_c, M2 = std::min<uint32_t>(M1, binv_mid);
        hipLaunchKernelGGL((k_binv_fwd<O>), dim3((M1 * LN + 255) / 256), dim3(256), 0, 0, din, n, M1, bpre, btot);
        d.launched();
        if (d.ok()) hipLaunchKernelGGL((k_binv_mid<O>), dim3((M2 * LN + 63) / 64), dim3(64), 0, 0, (const F*)btot, M1, M2, bpre2, bitot);
        d.launched();
        if (d.ok()) hipLaunchKernelGGL((k_binv_bwd<O>), dim3((M1 * LN + 255) / 256), dim3(256), 0, 0, din, n, M1, (const F*)bpre, (const F*)bitot, dout);
        d.launched();
    }
    return d.back(out, dout, bytes);
}

template <class O, int FORMS>
static int pt_run(int op, const uint8_t* acc, const uint8_t* b, const uint8_t* k, uint8_t* out, int n, int block) {
    constexpr size_t EB = sizeof(typename O::Base::T), TB = sizeof(typename O::T);
    const uint32_t lanes = pad_lanes((uint32_t)n * O::LANES), groups = lanes / O::LANES;
    const size_t pts = 4 * EB * (size_t)n, outb = 4 * TB * O::LANES * (size_t)n;
    DevRun d;
    const uint8_t *da = d.up(acc, pts, 4 * EB * (size_t)groups), *db = d.up(b, pts, 4 * EB * (size_t)groups);
    const uint8_t* dk = d.up(k, 32 * (size_t)n, 32 * (size_t)groups);
    uint8_t* dout = d.alloc(outb);
    if (!d.ok()) return d.err;
    hipLaunchKernelGGL((k_pt_ops<O, FORMS>), dim3(lanes / block), dim3(block), 0, 0, op, da, db, dk, dout, (uint32_t)n);
    d.launched();
    return d.back(out, dout, outb);
}

extern "C" {
// which: 0 Fp (48 B) 1 Fr (32 B); e: ne little-endian 32-bit words of the exponent of op 4
int mh_inv_ops(int which, int op, const uint8_t* a, const uint32_t* e, int ne, uint8_t* out, int n) {
    for (int i = 0; i < n; ++i) {
        if (which == 0)
            inv_op<FpCfg>(op, a + 48 * (size_t)i, e, ne, out + 48 * (size_t)i);
        else
            inv_op<FrCfg>(op, a + 32 * (size_t)i, e, ne, out + 32 * (size_t)i);
    }
    return 0;
}
int mh_inv_ops_gpu(int which, int op, const uint8_t* a, const uint32_t* e, int ne, uint8_t* out, int n) {
    const size_t bytes = (size_t)(which == 0 ? 48 : 32) * n;
    DevRun d;
    const uint8_t* da = d.up(a, bytes);
    const uint32_t* de = d.up<uint32_t>(e, 4 * (size_t)ne);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    if (which == 0)
        hipLaunchKernelGGL((k_inv_ops<FpCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, de, ne, dout, (uint32_t)n);
    else
        hipLaunchKernelGGL((k_inv_ops<FrCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, de, ne, dout, (uint32_t)n);
    d.launched();
    return d.back(out, dout, bytes);
}
int mh_cold_products_gpu(int which, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const size_t bytes = (size_t)(which == 0 ? 48 : 32) * n;
    DevRun d;
    const uint8_t *da = d.up(a, bytes), *db = d.up(b, bytes);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    if (which == 0)
        hipLaunchKernelGGL((k_cold_products<FpCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, (uint32_t)n);
    else
        hipLaunchKernelGGL((k_cold_products<FrCfg>), dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, (uint32_t)n);
    d.launched();
    return d.back(out, dout, bytes);
}
int mh_fp2_ops(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    for (int i = 0; i < n; ++i) fp2_op(op, a + 96 * (size_t)i, b + 96 * (size_t)i, out + 96 * (size_t)i);
    return 0;
}
int mh_fp2_ops_gpu(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n) {
    const size_t bytes = (size_t)96 * n;
    DevRun d;
    const uint8_t *da = d.up(a, bytes), *db = d.up(b, bytes);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    hipLaunchKernelGGL(k_fp2_ops, dim3((n + 63) / 64), dim3(64), 0, 0, op, da, db, dout, (uint32_t)n);
    d.launched();
    return d.back(out, dout, bytes);
}
// block: 64 or 256 threads
int mh_fp2pair_ops_gpu(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int block) {
    const uint32_t lanes = pad_lanes(2u * n);
    const size_t bytes = (size_t)96 * n, cap = (size_t)48 * lanes;
    DevRun d;
    const uint8_t *da = d.up(a, bytes, cap), *db = d.up(b, bytes, cap);
    uint8_t* dout = d.alloc(bytes);
    if (!d.ok()) return d.err;
    hipLaunchKernelGGL(k_fp2pair_ops, dim3(lanes / block), dim3(block), 0, 0, op, da, db, dout, (uint32_t)n);
    d.launched();
    return d.back(out, dout, bytes);
}
// which: 0 FpOps 1 Fp2Ops (host and device) 2 Fp2PairOps 3 FpQuadOps 4 Fp2OctOps (device).  acc, b: n stored points; k: n scalars
// (32 B); out: n * O::LANES * 4 * sizeof(O::T) bytes
int mh_pt_ops(int which, int op, const uint8_t* acc, const uint8_t* b, const uint8_t* k, uint8_t* out, int n) {
    for (int i = 0; i < n; ++i) {
        if (which == 0) {
            Xyzz<FpOps> pa, pb;
            pt_load(pa, acc + 192 * (size_t)i, 0);
            pt_load(pb, b + 192 * (size_t)i, 0);
            pt_store(pt_op<FpOps, PT_ALL>(op, pa, pb, k + 32 * (size_t)i), out + 192 * (size_t)i);
        } else {
            Xyzz<Fp2Ops> pa, pb;
            pt_load(pa, acc + 384 * (size_t)i, 0);
            pt_load(pb, b + 384 * (size_t)i, 0);
            pt_store(pt_op<Fp2Ops, PT_ALL>(op, pa, pb, k + 32 * (size_t)i), out + 384 * (size_t)i);
        }
    }
    return 0;
}
int mh_pt_ops_gpu(int which, int op, const uint8_t* acc, const uint8_t* b, const uint8_t* k, uint8_t* out, int n, int block) {
    switch (which) {
        case 0: return pt_run<FpOps, PT_ALL>(op, acc, b, k, out, n, block);
        case 1: return pt_run<Fp2Ops, PT_ALL>(op, acc, b, k, out, n, block);
        case 2: return pt_run<Fp2PairOps, PT_NO_AFFINE>(op, acc, b, k, out, n, block);
        case 3: return pt_run<FpQuadOps, PT_COOP>(op, acc, b, k, out, n, block);
        default: return pt_run<Fp2OctOps, PT_COOP>(op, acc, b, k, out, n, block);
    }
}
// which: 0 FpOps (48 B per element) 1 Fp2PairOps (96 B); raw limbs in and out
int mh_binv_gpu(int which, const uint8_t* in, int n, int binv_c, int binv_mid, uint8_t* out) {
    if (which == 0) return binv_run<FpOps>(in, (uint32_t)n, (uint32_t)binv_c, (uint32_t)binv_mid, out);
    return binv_run<Fp2PairOps>(in, (uint32_t)n, (uint32_t)binv_c, (uint32_t)binv_mid, out);
}
}
