// Groth16 parameter generation from explicit toxic waste, on the GPU.
//
// Mirrors bellperson's `groth16::generate_random_parameters` / `generate_parameters` (nam-bellperson
// 0.26.6-nam.1, un-vendored; called by the reference's benches at
// /root/reference/masp_proofs/benches/sapling.rs:24-36 and benches/convert.rs:19-29) with the semantics of
// QAP polynomials evaluated at tau through the Lagrange basis of the 2^k domain, queries
// h, l, ic, a, b_g1, b_g2 as fixed-base multiples of the standard generators, identities filtered out.
// The real MASP parameters come from an MPC and cannot be regenerated; this exists so that benches and
// tests have a CRS (no network).
#pragma once
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "fr_io.hpp"
#include "io.hpp"

namespace masp {

// lag[k] = (Z(tau)/m) * w^k / (tau - w^k)      (Montgomery)
__global__ void k_setup_lagrange(Fr* __restrict__ lag, uint32_t nrows, Fr omega, Fr tau, Fr z_over_m) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrows) return;
    uint32_t e[1] = {k};
    Fr wk = fe_pow(omega, e, 1);
    Fr den = fe_inv(fe_sub(tau, wk));
    fr_store(lag + k, fe_mul(fe_mul(z_over_m, wk), den));
}
// per variable v: out[v] = sum over its column entries coef * lag[row]   (CSC; coef Montgomery)
__global__ void k_setup_qap(const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ rowidx, const Fr* __restrict__ coef,
                            const Fr* __restrict__ lag, uint32_t nv, uint32_t n_inputs, uint32_t n_constraints, int is_a,
                            Fr* __restrict__ out) {
    uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    Fr acc = fe_zero<FrCfg>();
    for (uint32_t t = colptr[v]; t < colptr[v + 1]; ++t) acc = fe_add(acc, fe_mul(fr_load(coef + t), fr_load(lag + rowidx[t])));
    if (is_a && v < n_inputs) acc = fe_add(acc, fr_load(lag + n_constraints + v));  // the extra Input(i) * 0 = 0 rows
    fr_store(out + v, acc);
}
// k[v] = (beta * at[v] + alpha * bt[v] + ct[v]) * scale
__global__ void k_setup_lc(const Fr* __restrict__ at, const Fr* __restrict__ bt, const Fr* __restrict__ ct, uint32_t n, Fr alpha, Fr beta,
                           Fr scale, Fr* __restrict__ out) {
    uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    Fr x = fe_add(fe_add(fe_mul(beta, fr_load(at + v)), fe_mul(alpha, fr_load(bt + v))), fr_load(ct + v));
    fr_store(out + v, fe_mul(x, scale));
}
// flags[v] = value != 0
__global__ void k_setup_nonzero(const Fr* __restrict__ x, uint32_t n, uint8_t* __restrict__ flags) {
    uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    flags[v] = fe_is_zero(fr_load(x + v)) ? 0 : 1;
}

// Fixed-base tables: tab[w*255 + d-1] = d * 2^(8w) * G  (affine), w < 32.  One lane per window.
template <class O>
__global__ void k_setup_fixed_table(Affine<O> gen, Affine<O>* __restrict__ tab) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= 32) return;
    Xyzz<O> base = xyzz_from_affine(gen);
    for (uint32_t k = 0; k < 8 * w; ++k) base = xyzz_dbl(base);
    Affine<O> b = xyzz_to_affine(base);
    Xyzz<O> cur = xyzz_from_affine(b);
    for (uint32_t d = 1; d <= 255; ++d) {
        tab[w * 255 + d - 1] = xyzz_to_affine(cur);
        xyzz_madd_nc(cur, b, false);
    }
}
// out[i] = [k_i] G as uncompressed bytes; scalars Montgomery (mont != 0) or canonical
template <class O, int BYTES>
__global__ void __launch_bounds__(64) k_setup_fixed_mul(const Affine<O>* __restrict__ tab, const Fr* __restrict__ scalars, uint32_t n, int mont,
                                                        uint8_t* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr k = fr_load(scalars + i);
    if (mont) k = fe_from_mont(k);
    Xyzz<O> acc = xyzz_inf<O>();
    for (int w = 0; w < 32; ++w) {
        uint32_t d = (k.v[w >> 2] >> (8 * (w & 3))) & 0xffu;
        if (d) xyzz_madd_nc(acc, tab[w * 255 + d - 1], false);
    }
    Affine<O> p = xyzz_to_affine(acc);
    if constexpr (BYTES == 96)
        g1_write_uncompressed(p, out + (size_t)i * 96);
    else
        g2_write_uncompressed(p, out + (size_t)i * 192);
}
// dst[k] = src[idx[k]]
__global__ void k_setup_gather(const Fr* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, Fr* __restrict__ dst) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    fr_store(dst + k, fr_load(src + idx[k]));
}
// h scalars: out[i] = tau^i * c    (c = Z(tau)/delta)
__global__ void k_setup_h_scalars(Fr tau, Fr c, uint32_t n, Fr* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t e[1] = {i};
    fr_store(out + i, fe_mul(fe_pow(tau, e, 1), c));
}


// ---- the quotient's evaluation form: bases derived once per circuit (k_setup.hip: build_eval_bases) ---------------------------
// Set-up code: one lane per point or butterfly, every field product a call (the _nc forms), a full double-and-add per twiddle.

// Two group-valued transforms side by side (blockIdx.y): X[y][rev(k)] = [s_k] H_k for k < n_h, infinity above.
// y = 0: s_k = scale_tab[k];  y = 1: s_k = scale_const.  Scalars canonical; H_k uncompressed (96 bytes).
__global__ void __launch_bounds__(64) k_g1ntt_load(const uint8_t* __restrict__ h_raw, uint32_t n_h, const Fr* __restrict__ scale_tab, Fr scale_const,
                                                   uint32_t logm, G1Xyzz* __restrict__ X) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << logm)) return;
    X += (size_t)blockIdx.y << logm;
    G1Xyzz r = xyzz_inf<FpOps>();
    if (k < n_h) {
        G1Affine p;
        g1_read_uncompressed(h_raw + (size_t)96 * k, p);
        const Fr sc = blockIdx.y == 0 ? fr_load(scale_tab + k) : scale_const;
        r = xyzz_mul_scalar(xyzz_from_affine(p), sc.v);
    }
    X[__brev(k) >> (32 - logm)] = r;
}
// Stage st of the decimation-in-time transform over G1 on bit-reversed input, in place: lane b owns the pair (i0, i0 + 2^st).
// tw[k] = w^k for k < m/2, Montgomery (NttDomain::tw_inv); the same index arithmetic as k_ntt_pass's single stages.
__global__ void __launch_bounds__(64) k_g1ntt_stage(G1Xyzz* __restrict__ X, const Fr* __restrict__ tw, uint32_t logm, uint32_t st) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (1u << (logm - 1))) return;
    X += (size_t)blockIdx.y << logm;
    const uint32_t j = b & ((1u << st) - 1u), i0 = ((b >> st) << (st + 1)) | j, i1 = i0 + (1u << st);
    G1Xyzz u = X[i0], t = X[i1];
    if (j) {
        const Fr w = fe_from_mont(fr_load(tw + ((size_t)j << (logm - st - 1))));
        t = xyzz_mul_scalar(t, w.v);
    }
    G1Xyzz v = u;
    xyzz_add_nc(v, t);
    xyzz_add_nc(u, xyzz_neg(t));
    X[i0] = v;
    X[i1] = u;
}
// out[i] = X[i] as uncompressed bytes; *any_inf |= 1 if one of them is the point at infinity
__global__ void __launch_bounds__(64) k_g1_xyzz_to_bytes(const G1Xyzz* __restrict__ X, uint32_t n, uint8_t* __restrict__ out, int* __restrict__ any_inf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = xyzz_to_affine(X[i]);
    if (aff_is_inf(p)) atomicOr(any_inf, 1);
    g1_write_uncompressed(p, out + (size_t)96 * i);
}

// acc += [c] p for a canonical coefficient c; +-1 without a multiplication (nearly every coefficient of a MASP circuit's C)
__device__ __forceinline__ void eval_combine_term(G1Xyzz& acc, const G1Xyzz& p, const Fr& c, const Fr& minus_one) {
    Fr one = fe_zero<FrCfg>();
    one.v[0] = 1;
    if (fe_eq(c, one))
        xyzz_add_nc(acc, p);
    else if (fe_eq(c, minus_one))
        xyzz_add_nc(acc, xyzz_neg(p));
    else
        xyzz_add_nc(acc, xyzz_mul_scalar(p, c.v));
}
// what every derived slot ends with: + L_j for an aux column, to affine bytes, infinity flagged
__device__ __forceinline__ void eval_combine_finish(G1Xyzz acc, uint32_t o, uint32_t n_aux, const uint8_t* __restrict__ l_raw, uint8_t* __restrict__ out,
                                                    int* __restrict__ any_inf) {
    if (o < n_aux) {
        G1Affine l;
        g1_read_uncompressed(l_raw + (size_t)96 * o, l);
        xyzz_madd_nc(acc, l, false);
    }
    const G1Affine p = xyzz_to_affine(acc);
    if (aff_is_inf(p)) atomicOr(any_inf, 1);
    g1_write_uncompressed(p, out + (size_t)96 * o);
}
// The sparse combine.  Derived slot o (aux columns first, then the input columns C uses: slot_cols[o] is its column of C, CSC with
// canonical coefficients): out[o] = sum_t coef[t] * T[rowidx[t]]  (+ L_o for o < n_aux).  One lane per slot; a column of long_col or more
// entries is left to k_eval_combine_long.
__global__ void __launch_bounds__(64) k_eval_combine(const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ rowidx, const Fr* __restrict__ coef,
                                                     const G1Xyzz* __restrict__ T, const uint32_t* __restrict__ slot_cols, uint32_t n_slots, uint32_t n_aux,
                                                     uint32_t long_col, Fr minus_one, const uint8_t* __restrict__ l_raw, uint8_t* __restrict__ out,
                                                     int* __restrict__ any_inf) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_slots) return;
    const uint32_t v = slot_cols[o], lo = colptr[v], hi = colptr[v + 1];
    if (hi - lo >= long_col) return;
    G1Xyzz acc = xyzz_inf<FpOps>();
    for (uint32_t t = lo; t < hi; ++t) eval_combine_term(acc, T[rowidx[t]], fr_load(coef + t), minus_one);
    eval_combine_finish(acc, o, n_aux, l_raw, out, any_inf);
}
// the long columns (the constant-one input can be one): a wave per slot of long_slots, lanes stride over the entries, a shuffle tree adds
__global__ void __launch_bounds__(64) k_eval_combine_long(const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ rowidx, const Fr* __restrict__ coef,
                                                          const G1Xyzz* __restrict__ T, const uint32_t* __restrict__ slot_cols,
                                                          const uint32_t* __restrict__ long_slots, uint32_t n_aux, Fr minus_one,
                                                          const uint8_t* __restrict__ l_raw, uint8_t* __restrict__ out, int* __restrict__ any_inf) {
    const uint32_t o = long_slots[blockIdx.x], lane = threadIdx.x;
    const uint32_t v = slot_cols[o], lo = colptr[v], hi = colptr[v + 1];
    G1Xyzz acc = xyzz_inf<FpOps>();
    for (uint32_t t = lo + lane; t < hi; t += 64) eval_combine_term(acc, T[rowidx[t]], fr_load(coef + t), minus_one);
    for (int d = 32; d >= 1; d >>= 1) {
        G1Xyzz other;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            other.X.v[i] = (uint32_t)__shfl_down((int)acc.X.v[i], d, 64);
            other.Y.v[i] = (uint32_t)__shfl_down((int)acc.Y.v[i], d, 64);
            other.ZZ.v[i] = (uint32_t)__shfl_down((int)acc.ZZ.v[i], d, 64);
            other.ZZZ.v[i] = (uint32_t)__shfl_down((int)acc.ZZZ.v[i], d, 64);
        }
        xyzz_add_nc(acc, other);
    }
    if (lane == 0) eval_combine_finish(acc, o, n_aux, l_raw, out, any_inf);
}

}  // namespace masp
