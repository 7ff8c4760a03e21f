// Radix-2 NTT over the BLS12-381 scalar field and the Groth16 quotient  h = (A*B - C)/Z  for gfx950.
//
// Six transforms, not bellperson's seven: with Z = x^m - 1 and C = A B mod Z (c = a o b on the domain), the product reduced
// on the coset g H is  A B mod (x^m - g^m) = (g^m - 1) h + C,  so  h = (icoset_fft(A B on the coset) - C) / (g^m - 1)  and C
// never has to be carried onto the coset and back (its coefficients come out of the first inverse transform anyway).
// Same field elements as the reference sequence: h is unique.
//
// Replaces bellperson's `EvaluationDomain::{ifft, coset_fft, mul_assign, sub_assign,
// divide_by_z_on_coset, icoset_fft}` sequence (nam-bellperson 0.26.6-nam.1, un-vendored; SURVEY.md A.3
// step 3, reached from /root/reference/masp_proofs/src/sapling/prover.rs:117,202,252) and the
// `<Fr>_radix_fft` kernel of nam-ec-gpu-gen.
//
// A transform of 2^logm points in the general chain (k_ntt_pass) is: one bit-reversal pass (fused with whatever pointwise
// work precedes it) and then ceil(logm / 10) LDS passes, each doing up to 10 butterfly stages on a
// 1024-element (32 KiB) tile held in LDS.  A lone transform (<= 4 MiB) stays in L2 / Infinity Cache
// between passes; in batch mode every pass runs over the whole batch (np x 4 MiB per buffer), which streams
// through HBM — see enqueue_quotient for how the batch is cut so that a sub-batch's working set stays in MALL.
//
// The evaluation-form quotient of a batch (10 < logm <= 20) has no bit-reversal pass at all: its inverse transform is decimation
// in FREQUENCY (natural order in, bit-reversed out), its forward transform decimation in time (bit-reversed in, natural out), and
// the low ten stages of both work on the same contiguous tile.  Three kernels, at the end of this file: k_ntt_dif_top (reads the
// evaluation vectors where k_r1cs_eval left them), k_ntt_mid (both transforms' low stages with the coset scale between them) and
// k_ntt_dit_top_ab (a's and b's top stages and their product, straight into the merged scalar buffer).
#pragma once
#include <hip/hip_runtime.h>

#include "field.hpp"
#include "fr_io.hpp"
#include "ntt_geom.h"

namespace masp {


__device__ __forceinline__ uint32_t bitrev(uint32_t k, uint32_t logm) { return __brev(k) >> (32 - logm); }

// table[k] = scale * base^k  (Montgomery in, Montgomery out; `plain` strips the Montgomery factor)
__global__ void k_fr_powers(Fr* __restrict__ table, uint32_t n, Fr base, Fr scale, int plain) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t e[1] = {k};
    Fr r = fe_mul(fe_pow(base, e, 1), scale);
    if (plain) r = fe_from_mont(r);
    fr_store(table + k, r);
}

// table[i] = scale * base^rev(i), rev over logn bits (Montgomery): a k_fr_powers table in the order a decimation-in-frequency transform leaves
__global__ void k_fr_powers_bitrev(Fr* __restrict__ table, uint32_t logn, Fr base, Fr scale) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << logn)) return;
    uint32_t e[1] = {bitrev(i, logn)};
    fr_store(table + i, fe_mul(fe_pow(base, e, 1), scale));
}

// Prove-time kernels take gridDim.y = proofs in the batch; proof p uses `ptr + p * stride` (strides in elements).
#define NTT_P (blockIdx.y)

// ---- bit-reversal passes with fused pointwise work ------------------------------------------------
// y[rev(k)] = to_mont(x[k]) for k < nrows, 0 above   (x canonical little-endian limbs)
__global__ void k_ntt_load_bitrev(const Fr* __restrict__ x, size_t x_stride, uint32_t nrows, Fr* __restrict__ y, uint32_t logm) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << logm)) return;
    x += NTT_P * x_stride;
    y += (size_t)NTT_P << logm;
    Fr v = fe_zero<FrCfg>();
    if (k < nrows) v = fe_to_mont(fr_load(x + k));
    fr_store(y + bitrev(k, logm), v);
}
// same but the input is already in Montgomery form
__global__ void k_ntt_copy_bitrev(const Fr* __restrict__ x, size_t x_stride, uint32_t nrows, Fr* __restrict__ y, uint32_t logm) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << logm)) return;
    x += NTT_P * x_stride;
    y += (size_t)NTT_P << logm;
    Fr v = fe_zero<FrCfg>();
    if (k < nrows) v = fr_load(x + k);
    fr_store(y + bitrev(k, logm), v);
}
// y[rev(k)] = x[k] * scale[k]
__global__ void k_ntt_scale_bitrev(const Fr* __restrict__ x, const Fr* __restrict__ scale, Fr* __restrict__ y, uint32_t logm) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << logm)) return;
    x += (size_t)NTT_P << logm;
    y += (size_t)NTT_P << logm;
    fr_store(y + bitrev(k, logm), fe_mul(fr_load(x + k), fr_load(scale + k)));
}
// y[rev(k)] = a[k] * b[k]
__global__ void k_ntt_ab_bitrev(const Fr* __restrict__ a, const Fr* __restrict__ b, Fr* __restrict__ y, uint32_t logm) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << logm)) return;
    a += (size_t)NTT_P << logm;
    b += (size_t)NTT_P << logm;
    y += (size_t)NTT_P << logm;
    fr_store(y + bitrev(k, logm), fe_mul(fr_load(a + k), fr_load(b + k)));
}
// y[k] = a[k] * b[k] * scale   (no permutation; a plain-form scale: the result leaves Montgomery form).  The quotient's evaluation form:
// a, b are the coset evaluations, scale = 1 / (g^m - 1), y a proof's share of the merged scalar buffer.
__global__ void k_ntt_ab_eval(const Fr* __restrict__ a, const Fr* __restrict__ b, Fr scale, Fr* __restrict__ y, uint32_t n, size_t y_stride) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    a += (size_t)NTT_P * n;
    b += (size_t)NTT_P * n;
    y += (size_t)NTT_P * y_stride;
    fr_store(y + k, fe_mul(fe_mul(fr_load(a + k), fr_load(b + k)), scale));
}
// y[k] = x[k] * scale[k] - c[k] * cscale   (plain-form scale factors: the result leaves Montgomery form)
__global__ void k_fr_scale_sub(const Fr* __restrict__ x, const Fr* __restrict__ scale, const Fr* __restrict__ c, Fr cscale, Fr* __restrict__ y,
                               uint32_t n, size_t y_stride) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    x += (size_t)NTT_P * n;
    c += (size_t)NTT_P * n;
    y += (size_t)NTT_P * y_stride;
    fr_store(y + k, fe_sub(fe_mul(fr_load(x + k), fr_load(scale + k)), fe_mul(fr_load(c + k), cscale)));
}
// y[k] = x[k] * scale[k]  (no permutation; with a plain-form scale table this also leaves Montgomery form)
__global__ void k_fr_scale(const Fr* __restrict__ x, const Fr* __restrict__ scale, Fr* __restrict__ y, uint32_t n, size_t y_stride) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    x += (size_t)NTT_P * n;
    y += (size_t)NTT_P * y_stride;
    fr_store(y + k, fe_mul(fr_load(x + k), fr_load(scale + k)));
}
__global__ void k_fr_from_mont(const Fr* __restrict__ x, Fr* __restrict__ y, uint32_t n) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    fr_store(y + k, fe_from_mont(fr_load(x + k)));
}

// ---- LDS pass: stages [s0, s0 + nst) of a decimation-in-time transform on bit-reversed input -------
// Index bits of an element: [0, s0) "lo" | [s0, s0+nst) "h" (the butterfly bits of this pass) | rest "top".
// A tile holds every h for `cols` = 2^(LT - nst) consecutive columns, column = top * 2^s0 + lo.
// tw[k] = w^k for k < m/2 (w = omega or omega^-1).
__global__ void __launch_bounds__(256) k_ntt_pass(Fr* __restrict__ data, const Fr* __restrict__ tw, uint32_t logm, uint32_t s0,
                                                  uint32_t nst) {
    __shared__ uint4 tile[2 << NTT_LT];  // 2 x uint4 per element, split planes to keep ds_read_b128 conflict-light
    const uint32_t lt = nst + (NTT_LT - nst < logm - nst ? NTT_LT - nst : logm - nst);  // log2 of this tile's size
    const uint32_t cols_log = lt - nst;
    const uint32_t cols = 1u << cols_log;
    const uint32_t tsize = 1u << lt;
    const uint32_t col0 = blockIdx.x << cols_log;
    const uint32_t lomask = (1u << s0) - 1u;
    data += (size_t)NTT_P << logm;
    // load
    for (uint32_t L = threadIdx.x; L < tsize; L += blockDim.x) {
        uint32_t h = L >> cols_log, col = col0 + (L & (cols - 1));
        uint32_t idx = ((col >> s0) << (s0 + nst)) | (h << s0) | (col & lomask);
        const uint4* q = reinterpret_cast<const uint4*>(data + idx);
        tile[L] = q[0];
        tile[tsize + L] = q[1];
    }
    __syncthreads();
    auto ld = [&](uint32_t L) {
        Fr r;
        uint4 a0 = tile[L], a1 = tile[tsize + L];
        r.v[0] = a0.x; r.v[1] = a0.y; r.v[2] = a0.z; r.v[3] = a0.w; r.v[4] = a1.x; r.v[5] = a1.y; r.v[6] = a1.z; r.v[7] = a1.w;
        return r;
    };
    auto st = [&](uint32_t L, const Fr& x) {
        tile[L] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
        tile[tsize + L] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    };
    uint32_t q = 0;
    // two stages at a time: a lane holds the four elements that differ in bits q, q + 1 of the butterfly index and does both
    // stages in registers (same four products as two radix-2 stages, half the LDS round trips and barriers)
    for (; q + 1 < nst; q += 2) {
        const uint32_t s = s0 + q;
        for (uint32_t gidx = threadIdx.x; gidx < (tsize >> 2); gidx += blockDim.x) {
            const uint32_t cl = gidx & (cols - 1), r = gidx >> cols_log;
            const uint32_t hj = r & ((1u << q) - 1u), hg = r >> q;
            const uint32_t h00 = (hg << (q + 2)) | hj;
            const uint32_t L0 = (h00 << cols_log) | cl, d = cols << q;  // elements at L0, L0 + d, L0 + 2d, L0 + 3d
            const uint32_t lo = (col0 + cl) & lomask;
            const uint32_t j1 = (hj << s0) | lo;                          // stage s: both pairs
            const uint32_t j2a = j1, j2b = ((hj | (1u << q)) << s0) | lo;  // stage s + 1: pairs with bit q clear / set
            Fr x0 = ld(L0), x1 = ld(L0 + d), x2 = ld(L0 + 2 * d), x3 = ld(L0 + 3 * d);
            if (s == 0) {  // the first two stages of a transform: twiddles 1, 1 and (1, w^(m/4)) — one product instead of four
                const Fr y0 = fe_add(x0, x1), y1 = fe_sub(x0, x1), y2 = fe_add(x2, x3), y3 = fe_sub(x2, x3);
                st(L0, fe_add(y0, y2));
                st(L0 + 2 * d, fe_sub(y0, y2));
                const Fr t = fe_mul(y3, fr_load(tw + ((size_t)1 << (logm - 2))));
                st(L0 + d, fe_add(y1, t));
                st(L0 + 3 * d, fe_sub(y1, t));
                continue;
            }
            const Fr w1 = fr_load(tw + ((size_t)j1 << (logm - s - 1)));
            const Fr w2a = fr_load(tw + ((size_t)j2a << (logm - s - 2)));
            const Fr w2b = fr_load(tw + ((size_t)j2b << (logm - s - 2)));
            Fr t = fe_mul(x1, w1);
            Fr y0 = fe_add(x0, t), y1 = fe_sub(x0, t);
            t = fe_mul(x3, w1);
            Fr y2 = fe_add(x2, t), y3 = fe_sub(x2, t);
            t = fe_mul(y2, w2a);
            st(L0, fe_add(y0, t));
            st(L0 + 2 * d, fe_sub(y0, t));
            t = fe_mul(y3, w2b);
            st(L0 + d, fe_add(y1, t));
            st(L0 + 3 * d, fe_sub(y1, t));
        }
        __syncthreads();
    }
    for (; q < nst; ++q) {
        const uint32_t s = s0 + q;
        for (uint32_t b = threadIdx.x; b < (tsize >> 1); b += blockDim.x) {
            uint32_t cl = b & (cols - 1), hb = b >> cols_log;
            uint32_t hj = hb & ((1u << q) - 1u), hg = hb >> q;
            uint32_t L0 = (((hg << (q + 1)) | hj) << cols_log) | cl;
            uint32_t L1 = L0 + (cols << q);
            uint32_t col = col0 + cl;
            uint32_t jglob = (hj << s0) | (col & lomask);
            Fr w = fr_load(tw + ((size_t)jglob << (logm - s - 1)));
            Fr u = ld(L0), v = fe_mul(ld(L1), w);
            st(L0, fe_add(u, v));
            st(L1, fe_sub(u, v));
        }
        __syncthreads();
    }
    for (uint32_t L = threadIdx.x; L < tsize; L += blockDim.x) {
        uint32_t h = L >> cols_log, col = col0 + (L & (cols - 1));
        uint32_t idx = ((col >> s0) << (s0 + nst)) | (h << s0) | (col & lomask);
        uint4* q = reinterpret_cast<uint4*>(data + idx);
        q[0] = tile[L];
        q[1] = tile[tsize + L];
    }
}

// ---- the evaluation-form quotient without permutation passes: three kernels for NTT_LT < logm <= 2 NTT_LT ---------------------------
// Stage s of either transform pairs the elements whose indices differ in bit s, with the twiddle tw[j << (logm - s - 1)], j = the index's
// bits below s — k_ntt_pass's numbering.  Decimation in time runs s upwards with the butterfly (u + v w, u - v w); decimation in
// frequency runs s downwards with (u + v, (u - v) w) and leaves element k at index rev(k).  Interpolation on H by DIF with tw_inv, times
// g^rev(i) / m at index i, then DIT with tw_fwd: the evaluations on g H in natural order, with no permutation anywhere.
// A tile is always 2^NTT_LT elements (logm > NTT_LT) and is worked on by 256 lanes: a quarter of a tile is one lane each.
static constexpr uint32_t NTT_TILE = 1u << NTT_LT, NTT_TILE_LANES = NTT_TILE / 4;

__device__ __forceinline__ Fr ntt_tile_ld(const uint4* tile, uint32_t L) {
    Fr r;
    uint4 a0 = tile[L], a1 = tile[NTT_TILE + L];
    r.v[0] = a0.x; r.v[1] = a0.y; r.v[2] = a0.z; r.v[3] = a0.w; r.v[4] = a1.x; r.v[5] = a1.y; r.v[6] = a1.z; r.v[7] = a1.w;
    return r;
}
__device__ __forceinline__ void ntt_tile_st(uint4* tile, uint32_t L, const Fr& x) {
    tile[L] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    tile[NTT_TILE + L] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
// The top stages [NTT_LT, logm) on a tile in LDS — every value h of the index bits from NTT_LT up, for the 2^cols_log consecutive
// columns (index bits below NTT_LT) from col0: tile[(h << cols_log) | cl] is element (h << NTT_LT) | (col0 + cl), k_ntt_pass's tile of
// its second pass.  t: this lane among the tile's 256.  Every lane of the workgroup must call it (barriers); it ends behind one.
template <bool DIF>
__device__ __forceinline__ void ntt_top_stages(uint4* tile, const Fr* __restrict__ tw, uint32_t logm, uint32_t col0, uint32_t t) {
    const uint32_t s0 = NTT_LT, nst = logm - NTT_LT, cols_log = NTT_LT - nst, cols = 1u << cols_log;
    // two stages at a time, as k_ntt_pass: a lane holds the four elements that differ in bits q, q + 1 of h
    auto pair = [&](uint32_t q) {
        const uint32_t s = s0 + q;
        const uint32_t cl = t & (cols - 1), r = t >> cols_log;
        const uint32_t hj = r & ((1u << q) - 1u), hg = r >> q;
        const uint32_t L0 = (((hg << (q + 2)) | hj) << cols_log) | cl, d = cols << q;
        const uint32_t lo = col0 + cl;
        const uint32_t j1 = (hj << s0) | lo;                          // stage s: both pairs
        const uint32_t j2a = j1, j2b = ((hj | (1u << q)) << s0) | lo;  // stage s + 1: pairs with bit q clear / set
        const Fr w1 = fr_load(tw + ((size_t)j1 << (logm - s - 1)));
        const Fr w2a = fr_load(tw + ((size_t)j2a << (logm - s - 2)));
        const Fr w2b = fr_load(tw + ((size_t)j2b << (logm - s - 2)));
        const Fr x0 = ntt_tile_ld(tile, L0), x1 = ntt_tile_ld(tile, L0 + d), x2 = ntt_tile_ld(tile, L0 + 2 * d), x3 = ntt_tile_ld(tile, L0 + 3 * d);
        if (DIF) {  // stage s + 1 first
            const Fr y0 = fe_add(x0, x2), y2 = fe_mul(fe_sub(x0, x2), w2a);
            const Fr y1 = fe_add(x1, x3), y3 = fe_mul(fe_sub(x1, x3), w2b);
            ntt_tile_st(tile, L0, fe_add(y0, y1));
            ntt_tile_st(tile, L0 + d, fe_mul(fe_sub(y0, y1), w1));
            ntt_tile_st(tile, L0 + 2 * d, fe_add(y2, y3));
            ntt_tile_st(tile, L0 + 3 * d, fe_mul(fe_sub(y2, y3), w1));
        } else {
            Fr u = fe_mul(x1, w1);
            const Fr y0 = fe_add(x0, u), y1 = fe_sub(x0, u);
            u = fe_mul(x3, w1);
            const Fr y2 = fe_add(x2, u), y3 = fe_sub(x2, u);
            u = fe_mul(y2, w2a);
            ntt_tile_st(tile, L0, fe_add(y0, u));
            ntt_tile_st(tile, L0 + 2 * d, fe_sub(y0, u));
            u = fe_mul(y3, w2b);
            ntt_tile_st(tile, L0 + d, fe_add(y1, u));
            ntt_tile_st(tile, L0 + 3 * d, fe_sub(y1, u));
        }
        __syncthreads();
    };
    auto single = [&](uint32_t q) {
        const uint32_t s = s0 + q;
        for (uint32_t b = t; b < (NTT_TILE >> 1); b += NTT_TILE_LANES) {
            const uint32_t cl = b & (cols - 1), hb = b >> cols_log;
            const uint32_t hj = hb & ((1u << q) - 1u), hg = hb >> q;
            const uint32_t L0 = (((hg << (q + 1)) | hj) << cols_log) | cl, L1 = L0 + (cols << q);
            const Fr w = fr_load(tw + ((size_t)((hj << s0) | (col0 + cl)) << (logm - s - 1)));
            const Fr u = ntt_tile_ld(tile, L0), v = ntt_tile_ld(tile, L1);
            if (DIF) {
                ntt_tile_st(tile, L0, fe_add(u, v));
                ntt_tile_st(tile, L1, fe_mul(fe_sub(u, v), w));
            } else {
                const Fr vw = fe_mul(v, w);
                ntt_tile_st(tile, L0, fe_add(u, vw));
                ntt_tile_st(tile, L1, fe_sub(u, vw));
            }
        }
        __syncthreads();
    };
    if (DIF) {  // stages nst - 1 ... 0: pairs from the top, an odd count's last stage alone
        uint32_t q = nst;
        for (; q >= 2; q -= 2) pair(q - 2);
        if (q) single(0);
    } else {    // stages 0 ... nst - 1: pairs from the bottom, an odd count's last stage alone
        uint32_t q = 0;
        for (; q + 1 < nst; q += 2) pair(q);
        if (q < nst) single(q);
    }
}

// First kernel: the inverse transform's top stages, out of place.  gridDim.y = 2 q transforms — proof p of a for blockIdx.y = p < q, of b
// above — read as k_r1cs_eval left them (Montgomery, natural order, in_stride apart, nrows entries: zero above), written to y + blockIdx.y * m.
__global__ void __launch_bounds__(256) k_ntt_dif_top(const Fr* __restrict__ a, const Fr* __restrict__ b, size_t in_stride, uint32_t nrows, uint32_t q,
                                                     Fr* __restrict__ y, const Fr* __restrict__ tw, uint32_t logm) {
    __shared__ uint4 tile[2 << NTT_LT];
    const uint32_t cols_log = 2 * NTT_LT - logm, cols = 1u << cols_log, col0 = blockIdx.x << cols_log;
    const Fr* x = NTT_P < q ? a + (size_t)NTT_P * in_stride : b + (size_t)(NTT_P - q) * in_stride;
    y += (size_t)NTT_P << logm;
    for (uint32_t L = threadIdx.x; L < NTT_TILE; L += blockDim.x) {
        const uint32_t idx = ((L >> cols_log) << NTT_LT) | (col0 + (L & (cols - 1)));
        Fr v = fe_zero<FrCfg>();
        if (idx < nrows) v = fr_load(x + idx);
        ntt_tile_st(tile, L, v);
    }
    __syncthreads();
    ntt_top_stages<true>(tile, tw, logm, col0, threadIdx.x);
    for (uint32_t L = threadIdx.x; L < NTT_TILE; L += blockDim.x) {
        const uint32_t idx = ((L >> cols_log) << NTT_LT) | (col0 + (L & (cols - 1)));
        uint4* o = reinterpret_cast<uint4*>(y + idx);
        o[0] = tile[L];
        o[1] = tile[NTT_TILE + L];
    }
}

// Middle kernel, in place on the contiguous tile blockIdx.x of transform blockIdx.y: the inverse transform's stages NTT_LT - 1 ... 0 (tw_inv),
// element i times scale_rev[i] = g^rev(i) / m, the forward transform's stages 0 ... NTT_LT - 1 (tw_fwd).  The inverse's last two stages,
// the scale and the forward's first two act on the same four consecutive elements: one lane, in registers, and those are the stages whose
// twiddles are 1 and w^(m/4) — two products where eight would stand.
__global__ void __launch_bounds__(256) k_ntt_mid(Fr* __restrict__ data, const Fr* __restrict__ tw_inv, const Fr* __restrict__ scale_rev,
                                                 const Fr* __restrict__ tw_fwd, uint32_t logm) {
    static_assert(NTT_LT % 2 == 0 && NTT_LT >= 4, "the tile's stages go in pairs around the fused middle");
    __shared__ uint4 tile[2 << NTT_LT];
    const uint32_t base = blockIdx.x << NTT_LT, t = threadIdx.x;
    data += (size_t)NTT_P << logm;
    for (uint32_t L = t; L < NTT_TILE; L += blockDim.x) {
        const uint4* p = reinterpret_cast<const uint4*>(data + base + L);
        tile[L] = p[0];
        tile[NTT_TILE + L] = p[1];
    }
    __syncthreads();
    for (uint32_t q = NTT_LT - 2; q >= 2; q -= 2) {  // DIF stages q + 1, q
        const uint32_t hj = t & ((1u << q) - 1u), hg = t >> q, L0 = (hg << (q + 2)) | hj, d = 1u << q;
        const Fr w1 = fr_load(tw_inv + ((size_t)hj << (logm - q - 1)));
        const Fr w2a = fr_load(tw_inv + ((size_t)hj << (logm - q - 2)));
        const Fr w2b = fr_load(tw_inv + ((size_t)(hj | d) << (logm - q - 2)));
        const Fr x0 = ntt_tile_ld(tile, L0), x1 = ntt_tile_ld(tile, L0 + d), x2 = ntt_tile_ld(tile, L0 + 2 * d), x3 = ntt_tile_ld(tile, L0 + 3 * d);
        const Fr y0 = fe_add(x0, x2), y2 = fe_mul(fe_sub(x0, x2), w2a);
        const Fr y1 = fe_add(x1, x3), y3 = fe_mul(fe_sub(x1, x3), w2b);
        ntt_tile_st(tile, L0, fe_add(y0, y1));
        ntt_tile_st(tile, L0 + d, fe_mul(fe_sub(y0, y1), w1));
        ntt_tile_st(tile, L0 + 2 * d, fe_add(y2, y3));
        ntt_tile_st(tile, L0 + 3 * d, fe_mul(fe_sub(y2, y3), w1));
        __syncthreads();
    }
    {   // DIF stages 1, 0; the scale; DIT stages 0, 1 — elements 4 t ... 4 t + 3
        const uint32_t L0 = t << 2;
        const Fr* sc = scale_rev + base + L0;
        Fr x0 = ntt_tile_ld(tile, L0), x1 = ntt_tile_ld(tile, L0 + 1), x2 = ntt_tile_ld(tile, L0 + 2), x3 = ntt_tile_ld(tile, L0 + 3);
        Fr y0 = fe_add(x0, x2), y2 = fe_sub(x0, x2), y1 = fe_add(x1, x3);
        Fr y3 = fe_mul(fe_sub(x1, x3), fr_load(tw_inv + ((size_t)1 << (logm - 2))));
        x0 = fe_mul(fe_add(y0, y1), fr_load(sc));
        x1 = fe_mul(fe_sub(y0, y1), fr_load(sc + 1));
        x2 = fe_mul(fe_add(y2, y3), fr_load(sc + 2));
        x3 = fe_mul(fe_sub(y2, y3), fr_load(sc + 3));
        y0 = fe_add(x0, x1), y1 = fe_sub(x0, x1), y2 = fe_add(x2, x3);
        y3 = fe_mul(fe_sub(x2, x3), fr_load(tw_fwd + ((size_t)1 << (logm - 2))));
        ntt_tile_st(tile, L0, fe_add(y0, y2));
        ntt_tile_st(tile, L0 + 2, fe_sub(y0, y2));
        ntt_tile_st(tile, L0 + 1, fe_add(y1, y3));
        ntt_tile_st(tile, L0 + 3, fe_sub(y1, y3));
        __syncthreads();
    }
    for (uint32_t q = 2; q + 1 < (uint32_t)NTT_LT; q += 2) {  // DIT stages q, q + 1
        const uint32_t hj = t & ((1u << q) - 1u), hg = t >> q, L0 = (hg << (q + 2)) | hj, d = 1u << q;
        const Fr w1 = fr_load(tw_fwd + ((size_t)hj << (logm - q - 1)));
        const Fr w2a = fr_load(tw_fwd + ((size_t)hj << (logm - q - 2)));
        const Fr w2b = fr_load(tw_fwd + ((size_t)(hj | d) << (logm - q - 2)));
        const Fr x0 = ntt_tile_ld(tile, L0), x1 = ntt_tile_ld(tile, L0 + d), x2 = ntt_tile_ld(tile, L0 + 2 * d), x3 = ntt_tile_ld(tile, L0 + 3 * d);
        Fr u = fe_mul(x1, w1);
        const Fr y0 = fe_add(x0, u), y1 = fe_sub(x0, u);
        u = fe_mul(x3, w1);
        const Fr y2 = fe_add(x2, u), y3 = fe_sub(x2, u);
        u = fe_mul(y2, w2a);
        ntt_tile_st(tile, L0, fe_add(y0, u));
        ntt_tile_st(tile, L0 + 2 * d, fe_sub(y0, u));
        u = fe_mul(y3, w2b);
        ntt_tile_st(tile, L0 + d, fe_add(y1, u));
        ntt_tile_st(tile, L0 + 3 * d, fe_sub(y1, u));
        __syncthreads();
    }
    for (uint32_t L = t; L < NTT_TILE; L += blockDim.x) {
        uint4* p = reinterpret_cast<uint4*>(data + base + L);
        p[0] = tile[L];
        p[1] = tile[NTT_TILE + L];
    }
}

// Last kernel: the forward transform's top stages on the same strided tile of a (lanes 0 - 255: proof blockIdx.y at x) and of b (lanes
// 256 - 511: at x + b_off, the sub-batch's own q m), then y[k] = a[k] b[k] scale, canonical (plain-form scale), natural order, at
// y + blockIdx.y * y_stride — what k_ntt_ab_eval writes.  Both tiles in LDS (64 KiB): two workgroups of eight waves per CU, the four waves per
// SIMD that k_ntt_pass has.
__global__ void __launch_bounds__(512) k_ntt_dit_top_ab(const Fr* __restrict__ x, size_t b_off, const Fr* __restrict__ tw, Fr scale, Fr* __restrict__ y,
                                                        size_t y_stride, uint32_t logm) {
    __shared__ uint4 tiles[4 << NTT_LT];
    const uint32_t cols_log = 2 * NTT_LT - logm, cols = 1u << cols_log, col0 = blockIdx.x << cols_log;
    const uint32_t half = threadIdx.x >> 8, t = threadIdx.x & (NTT_TILE_LANES - 1);
    uint4* tile = tiles + half * (2u << NTT_LT);
    x += ((size_t)NTT_P << logm) + half * b_off;
    for (uint32_t L = t; L < NTT_TILE; L += NTT_TILE_LANES) {
        const uint32_t idx = ((L >> cols_log) << NTT_LT) | (col0 + (L & (cols - 1)));
        const uint4* p = reinterpret_cast<const uint4*>(x + idx);
        tile[L] = p[0];
        tile[NTT_TILE + L] = p[1];
    }
    __syncthreads();
    ntt_top_stages<false>(tile, tw, logm, col0, t);
    y += (size_t)NTT_P * y_stride;
    for (uint32_t L = threadIdx.x; L < NTT_TILE; L += blockDim.x) {
        const uint32_t idx = ((L >> cols_log) << NTT_LT) | (col0 + (L & (cols - 1)));
        fr_store(y + idx, fe_mul(fe_mul(ntt_tile_ld(tiles, L), ntt_tile_ld(tiles + (2u << NTT_LT), L)), scale));
    }
}

}  // namespace masp
