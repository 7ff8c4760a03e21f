// Device half of the GPU Groth16 batch verifier (bellman `verify_proofs_batch`, reached from
// /root/reference/masp_proofs/src/sapling/verifier/batch.rs:24-31,201-239):
//   k_verify_prepare   one lane per proof: decompress A, C (G1) and B (G2) from the 192 proof bytes (square roots in Fp /
//                      Fp2, zcash sign convention), z_i * A_i in affine form and z_i * C_i for the random 128-bit z_i
//   k_miller_pairs     one WAVE per pair (z_i A_i, B_i): the ate Miller loop as an interpreter of the levelled straight-line
//                      programs built on the host (host/pairing_prog.h): values in LDS slots, lane k executes operation k
//                      of the current step, so the ~135 dependent 384-bit products of an iteration become 3-4 product steps
//   k_fp12_product     the product of the pairs' Miller values (same interpreter, Fp12 multiplication program)
// For the batch call the public-input combination, the two remaining pairs and the final exponentiation stay on the host
// (host/pairing.h); the per-proof call (masp_hip_verify_each) runs all of it here: see "per-proof verdicts" below.
#pragma once
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "subgroup.hpp"
#include "io.hpp"
#include "point_read.hpp"

namespace masp {

// ---- stage 1: decode + randomise ---------------------------------------------------------------------------------
// proofs: n x 192 B; z: n x 16 B (little-endian, bit 0 forced to 1 like the host verifier).  Outputs per proof: za = z A
// (affine), b = B (affine), zc = z C (XYZZ), status = PT_* bits of the three points (the host refuses every one of them, PT_INFINITY included: k_verify.hip).
__global__ void __launch_bounds__(64) k_verify_prepare(const uint8_t* __restrict__ proofs, const uint8_t* __restrict__ z, uint32_t n,
                                                       G1Affine* __restrict__ za, G2Affine* __restrict__ b, G1Xyzz* __restrict__ zc,
                                                       int* __restrict__ status) {
    // gridDim.y = 5: y = 0 -> z A, 1 -> z C, 2 -> B and its subgroup test, 3 / 4 -> the subgroup tests of A / C (every wave does
    // one kind of work; B's square root + 64-bit multiple is the longest chain, the tests of A and C run next to their multiples)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, what = blockIdx.y;
    if (i >= n) return;
    const uint8_t* pr = proofs + 192 * (size_t)i;
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 4; ++w)
        k[w] = (uint32_t)z[16 * i + 4 * w] | ((uint32_t)z[16 * i + 4 * w + 1] << 8) | ((uint32_t)z[16 * i + 4 * w + 2] << 16) |
               ((uint32_t)z[16 * i + 4 * w + 3] << 24);
    k[0] |= 1u;
    int st;
    if (what == 2) {
        G2Affine q;
        st = g2_read_compressed(pr + 48, q);
        if (st == PT_OK && !g2_in_subgroup(q)) st = PT_NOT_IN_SUBGROUP;
        b[i] = q;
    } else if (what >= 3) {
        G1Affine p;
        st = g1_read_compressed(pr + (what == 3 ? 0 : 144), p);
        st = st == PT_OK && !g1_in_subgroup(p) ? PT_NOT_IN_SUBGROUP : 0;   // (decoding errors are reported by the lanes of y = 0 / 1)
    } else {
        G1Affine p;
        st = g1_read_compressed(pr + (what == 0 ? 0 : 144), p);
        G1Xyzz m = (st & ~PT_INFINITY) ? xyzz_inf<FpOps>() : xyzz_mul_scalar(xyzz_from_affine(p), k);
        if (what == 0)
            za[i] = xyzz_to_affine<FpOps, true>(m);
        else
            zc[i] = m;
    }
    if (st) atomicOr(status + i, st);
}

// sum of the n points zc[] (one workgroup of 256 lanes: strided serial sums, then an LDS tree), written as an uncompressed
// affine point (96 bytes, bellman wire format) for the host
__global__ void __launch_bounds__(256) k_g1_sum_export(const G1Xyzz* __restrict__ zc, uint32_t n, uint8_t* __restrict__ out96) {
    __shared__ G1Xyzz sh[256];
    const uint32_t tid = threadIdx.x;
    G1Xyzz acc = xyzz_inf<FpOps>();
    for (uint32_t k = tid; k < n; k += 256) xyzz_add_nc(acc, zc[k]);
    for (uint32_t d = 128; d >= 1; d >>= 1) {
        sh[tid] = acc;
        __syncthreads();
        if (tid < d) xyzz_add_nc(acc, sh[tid + d]);
        __syncthreads();
    }
    if (tid == 0) g1_write_uncompressed(xyzz_to_affine<FpOps, true>(acc), out96);
}

// ---- stage 2: Miller loops, one wave per pair -------------------------------------------------------------------------
// program word: op | dst << 2 | a << 12 | b << 22 ; steps[s] .. steps[s + 1] = the mutually independent operations of step s
struct PairingProgramDev {
    const uint32_t* ops;
    const uint32_t* steps;
    uint32_t n_steps;
};
__device__ __forceinline__ Fp slot_load(const uint32_t* sl, uint32_t s) {
    const uint4* q = reinterpret_cast<const uint4*>(sl + 12 * s);
    uint4 a = q[0], b = q[1], c = q[2];
    Fp r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    r.v[8] = c.x; r.v[9] = c.y; r.v[10] = c.z; r.v[11] = c.w;
    return r;
}
__device__ __forceinline__ void slot_store(uint32_t* sl, uint32_t s, const Fp& r) {
    uint4* q = reinterpret_cast<uint4*>(sl + 12 * s);
    q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
    q[2] = make_uint4(r.v[8], r.v[9], r.v[10], r.v[11]);
}
// the wave runs one program over its slots
__device__ __forceinline__ void run_program(const PairingProgramDev& P, uint32_t* sl, uint32_t lane) {
    uint32_t lo = P.steps[0];
    for (uint32_t s = 0; s < P.n_steps; ++s) {
        const uint32_t hi = P.steps[s + 1];
        for (uint32_t k = lo + lane; k < hi; k += 64) {
            const uint32_t w = P.ops[k], op = w & 3u, dst = (w >> 2) & 1023u, a = (w >> 12) & 1023u, b = (w >> 22) & 1023u;
            const Fp x = slot_load(sl, a);
            Fp r;
            if (op == 0u)
                r = fe_mul(x, slot_load(sl, b));
            else if (op == 1u)
                r = fe_add(x, slot_load(sl, b));
            else if (op == 2u)
                r = fe_sub(x, slot_load(sl, b));
            else
                r = x;
            slot_store(sl, dst, r);
        }
        // one wave: LDS operations execute in order; only the compiler must not move them across the step boundary
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        lo = hi;
    }
}
// slot numbers: host/pairing_prog.h (SLOT_ZERO 0, SLOT_F 1..12, SLOT_T 13..18, SLOT_P 19..20, SLOT_Q 21..24)
__global__ void __launch_bounds__(64) k_miller_pairs(PairingProgramDev dbl, PairingProgramDev add, uint32_t n_slots, const G1Affine* __restrict__ Pp,
                                                     const G2Affine* __restrict__ Qp, Fp* __restrict__ out) {
    extern __shared__ uint4 pairing_lds[];
    uint32_t* sl = reinterpret_cast<uint32_t*>(pairing_lds);
    const uint32_t lane = threadIdx.x, pair = blockIdx.x;
    const G1Affine P = Pp[pair];
    const G2Affine Q = Qp[pair];
    Fp* o = out + 12 * (size_t)pair;
    const Fp one = fe_one<FpCfg>(), zero = fe_zero<FpCfg>();
    if (aff_is_inf(P) || aff_is_inf(Q)) {  // a pair with a point at infinity contributes 1
        if (lane < 12) o[lane] = lane == 0 ? one : zero;
        return;
    }
    for (uint32_t s = lane; s < n_slots; s += 64) slot_store(sl, s, zero);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
        slot_store(sl, 1, one);  // f = 1
        slot_store(sl, 13, Q.x.c0); slot_store(sl, 14, Q.x.c1); slot_store(sl, 15, Q.y.c0); slot_store(sl, 16, Q.y.c1); slot_store(sl, 17, one);  // T = Q
        slot_store(sl, 19, P.x); slot_store(sl, 20, P.y);
        slot_store(sl, 21, Q.x.c0); slot_store(sl, 22, Q.x.c1); slot_store(sl, 23, Q.y.c0); slot_store(sl, 24, Q.y.c1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint64_t xabs = 0xd201000000010000ull;  // |x| of BLS12-381; the value is conjugated at the end because x < 0
    for (int bit = 62; bit >= 0; --bit) {
        run_program(dbl, sl, lane);  // f <- f^2 l_{T,T}(P), T <- 2T   (squaring f = 1 in the first round is harmless)
        if ((xabs >> bit) & 1) run_program(add, sl, lane);
    }
    if (lane < 12) {
        Fp v = slot_load(sl, 1 + lane);
        o[lane] = lane >= 6 ? fe_neg(v) : v;  // conj: the w-part negated
    }
}

// ---- stage 3: product of the Miller values ---------------------------------------------------------------------------------
// wave w multiplies vals[w], vals[w + stride], vals[w + 2 stride], ... (12 Fp each) into vals[w]
__global__ void __launch_bounds__(64) k_fp12_product(PairingProgramDev mul12, uint32_t n_slots, Fp* __restrict__ vals, uint32_t n, uint32_t stride) {
    extern __shared__ uint4 pairing_lds[];
    uint32_t* sl = reinterpret_cast<uint32_t*>(pairing_lds);
    const uint32_t lane = threadIdx.x, w = blockIdx.x;
    if (w >= n) return;
    const Fp zero = fe_zero<FpCfg>();
    for (uint32_t s = lane; s < n_slots; s += 64) slot_store(sl, s, zero);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 12) slot_store(sl, 1 + lane, vals[12 * (size_t)w + lane]);
    for (uint32_t k = w + stride; k < n; k += stride) {
        if (lane < 12) slot_store(sl, 13 + lane, vals[12 * (size_t)k + lane]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        run_program(mul12, sl, lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 12) vals[12 * (size_t)w + lane] = slot_load(sl, 1 + lane);
}

// ---- per-proof verdicts (masp_hip_verify_each) ------------------------------------------------------------------------------
// Per proof i three pairs, at 3 i .. 3 i + 2 of the pair arrays k_miller_pairs runs over:  (A_i, B_i)  (-acc_i, gamma)  (-C_i, delta)
//   k_verify_decode    one lane per point: A, B, C from the 192 proof bytes with Proof::read's refusals (no multiples: nothing is
//                      randomised when every proof gets a verdict of its own); gamma and delta are written next to B
//   k_verify_acc       one lane per proof: the inputs' range check and -acc_i = -(IC_0 + sum_j x_ij IC_j) in affine form
//   k_final_exp        one WAVE per proof: the product of its three Miller values and conj(alpha_beta), then the final
//                      exponentiation as the host's schedule over the host's programs (host/pairing_prog.h), compared with one
// verdict bytes: 1 the pairing equation holds, 0 it fails, 2 Proof::read refuses the proof, 3 a public input >= r (2 before 3)
enum : uint8_t { VERDICT_INVALID = 0, VERDICT_VALID = 1, VERDICT_PROOF_ENCODING = 2, VERDICT_INPUT_RANGE = 3 };

__global__ void __launch_bounds__(64) k_verify_decode(const uint8_t* __restrict__ proofs, uint32_t n, const G2Affine* __restrict__ gamma_delta,
                                                      G1Affine* __restrict__ Pp, G2Affine* __restrict__ Qp, int* __restrict__ status) {
    // gridDim.y = 3: y = 0 -> A, 1 -> B (the longest chain: a square root in Fp2), 2 -> C, each with its subgroup test
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, what = blockIdx.y;
    if (i >= n) return;
    const uint8_t* pr = proofs + 192 * (size_t)i;
    int st;
    if (what == 1) {
        G2Affine q;
        st = g2_read_compressed(pr + 48, q);
        if (st == PT_OK && !g2_in_subgroup(q)) st = PT_NOT_IN_SUBGROUP;
        if (st) q = {Fp2Ops::zero(), Fp2Ops::zero()};  // a refused proof's pairs contribute 1 and its verdict never reads them
        Qp[3 * (size_t)i] = q;
        Qp[3 * (size_t)i + 1] = gamma_delta[0];
        Qp[3 * (size_t)i + 2] = gamma_delta[1];
    } else {
        G1Affine p;
        st = g1_read_compressed(pr + (what == 0 ? 0 : 144), p);
        if (st == PT_OK && !g1_in_subgroup(p)) st = PT_NOT_IN_SUBGROUP;
        if (st)
            p = {fe_zero<FpCfg>(), fe_zero<FpCfg>()};
        else if (what == 2)
            p.y = fe_neg(p.y);
        Pp[3 * (size_t)i + what] = p;
    }
    if (st) atomicOr(status + i, st);
}

// inputs: n x n_public x 32 B little-endian; ic0: IC_0; tab: per input j the 64 x 15 affine points d 16^w IC_j+1 at [(64 j + w) 15 + d - 1]
// (the identity as x = y = 0).  At most 64 n_public mixed additions and no doubling per proof; xyzz_madd is exact for P + P, P - P and
// the identity on either side.  pre[i]: 0 = go on to the pairing, or the verdict the proof already has.
__global__ void __launch_bounds__(64) k_verify_acc(const uint8_t* __restrict__ inputs, uint32_t n, uint32_t n_public, const G1Affine* __restrict__ ic0,
                                                   const G1Affine* __restrict__ tab, const int* __restrict__ status, G1Affine* __restrict__ Pp,
                                                   uint8_t* __restrict__ pre) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool refused = (status[i] & (PT_BAD_FLAGS | PT_NOT_CANONICAL | PT_NOT_IN_SUBGROUP | PT_INFINITY)) != 0;
    auto word = [&](uint32_t j, uint32_t k) {
        const uint8_t* b = inputs + 32 * ((size_t)i * n_public + j) + 4 * k;
        return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    };
    bool in_range = true;
    for (uint32_t j = 0; j < n_public; ++j) {
        Fr x;
#pragma unroll
        for (int k = 0; k < 8; ++k) x.v[k] = word(j, k);
        if (fe_canonical_ge_mod(x)) in_range = false;
    }
    pre[i] = refused ? VERDICT_PROOF_ENCODING : in_range ? 0 : VERDICT_INPUT_RANGE;
    G1Affine out = {fe_zero<FpCfg>(), fe_zero<FpCfg>()};
    if (!refused && in_range) {
        G1Xyzz acc = xyzz_from_affine(ic0[0]);
        for (uint32_t j = 0; j < n_public; ++j)
            for (uint32_t k = 0; k < 8; ++k) {
                uint32_t w = word(j, k);
                for (uint32_t d4 = 0; w; ++d4, w >>= 4)  // zero digits are skipped, and so is the rest of a word once it is zero
                    if (w & 15u) xyzz_madd_nc(acc, tab[((size_t)64 * j + 8 * k + d4) * 15 + (w & 15u) - 1], false);
            }
        out = xyzz_to_affine<FpOps>(acc);
        out.y = fe_neg(out.y);  // (the identity stays x = y = 0: its pair contributes 1)
    }
    Pp[3 * (size_t)i + 1] = out;
}

// the final exponentiation's programs and schedule on the device (host/pairing_prog.h: FinalExpPrograms, final_exp_schedule,
// final_exp_constants); prog[]: mul, sq, frob, frob2, inv1, inv2
struct FinalExpDev {
    const PairingProgramDev* prog;
    const uint32_t* sched;
    uint32_t n_sched;
    uint32_t n_slots;
    const Fp* consts;  // 15, for slots 25 .. 39
};
__device__ __forceinline__ void wave_step() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// One wave per item.  f_i = vals[per i] * ... * vals[per i + per - 1] (* tail[0..11] if tail), 12 Fp each; verdict[i] = 1 if
// f_i^(3 (p^12 - 1) / r) is one, else 0 — also for f_i of norm zero (f_i = 0), which branches off before the inversion.
// pre (may be null): a non-zero pre[i] is item i's verdict already and its wave does nothing else.  out (may be null): the power,
// 12 Fp per item (zeros for norm zero or a non-zero pre).  Slot numbers: host/pairing_prog.h (F 1..12, Y 13..24, FE_N 21).
__global__ void __launch_bounds__(64) k_final_exp(FinalExpDev fe, const Fp* __restrict__ vals, uint32_t per, const Fp* __restrict__ tail,
                                                  const uint8_t* __restrict__ pre, Fp* __restrict__ out, uint8_t* __restrict__ verdict) {
    extern __shared__ uint4 pairing_lds[];
    uint32_t* sl = reinterpret_cast<uint32_t*>(pairing_lds);
    const uint32_t lane = threadIdx.x;
    const size_t item = blockIdx.x;
    const Fp zero = fe_zero<FpCfg>();
    const uint8_t early = pre ? pre[item] : (uint8_t)0;
    if (early) {
        if (lane == 0) verdict[item] = early;
        if (out && lane < 12) out[12 * item + lane] = zero;
        return;
    }
    for (uint32_t s = lane; s < fe.n_slots; s += 64) slot_store(sl, s, zero);
    wave_step();
    const Fp* v = vals + 12 * per * item;
    if (lane < 12) slot_store(sl, 1 + lane, v[lane]);
    if (lane >= 16 && lane < 31) slot_store(sl, 25 + (lane - 16), fe.consts[lane - 16]);
    const PairingProgramDev mul = fe.prog[0];
    for (uint32_t k = 1; k <= per; ++k) {
        if (k == per && !tail) break;
        if (lane < 12) slot_store(sl, 13 + lane, k == per ? tail[lane] : v[12 * k + lane]);
        wave_step();
        run_program(mul, sl, lane);
    }
    wave_step();
    for (uint32_t t = 0; t < fe.n_sched; ++t) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(fe.sched[t]);
        const uint32_t kind = w & 3u, a = (w >> 2) & 1023u, b = (w >> 12) & 1023u;
        if (kind == 0u) {
            run_program(fe.prog[a], sl, lane);  // (ends on a wave_step of its own)
            continue;
        }
        if (kind == 1u) {  // 12 slots from b to a, the w-half negated if asked
            if (lane < 12) {
                Fp x = slot_load(sl, b + lane);
                if (((w >> 22) & 1u) && lane >= 6) x = fe_neg(x);
                slot_store(sl, a + lane, x);
            }
        } else if (kind == 2u) {
            if (lane >= 6 && lane < 12) slot_store(sl, 1 + lane, fe_neg(slot_load(sl, 1 + lane)));
        } else {
            const Fp nrm = slot_load(sl, 21);
            if (fe_is_zero(nrm)) {  // wave-uniform: no inverse, the verdict is "invalid"
                if (lane == 0) verdict[item] = VERDICT_INVALID;
                if (out && lane < 12) out[12 * item + lane] = zero;
                return;
            }
            wave_step();  // every lane has read the norm before lane 0 replaces it
            if (lane == 0) slot_store(sl, 21, fe_inv_bingcd_nc(nrm));
        }
        wave_step();
    }
    bool same = true;
    if (lane < 12) {
        const Fp x = slot_load(sl, 1 + lane);
        same = fe_eq(x, lane == 0 ? fe_one<FpCfg>() : zero);
        if (out) out[12 * item + lane] = x;
    }
    const bool all_same = __all(same);
    if (lane == 0) verdict[item] = all_same ? VERDICT_VALID : VERDICT_INVALID;
}

}  // namespace masp
