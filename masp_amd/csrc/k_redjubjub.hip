// RedJubjub batch verification on the GPU and the Jubjub multi-scalar sum under it: the C ABI entry points masp_hip_jubjub_msm and
// masp_hip_redjubjub_verify_batch (include/masp_hip.h).  The latter replaces `signatures.verify(rng)` of BatchValidator::validate
// (masp_proofs/src/sapling/verifier/batch.rs:213): redjubjub::batch::Verifier over the spend-authorisation items
// queued at batch.rs:100-113 and the binding items of :188-200.
//
// Device (device/jubjub.hpp): k_jj_scale decodes one point per lane with the host's ZIP 216 rules, multiplies it by its scalar and
// sums its workgroup's products in LDS; k_jj_sum, a second launch, adds the workgroups' sums and writes the encoding of the total (or
// of [8] total) and whether that is the identity.  Host: H* (BLAKE2b-512), the coefficients z_i c_i and -sum z_i s_i mod r_J, s_i < r_J.
#include <mutex>

#include "device/jubjub.hpp"
#include "host/blake2b.h"
#include "host/jubjub.h"
#include "internal.h"

using namespace masp;

namespace {

constexpr uint32_t JJ_BLOCK = 256;
constexpr size_t JJ_MAX_POINTS = (size_t)1 << 22;   // masp_hip_jubjub_msm; a signature batch of 2^20 items sums 2^21 + 2 points

__global__ __launch_bounds__(JJ_BLOCK) void k_jj_scale(const uint4* __restrict__ points, const uint4* __restrict__ scalars, uint32_t n,
                                                       int* __restrict__ status, JExt* __restrict__ partial) {
    __shared__ JExt sh[JJ_BLOCK];
    const uint32_t t = threadIdx.x, i = blockIdx.x * JJ_BLOCK + t;
    JExt acc = jj_identity();
    if (i < n) {
        const uint4 p0 = points[2 * i], p1 = points[2 * i + 1], k0 = scalars[2 * i], k1 = scalars[2 * i + 1];
        const uint32_t w[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const uint32_t k[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
        JExt p;
        const int rc = jj_decode(p, w);
        status[i] = rc;
        if (rc == JJ_OK) acc = jj_mul(p, k);
    }
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = JJ_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = jj_add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = sh[0];
}

// out[0..7] = the encoding of the sum of nb partial sums (times 8 if `cofactor`), out[8] = 1 if that is the identity
__global__ __launch_bounds__(JJ_BLOCK) void k_jj_sum(const JExt* __restrict__ partial, uint32_t nb, int cofactor, uint32_t* __restrict__ out) {
    __shared__ JExt sh[JJ_BLOCK];
    const uint32_t t = threadIdx.x;
    JExt acc = jj_identity();
    for (uint32_t b = t; b < nb; b += JJ_BLOCK) acc = jj_add(acc, partial[b]);
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = JJ_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = jj_add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) {
        JExt r = sh[0];
        if (cofactor) r = jj_mul_by_cofactor(r);
        uint32_t w[8];
        jj_encode(w, r);
        for (int i = 0; i < 8; ++i) out[i] = w[i];
        out[8] = jj_is_identity(r) ? 1u : 0u;
    }
}

// sum_i [scalars_i] points_i over m >= 1 points (m x 32 bytes each) on the context's verifier stream.  status (m): 0 or why point i
// does not decode (its product is left out of the sum); out9: the encoding of the sum, or of [8] sum with `cofactor`, and the identity flag.
// Caller: ctx->mu shared, ctx->jj.mu held.
int jj_msm_run(masp_hip_ctx* ctx, size_t m, const uint8_t* points, const uint8_t* scalars, int cofactor, std::vector<int>& status, uint32_t out9[9]) {
    JubjubState& jj = ctx->jj;
    hipStream_t s = ctx->streams.vk[1];
    const uint32_t mm = (uint32_t)m, nb = (mm + JJ_BLOCK - 1) / JJ_BLOCK;
    int rc;
    if ((rc = jj.points.upload(points, 32 * m, s)) || (rc = jj.scalars.upload(scalars, 32 * m, s)) || (rc = jj.status.reserve(m)) ||
        (rc = jj.partial.reserve(sizeof(JExt) * nb)) || (rc = jj.out.reserve(9)))
        return rc;
    MASP_LAUNCH(k_jj_scale, dim3(nb), dim3(JJ_BLOCK), 0, s, (const uint4*)jj.points.p, (const uint4*)jj.scalars.p, mm, jj.status.p, (JExt*)jj.partial.p);
    MASP_LAUNCH(k_jj_sum, dim3(1), dim3(JJ_BLOCK), 0, s, (const JExt*)jj.partial.p, nb, cofactor, jj.out.p);
    status.resize(m);
    if (hipMemcpyAsync(status.data(), jj.status.p, sizeof(int) * m, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(out9, jj.out.p, 9 * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("jubjub multi-scalar sum failed: ") + hipGetErrorString(hipGetLastError());
        return MASP_HIP_E_HIP;
    }
    return launch_status();  // a refused launch: the buffers read back mean nothing
}

// ---- the Jubjub scalar field (order r_J of the prime-order subgroup: RjCfg, device/jubjub.hpp), host-side Montgomery arithmetic through
// field.hpp's host forms ----
typedef Fe<RjCfg> Rj;

// One lane per signature, no sum across lanes: items[i] = Rbar | vk | c | S (4 x 32 bytes; c = H*(Rbar || vk || sighash) reduced mod
// r_J by the host), kinds[i] picks one of the two basepoint encodings at `bases`.  verdict[i] = 1 iff Rbar and vk decode (ZIP 216),
// S < r_J and [8] (R + [c] vk - [S] G) = O: PublicKey::verify.  [c] vk - [S] G is one double-and-add over both scalars (the doublings
// are shared; the three possible addends vk, -G, vk - G are ready before the loop), with the scalars shifted out of registers as in jj_mul.
__global__ __launch_bounds__(64) void k_jj_verify_each(const uint4* __restrict__ items, const uint8_t* __restrict__ kinds, const uint4* __restrict__ bases,
                                                       uint32_t n, uint8_t* __restrict__ verdict) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto words = [](const uint4* p, uint32_t* w) {
        const uint4 a = p[0], b = p[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    };
    uint32_t w[8], c[8], sc[8];
    JExt R, vk, G;
    words(items + 8 * (size_t)i, w);
    bool ok = jj_decode(R, w) == JJ_OK;
    words(items + 8 * (size_t)i + 2, w);
    ok = (jj_decode(vk, w) == JJ_OK) && ok;
    words(items + 8 * (size_t)i + 4, c);
    words(items + 8 * (size_t)i + 6, sc);
    // (rj_is_canonical(sc) says the same; written out because the kernel's code is then what it has been, instruction for instruction)
    bool s_ge = true;   // S >= r_J, decided at the first word that differs from the top
    for (int k = 7; k >= 0; --k)
        if (sc[k] != RjCfg::MOD[k]) {
            s_ge = sc[k] > RjCfg::MOD[k];
            break;
        }
    ok = ok && !s_ge;
    words(bases + 2 * (kinds[i] ? 1 : 0), w);
    ok = (jj_decode(G, w) == JJ_OK) && ok;
    if (!ok) {
        verdict[i] = 0;
        return;
    }
    const JExt nG = {fe_neg(G.U), G.V, G.Z, fe_neg(G.T)}, both = jj_add(vk, nG);
    JExt r = jj_identity();
    for (int bit = 0; bit < 256; ++bit) {
        const uint32_t cb = c[7] >> 31, sb = sc[7] >> 31;
#pragma unroll
        for (int k = 7; k > 0; --k) {
            c[k] = (c[k] << 1) | (c[k - 1] >> 31);
            sc[k] = (sc[k] << 1) | (sc[k - 1] >> 31);
        }
        c[0] <<= 1;
        sc[0] <<= 1;
        r = jj_dbl(r);
        if (cb | sb) r = jj_add(r, cb && sb ? both : cb ? vk : nG);
    }
    verdict[i] = jj_is_identity(jj_mul_by_cofactor(jj_add(r, R))) ? 1 : 0;
}

Rj rj_words(const uint8_t* le32) {
    Rj a;
    memcpy(a.v, le32, 32);   // (little-endian host)
    return a;
}
// any 256-bit integer -> the Montgomery form of its residue (a < 2^256 = R and R2 < r_J keep CIOS below 2 r_J)
Rj rj_mont(const uint8_t* le32) {
    Rj r2;
    memcpy(r2.v, RjCfg::R2, 32);
    return fe_mul(rj_words(le32), r2);
}
void rj_store(uint8_t* le32, const Rj& mont) {
    Rj one = fe_zero<RjCfg>();
    one.v[0] = 1;
    const Rj c = fe_mul(mont, one);
    memcpy(le32, c.v, 32);
}
// c = H*(Rbar || vk || sighash) = BLAKE2b-512 personalised "MASP__RedJubjubH", the 512-bit digest reduced mod r_J (Montgomery form)
Rj h_star(const uint8_t* rbar, const uint8_t* vk, const uint8_t* sighash) {
    masp_host::Blake2b h((const uint8_t*)"MASP__RedJubjubH");
    h.update(rbar, 32);
    h.update(vk, 32);
    h.update(sighash, 32);
    uint8_t d[64];
    h.finalize(d);
    Rj r2;
    memcpy(r2.v, RjCfg::R2, 32);
    return fe_add(rj_mont(d), fe_mul(rj_mont(d + 32), r2));   // lo + hi 2^256: mont(hi 2^256) = mont(hi) R^2 / R
}

// the two basepoints' encodings: spending_key_generator, value_commitment_randomness_generator
const uint8_t* basepoints() {
    static const std::array<uint8_t, 64> b = [] {
        std::array<uint8_t, 64> x;
        masp_host::generators().spending_key.to_bytes(x.data());
        masp_host::generators().value_commitment_randomness.to_bytes(x.data() + 32);
        return x;
    }();
    return b.data();
}

}  // namespace

extern "C" {

int masp_hip_jubjub_msm(masp_hip_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* scalars, uint8_t out32[32], int64_t* bad_index) {
    if (bad_index) *bad_index = -1;
    if (!ctx || !out32 || (n && (!points || !scalars)) || n > JJ_MAX_POINTS) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) {
        memset(out32, 0, 32);
        out32[0] = 1;   // the identity (0, 1)
        return MASP_HIP_OK;
    }
    ApiCall call(ctx, CtxLock::SHARED);   // concurrent with provers and verifiers
    std::lock_guard<std::mutex> jlock(call.ctx->jj.mu);
    std::vector<int> status;
    uint32_t out9[9];
    int rc = jj_msm_run(call.ctx, n, points, scalars, 0, status, out9);
    if (rc) return call.done(rc);
    for (size_t i = 0; i < n; ++i)
        if (status[i]) {
            if (bad_index) *bad_index = (int64_t)i;
            return call.done(MASP_HIP_E_POINT_ENCODING);
        }
    memcpy(out32, out9, 32);
    return call.done(MASP_HIP_OK);
}

int masp_hip_redjubjub_verify_batch(masp_hip_ctx* ctx, size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* sighashes,
                                    const uint8_t* kinds, const uint8_t* z, int* all_valid) {
    if (!ctx || !all_valid || (n && (!vks || !sigs || !sighashes || !kinds || !z)) || n > (1u << 20)) return MASP_HIP_E_INVALID_ARG;
    *all_valid = 0;
    for (size_t i = 0; i < n; ++i)
        if (kinds[i] > 1) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) {
        *all_valid = 1;
        return MASP_HIP_OK;
    }
    // host: points R_0 .. R_n-1, vk_0 .. vk_n-1, G_spend_auth, G_binding with scalars z_i, z_i c_i, -sum z_i s_i per basepoint
    const size_t m = 2 * n + 2;
    std::vector<uint8_t> pts(32 * m), sc(32 * m, 0);
    Rj acc[2] = {fe_zero<RjCfg>(), fe_zero<RjCfg>()};
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *sig = sigs + 64 * i, *vk = vks + 32 * i;
        const Rj s = rj_words(sig + 32);
        if (fe_canonical_ge_mod(s)) return MASP_HIP_OK;   // S >= r_J: not a signature (*all_valid stays 0)
        uint8_t zi[32] = {0};
        memcpy(zi, z + 16 * i, 16);
        zi[0] |= 1;   // never zero (as masp_hip_verify_batch): an item with z = 0 would drop out of the check
        const Rj zm = rj_mont(zi);
        memcpy(&pts[32 * i], sig, 32);
        memcpy(&pts[32 * (n + i)], vk, 32);
        memcpy(&sc[32 * i], zi, 32);
        rj_store(&sc[32 * (n + i)], fe_mul(zm, h_star(sig, vk, sighashes + 32 * i)));
        acc[kinds[i]] = fe_add(acc[kinds[i]], fe_mul(zm, rj_mont(sig + 32)));
    }
    memcpy(&pts[32 * 2 * n], basepoints(), 64);
    rj_store(&sc[32 * 2 * n], fe_neg(acc[0]));
    rj_store(&sc[32 * (2 * n + 1)], fe_neg(acc[1]));
    ApiCall call(ctx, CtxLock::SHARED);
    std::lock_guard<std::mutex> jlock(call.ctx->jj.mu);
    std::vector<int> status;
    uint32_t out9[9];
    int rc = jj_msm_run(call.ctx, m, pts.data(), sc.data(), 1, status, out9);
    if (rc) return call.done(rc);
    for (int st : status)
        if (st) return call.done(MASP_HIP_OK);   // an R or vk that does not decode: not valid
    *all_valid = out9[8] == 1;
    return call.done(MASP_HIP_OK);
}

int masp_hip_redjubjub_verify_each(masp_hip_ctx* ctx, size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* sighashes,
                                   const uint8_t* kinds, uint8_t* verdicts) {
    if (!ctx || (n && (!vks || !sigs || !sighashes || !kinds || !verdicts)) || n > (1u << 20)) return MASP_HIP_E_INVALID_ARG;
    for (size_t i = 0; i < n; ++i)
        if (kinds[i] > 1) return MASP_HIP_E_INVALID_ARG;
    if (n == 0) return MASP_HIP_OK;
    // host: c_i = H*(Rbar_i || vk_i || sighash_i); items Rbar | vk | c | S, then the two basepoints
    std::vector<uint8_t> items(128 * n + 64);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *sig = sigs + 64 * i, *vk = vks + 32 * i;
        uint8_t* it = &items[128 * i];
        memcpy(it, sig, 32);
        memcpy(it + 32, vk, 32);
        rj_store(it + 64, h_star(sig, vk, sighashes + 32 * i));
        memcpy(it + 96, sig + 32, 32);
    }
    memcpy(&items[128 * n], basepoints(), 64);
    ApiCall call(ctx, CtxLock::SHARED);
    JubjubState& jj = call.ctx->jj;
    std::lock_guard<std::mutex> jlock(jj.mu);
    hipStream_t s = call.ctx->streams.vk[1];
    const uint32_t nn = (uint32_t)n;
    int rc;
    if ((rc = jj.points.upload(items.data(), items.size(), s)) || (rc = jj.scalars.upload(kinds, n, s)) || (rc = jj.partial.reserve(n))) return call.done(rc);
    MASP_LAUNCH(k_jj_verify_each, dim3((nn + 63) / 64), dim3(64), 0, s, (const uint4*)jj.points.p, (const uint8_t*)jj.scalars.p,
                (const uint4*)(jj.points.p + 128 * n), nn, jj.partial.p);
    if (hipMemcpyAsync(verdicts, jj.partial.p, n, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("per-signature verification failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    return call.done(MASP_HIP_OK);  // (a refused launch: the bytes read back mean nothing — done() asks)
}

}  // extern "C"
