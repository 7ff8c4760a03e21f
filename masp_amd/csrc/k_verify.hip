// GPU Groth16 batch verification: the C ABI entry points masp_hip_vk_prepare / masp_hip_verify_batch (include/masp_hip.h),
// the kernels of device/pairing.hpp, and the host-side remainder (host/groth16_vk.h: public-input combination, two pairs,
// final exponentiation — work that does not grow with the batch).
// Replaces bellman `verify_proofs_batch` as reached from /root/reference/masp_proofs/src/sapling/verifier/batch.rs:24-31,201-239
// and the per-proof `verify_proof` self-checks of the prover (sapling/prover.rs:148,266) when they are batched.
#include <mutex>

#include "device/pairing.hpp"
#include "host/groth16_vk.h"
#include "host/pairing_prog.h"
#include "internal.h"
#include "verify_launch.h"

using namespace masp;

struct masp_hip_vk {
    masp_host::PreparedVk vk;
    int device = 0;
    DevBuf<uint32_t> ops, steps;  // the three programs, concatenated
    PairingProgramDev dbl{}, add{}, mul12{};
    uint32_t n_slots = 0;
    bool lds_ok = false;  // the interpreter kernels' LDS limit was raised on THIS key's device (the attribute is per device)
    // work buffers, grown on demand and kept (hipFree would synchronise the device under the provers)
    DevBuf<uint8_t> d_proofs, d_z, d_sum;
    DevBuf<G1Affine> d_za;
    DevBuf<G2Affine> d_b;
    DevBuf<G1Xyzz> d_zc;
    DevBuf<int> d_status;
    DevBuf<Fp> d_f;
    // what only masp_hip_verify_each uses (prepare_each, at its first call, under mu): the final exponentiation's programs, schedule and
    // constants, the key's own points in device form, and that call's work buffers
    struct Each {
        bool ready = false, lds_ok = false;
        DevBuf<uint32_t> fe_ops, fe_steps, fe_sched;
        DevBuf<PairingProgramDev> fe_prog;
        DevBuf<Fp> fe_consts;          // 15 Frobenius constants, then conj(alpha_beta)
        DevBuf<G2Affine> d_gamma_delta;
        DevBuf<G1Affine> d_ic;         // IC_0, then per input the 64 x 15 multiples d 16^w IC_j
        FinalExpDev fe{};
        DevBuf<uint8_t> d_inputs, d_pre, d_verdict;
        DevBuf<G1Affine> d_pp;
        DevBuf<G2Affine> d_qp;
        Event ev[6];                   // around the stages of a chunk (masp_hip_verify_each_last_timing); created with the tables
        double ms[5] = {0, 0, 0, 0, 0};
    } each;
    hipStream_t stream = nullptr;  // verification runs next to the provers' batches, on one of the context's two verifier streams (not owned:
                                   // masp_hip_ctx::streams — created and kept off the batch streams' hardware queues with the context)
    std::mutex mu;                 // one verification at a time per key
};

namespace {

constexpr size_t EACH_CHUNK = (size_t)1 << 16;  // proofs per pass of masp_hip_verify_each: bounds its scratch (2.6 KB per proof)

// what masp_hip_verify_each needs beyond the batch call's, uploaded once per key.  Caller: ctx->mu shared, vk->mu held, device set.
int prepare_each(masp_hip_vk* vk) {
    masp_hip_vk::Each& e = vk->each;
    if (e.ready) return MASP_HIP_OK;
    const FinalExpTables ft = final_exp_tables();
    Fp consts[15 + 12];
    memcpy(consts, ft.consts, sizeof(ft.consts));
    const masp_host::bls::Fp12 ab = vk->vk.alpha_beta.conj();
    memcpy(consts + 15, &ab, 12 * 48);
    const G2Affine gd[2] = {dev_g2(vk->vk.gamma), dev_g2(vk->vk.delta)};
    const std::vector<G1Affine> ic = ic_table(vk->vk);
    hipStream_t s = vk->stream;
    int rc;
    if ((rc = e.fe_ops.upload(ft.ops.data(), ft.ops.size(), s)) || (rc = e.fe_steps.upload(ft.steps.data(), ft.steps.size(), s)) ||
        (rc = e.fe_sched.upload(ft.sched.data(), ft.sched.size(), s)) || (rc = e.fe_consts.upload(consts, 27, s)) ||
        (rc = e.d_gamma_delta.upload(gd, 2, s)) || (rc = e.d_ic.upload(ic.data(), ic.size(), s)) || (rc = e.fe_prog.reserve(6)))
        return rc;
    PairingProgramDev progs[6];
    for (int i = 0; i < 6; ++i) progs[i] = ft.dev(i, e.fe_ops.p, e.fe_steps.p);
    if ((rc = e.fe_prog.upload(progs, 6, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));  // the host arrays above go out of scope
    e.fe = {e.fe_prog.p, e.fe_sched.p, (uint32_t)ft.sched.size(), ft.n_slots, e.fe_consts.p};
    if ((rc = create_events(e.ev))) return rc;
    e.lds_ok = hipFuncSetAttribute((const void*)k_final_exp, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    e.ready = true;
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_vk_prepare(masp_hip_ctx* ctx, const uint8_t* params, size_t params_len, masp_hip_vk** out) {
    if (!ctx || !params || !out) return MASP_HIP_E_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<masp_hip_vk> v(new masp_hip_vk);
    if (!masp_host::prepare_vk(v->vk, params, params_len)) return MASP_HIP_E_PARAMS_FORMAT;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    v->device = ctx->device;
    const ProgramTable pt = pairing_program_table();
    int rc;
    hipStream_t s = ctx->streams.main;
    if ((rc = v->ops.upload(pt.ops.data(), pt.ops.size(), s)) || (rc = v->steps.upload(pt.steps.data(), pt.steps.size(), s)) ||
        (rc = HIP_RC(hipStreamSynchronize(s))))
        return call.done(rc);
    v->dbl = pt.dev(0, v->ops.p, v->steps.p);
    v->add = pt.dev(1, v->ops.p, v->steps.p);
    v->mul12 = pt.dev(2, v->ops.p, v->steps.p);
    v->n_slots = pt.n_slots;
    v->lds_ok = hipFuncSetAttribute((const void*)k_miller_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess &&
                hipFuncSetAttribute((const void*)k_fp12_product, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    v->stream = ctx->streams.vk[ctx->vk_next.fetch_add(1) % 2];
    if ((rc = call.done(MASP_HIP_OK)) == MASP_HIP_OK) *out = v.release();
    return rc;
}

void masp_hip_vk_free(masp_hip_vk* vk) {
    if (!vk) return;
    hipSetDevice(vk->device);
    delete vk;
}

int masp_hip_verify_batch(masp_hip_ctx* ctx, masp_hip_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs,
                          uint32_t n_public, const uint8_t* z, int* all_valid) {
    if (!ctx || !vk || !all_valid || (n && (!proofs || !z || (n_public && !public_inputs))) || n > (1u << 20)) return MASP_HIP_E_INVALID_ARG;
    if ((size_t)n_public + 1 != vk->vk.ic.size()) return MASP_HIP_E_PARAMS_SHAPE;
    *all_valid = 0;
    if (n == 0) {
        *all_valid = 1;
        return MASP_HIP_OK;
    }
    if (FIRST_DEVICE(ctx)->device != vk->device) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::SHARED);  // concurrent with provers (and with verifications under other keys)
    std::lock_guard<std::mutex> vlock(vk->mu);
    hipStream_t s = vk->stream;
    const uint32_t nn = (uint32_t)n;
    int rc;
    if ((rc = vk->d_proofs.upload(proofs, 192 * n, s)) || (rc = vk->d_z.upload(z, 16 * n, s)) || (rc = vk->d_za.reserve(n)) ||
        (rc = vk->d_b.reserve(n)) || (rc = vk->d_zc.reserve(n)) || (rc = vk->d_status.reserve(n)) || (rc = vk->d_f.reserve(12 * n)) ||
        (rc = vk->d_sum.reserve(96)) || (rc = HIP_RC(hipMemsetAsync(vk->d_status.p, 0, sizeof(int) * n, s))))
        return call.done(rc);
    // the interpreter keeps its slots in LDS: n_slots x 48 bytes per wave
    const uint32_t lds = vk->n_slots * 48;
    if (!vk->lds_ok || lds > 64 * 1024) {
        last_hip_error() = "pairing interpreter: LDS configuration failed";
        return call.done(MASP_HIP_E_HIP);
    }
    MASP_LAUNCH(k_verify_prepare, dim3((nn + 63) / 64, 5), dim3(64), 0, s, vk->d_proofs.p, vk->d_z.p, nn, vk->d_za.p, vk->d_b.p, vk->d_zc.p, vk->d_status.p);
    MASP_LAUNCH(k_g1_sum_export, dim3(1), dim3(256), 0, s, vk->d_zc.p, nn, vk->d_sum.p);
    MASP_LAUNCH(k_miller_pairs, dim3(nn), dim3(64), lds, s, vk->dbl, vk->add, vk->n_slots, vk->d_za.p, vk->d_b.p, vk->d_f.p);
    launch_fp12_product(s, vk->mul12, vk->n_slots, lds, vk->d_f.p, nn);
    std::vector<int> status(n);
    masp_host::bls::Fp12 f;
    uint8_t sum96[96];
    static_assert(sizeof(masp_host::bls::Fp12) == 12 * 48, "Fp12 is 12 packed Montgomery residues");
    if (hipMemcpyAsync(status.data(), vk->d_status.p, sizeof(int) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&f, vk->d_f.p, 12 * 48, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum96, vk->d_sum.p, 96, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("batch verification failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    if ((rc = launch_status())) return call.done(rc);  // a refused launch: the buffers read back mean nothing
    for (int st : status)
        if (st & (PT_BAD_FLAGS | PT_NOT_CANONICAL | PT_NOT_IN_SUBGROUP | PT_INFINITY)) return call.done(MASP_HIP_OK);  // what Proof::read refuses (the identity included: "point at infinity"): not valid (*all_valid stays 0)
    masp_host::bls::G1A csum;
    if (!masp_host::bls::g1_uncompressed(csum, sum96)) {
        last_hip_error() = "batch verification: device returned a malformed point";
        return call.done(MASP_HIP_E_HIP);
    }
    int v = masp_host::batch_verify_finish(vk->vk, n, public_inputs, n_public, z, f, csum);
    if (v < 0) return call.done(MASP_HIP_E_SCALAR_RANGE);
    *all_valid = v;
    return call.done(MASP_HIP_OK);
}

int masp_hip_verify_each(masp_hip_ctx* ctx, masp_hip_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint32_t n_public,
                         uint8_t* verdicts) {
    if (!ctx || !vk || (n && (!proofs || !verdicts || (n_public && !public_inputs))) || n > (1u << 20)) return MASP_HIP_E_INVALID_ARG;
    if ((size_t)n_public + 1 != vk->vk.ic.size()) return MASP_HIP_E_PARAMS_SHAPE;
    if (n == 0) return MASP_HIP_OK;
    if (FIRST_DEVICE(ctx)->device != vk->device) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::SHARED);  // concurrent with provers (and with verifications under other keys)
    std::lock_guard<std::mutex> vlock(vk->mu);
    hipStream_t s = vk->stream;
    int rc;
    if ((rc = prepare_each(vk))) return call.done(rc);
    masp_hip_vk::Each& e = vk->each;
    const uint32_t lds = vk->n_slots * 48, lds_fe = e.fe.n_slots * 48;
    if (!vk->lds_ok || !e.lds_ok || lds > 64 * 1024 || lds_fe > 64 * 1024) {
        last_hip_error() = "pairing interpreter: LDS configuration failed";
        return call.done(MASP_HIP_E_HIP);
    }
    for (double& t : e.ms) t = 0;
    for (size_t lo = 0; lo < n; lo += EACH_CHUNK) {
        const size_t m = std::min(EACH_CHUNK, n - lo);
        const uint32_t mm = (uint32_t)m;
        const Event* ev = e.ev;
        if ((rc = HIP_RC(hipEventRecord(ev[0], s))) || (rc = vk->d_proofs.upload(proofs + 192 * lo, 192 * m, s)) ||
            (rc = e.d_inputs.upload(n_public ? public_inputs + 32 * (size_t)n_public * lo : nullptr, 32 * (size_t)n_public * m, s)) ||
            (rc = vk->d_status.reserve(m)) || (rc = e.d_pp.reserve(3 * m)) || (rc = e.d_qp.reserve(3 * m)) || (rc = vk->d_f.reserve(36 * m)) ||
            (rc = e.d_pre.reserve(m)) || (rc = e.d_verdict.reserve(m)) || (rc = HIP_RC(hipMemsetAsync(vk->d_status.p, 0, sizeof(int) * m, s))))
            return call.done(rc);
        MASP_LAUNCH(k_verify_decode, dim3((mm + 63) / 64, 3), dim3(64), 0, s, vk->d_proofs.p, mm, e.d_gamma_delta.p, e.d_pp.p, e.d_qp.p, vk->d_status.p);
        if ((rc = HIP_RC(hipEventRecord(ev[1], s)))) return call.done(rc);
        MASP_LAUNCH(k_verify_acc, dim3((mm + 63) / 64), dim3(64), 0, s, e.d_inputs.p, mm, n_public, e.d_ic.p, e.d_ic.p + 1, vk->d_status.p, e.d_pp.p, e.d_pre.p);
        if ((rc = HIP_RC(hipEventRecord(ev[2], s)))) return call.done(rc);
        MASP_LAUNCH(k_miller_pairs, dim3(3 * mm), dim3(64), lds, s, vk->dbl, vk->add, vk->n_slots, e.d_pp.p, e.d_qp.p, vk->d_f.p);
        if ((rc = HIP_RC(hipEventRecord(ev[3], s)))) return call.done(rc);
        MASP_LAUNCH(k_final_exp, dim3(mm), dim3(64), lds_fe, s, e.fe, vk->d_f.p, 3u, e.fe_consts.p + 15, e.d_pre.p, (Fp*)nullptr, e.d_verdict.p);
        if ((rc = HIP_RC(hipEventRecord(ev[4], s)))) return call.done(rc);
        if (hipMemcpyAsync(verdicts + lo, e.d_verdict.p, m, hipMemcpyDeviceToHost, s) != hipSuccess || hipEventRecord(ev[5], s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            last_hip_error() = std::string("per-proof verification failed: ") + hipGetErrorString(hipGetLastError());
            return call.done(MASP_HIP_E_HIP);
        }
        if ((rc = launch_status())) return call.done(rc);  // a refused launch: the bytes read back mean nothing
        (void)add_elapsed(ev, 5, e.ms);
    }
    return call.done(MASP_HIP_OK);
}

int masp_hip_verify_each_last_timing(masp_hip_vk* vk, double ms[5]) {
    if (!vk || !ms) return MASP_HIP_E_INVALID_ARG;
    std::lock_guard<std::mutex> vlock(vk->mu);
    for (int k = 0; k < 5; ++k) ms[k] = vk->each.ms[k];
    return MASP_HIP_OK;
}

}  // extern "C"
