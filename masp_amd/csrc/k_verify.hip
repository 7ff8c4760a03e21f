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
    // masp_hip_verify_each (built by its first call, under mu): the final exponentiation's programs, schedule and constants, the
    // key's own points in device form, and that call's work buffers
    bool each_ready = false, each_lds_ok = false;
    DevBuf<uint32_t> fe_ops, fe_steps, fe_sched;
    DevBuf<PairingProgramDev> fe_prog;
    DevBuf<Fp> fe_consts;          // 15 Frobenius constants, then conj(alpha_beta)
    DevBuf<G2Affine> d_gamma_delta;
    DevBuf<G1Affine> d_ic;         // IC_0, then per input the 64 x 15 multiples d 16^w IC_j
    FinalExpDev fe{};
    DevBuf<uint8_t> d_inputs, d_pre, d_verdict;
    DevBuf<G1Affine> d_pp;
    DevBuf<G2Affine> d_qp;
    Event each_ev[6];              // around the stages of a chunk (masp_hip_verify_each_last_timing); created with the tables
    double each_ms[5] = {0, 0, 0, 0, 0};
    hipStream_t stream = nullptr;  // verification runs next to the provers' batches, on one of the context's two verifier streams (not owned:
                                   // masp_hip_ctx::streams — created and kept off the batch streams' hardware queues with the context)
    std::mutex mu;                 // one verification at a time per key
};

namespace {

constexpr size_t EACH_CHUNK = (size_t)1 << 16;  // proofs per pass of masp_hip_verify_each: bounds its scratch (2.6 KB per proof)

// what masp_hip_verify_each needs beyond the batch call's, uploaded once per key.  Caller: ctx->mu shared, vk->mu held, device set.
int prepare_each(masp_hip_ctx* ctx, masp_hip_vk* vk) {
    if (vk->each_ready) return MASP_HIP_OK;
    const FinalExpTables ft = final_exp_tables();
    Fp consts[15 + 12];
    memcpy(consts, ft.consts, sizeof(ft.consts));
    const masp_host::bls::Fp12 ab = vk->vk.alpha_beta.conj();
    memcpy(consts + 15, &ab, 12 * 48);
    const G2Affine gd[2] = {dev_g2(vk->vk.gamma), dev_g2(vk->vk.delta)};
    const std::vector<G1Affine> ic = ic_table(vk->vk);
    hipStream_t s = vk->stream;
    int rc;
    if ((rc = vk->fe_ops.upload(ft.ops.data(), ft.ops.size(), s)) || (rc = vk->fe_steps.upload(ft.steps.data(), ft.steps.size(), s)) ||
        (rc = vk->fe_sched.upload(ft.sched.data(), ft.sched.size(), s)) || (rc = vk->fe_consts.upload(consts, 27, s)) ||
        (rc = vk->d_gamma_delta.upload(gd, 2, s)) || (rc = vk->d_ic.upload(ic.data(), ic.size(), s)) || (rc = vk->fe_prog.reserve(6)))
        return rc;
    PairingProgramDev progs[6];
    for (int i = 0; i < 6; ++i) progs[i] = ft.dev(i, vk->fe_ops.p, vk->fe_steps.p);
    if ((rc = vk->fe_prog.upload(progs, 6, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));  // the host arrays above go out of scope
    vk->fe = {vk->fe_prog.p, vk->fe_sched.p, (uint32_t)ft.sched.size(), ft.n_slots, vk->fe_consts.p};
    if ((rc = create_events(vk->each_ev))) return rc;
    vk->each_lds_ok = hipFuncSetAttribute((const void*)k_final_exp, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    vk->each_ready = true;
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_vk_prepare(masp_hip_ctx* ctx, const uint8_t* params, size_t params_len, masp_hip_vk** out) {
    if (!ctx || !params || !out) return MASP_HIP_E_INVALID_ARG;
    *out = nullptr;
    ctx = FIRST_DEVICE(ctx);
    std::unique_ptr<masp_hip_vk> v(new masp_hip_vk);
    if (!masp_host::prepare_vk(v->vk, params, params_len)) return MASP_HIP_E_PARAMS_FORMAT;
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    v->device = ctx->device;
    const masp_host::prog::PairingPrograms& pp = masp_host::prog::pairing_programs();
    const masp_host::prog::Program* ps[3] = {&pp.dbl, &pp.add, &pp.mul12};
    std::vector<uint32_t> ops, steps;
    size_t op_off[3], st_off[3];
    for (int i = 0; i < 3; ++i) {
        op_off[i] = ops.size();
        st_off[i] = steps.size();
        for (uint32_t s : ps[i]->step_start) steps.push_back(s + (uint32_t)op_off[i]);  // absolute indices into the concatenation
        ops.insert(ops.end(), ps[i]->ops.begin(), ps[i]->ops.end());
    }
    int rc;
    hipStream_t s = ctx->streams.main;
    if ((rc = v->ops.upload(ops.data(), ops.size(), s)) || (rc = v->steps.upload(steps.data(), steps.size(), s))) return fail(ctx, rc);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(ctx, MASP_HIP_E_HIP);
    PairingProgramDev* dst[3] = {&v->dbl, &v->add, &v->mul12};
    for (int i = 0; i < 3; ++i) {
        dst[i]->ops = v->ops.p;
        dst[i]->steps = v->steps.p + st_off[i];
        dst[i]->n_steps = (uint32_t)ps[i]->step_start.size() - 1;
    }
    v->n_slots = pp.n_slots;
    v->lds_ok = hipFuncSetAttribute((const void*)k_miller_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess &&
                hipFuncSetAttribute((const void*)k_fp12_product, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    v->stream = ctx->streams.vk[ctx->vk_next.fetch_add(1) % 2];
    *out = v.release();
    return MASP_HIP_OK;
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
    const ApiLaunchScope api_scope;
    ctx = FIRST_DEVICE(ctx);
    if (ctx->device != vk->device) return MASP_HIP_E_INVALID_ARG;
    std::shared_lock<std::shared_mutex> lock(ctx->mu);  // concurrent with provers (and with verifications under other keys)
    std::lock_guard<std::mutex> vlock(vk->mu);
    hipSetDevice(ctx->device);
    hipStream_t s = vk->stream;
    const uint32_t nn = (uint32_t)n;
    DevBuf<uint8_t>&d_proofs = vk->d_proofs, &d_z = vk->d_z, &d_sum = vk->d_sum;
    DevBuf<G1Affine>& d_za = vk->d_za;
    DevBuf<G2Affine>& d_b = vk->d_b;
    DevBuf<G1Xyzz>& d_zc = vk->d_zc;
    DevBuf<int>& d_status = vk->d_status;
    DevBuf<Fp>& d_f = vk->d_f;
    int rc;
    if ((rc = d_proofs.upload(proofs, 192 * n, s)) || (rc = d_z.upload(z, 16 * n, s)) || (rc = d_za.reserve(n)) || (rc = d_b.reserve(n)) ||
        (rc = d_zc.reserve(n)) || (rc = d_status.reserve(n)) || (rc = d_f.reserve(12 * n)) || (rc = d_sum.reserve(96)))
        return fail(ctx, rc);
    HIP_TRY(hipMemsetAsync(d_status.p, 0, sizeof(int) * n, s));
    // the interpreter keeps its slots in LDS: n_slots x 48 bytes per wave
    const uint32_t lds = vk->n_slots * 48;
    if (!vk->lds_ok || lds > 64 * 1024) {
        last_hip_error() = "pairing interpreter: LDS configuration failed";
        return fail(ctx, MASP_HIP_E_HIP);
    }
    MASP_LAUNCH(k_verify_prepare, dim3((nn + 63) / 64, 5), dim3(64), 0, s, d_proofs.p, d_z.p, nn, d_za.p, d_b.p, d_zc.p, d_status.p);
    MASP_LAUNCH(k_g1_sum_export, dim3(1), dim3(256), 0, s, d_zc.p, nn, d_sum.p);
    MASP_LAUNCH(k_miller_pairs, dim3(nn), dim3(64), lds, s, vk->dbl, vk->add, vk->n_slots, d_za.p, d_b.p, d_f.p);
    launch_fp12_product(s, vk->mul12, vk->n_slots, lds, d_f.p, nn);
    std::vector<int> status(n);
    masp_host::bls::Fp12 f;
    uint8_t sum96[96];
    static_assert(sizeof(masp_host::bls::Fp12) == 12 * 48, "Fp12 is 12 packed Montgomery residues");
    if (hipMemcpyAsync(status.data(), d_status.p, sizeof(int) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&f, d_f.p, 12 * 48, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum96, d_sum.p, 96, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("batch verification failed: ") + hipGetErrorString(hipGetLastError());
        return fail(ctx, MASP_HIP_E_HIP);
    }
    if (launch_status() != MASP_HIP_OK) return fail(ctx, MASP_HIP_E_HIP);  // a refused launch: the buffers read back mean nothing
    for (int st : status)
        if (st & (PT_BAD_FLAGS | PT_NOT_CANONICAL | PT_NOT_IN_SUBGROUP | PT_INFINITY)) return MASP_HIP_OK;  // what Proof::read refuses (the identity included: "point at infinity"): not valid (*all_valid stays 0)
    masp_host::bls::G1A csum;
    if (!masp_host::bls::g1_uncompressed(csum, sum96)) {
        last_hip_error() = "batch verification: device returned a malformed point";
        return fail(ctx, MASP_HIP_E_HIP);
    }
    int v = masp_host::batch_verify_finish(vk->vk, n, public_inputs, n_public, z, f, csum);
    if (v < 0) return MASP_HIP_E_SCALAR_RANGE;
    *all_valid = v;
    return MASP_HIP_OK;
}

int masp_hip_verify_each(masp_hip_ctx* ctx, masp_hip_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint32_t n_public,
                         uint8_t* verdicts) {
    if (!ctx || !vk || (n && (!proofs || !verdicts || (n_public && !public_inputs))) || n > (1u << 20)) return MASP_HIP_E_INVALID_ARG;
    if ((size_t)n_public + 1 != vk->vk.ic.size()) return MASP_HIP_E_PARAMS_SHAPE;
    if (n == 0) return MASP_HIP_OK;
    const ApiLaunchScope api_scope;
    ctx = FIRST_DEVICE(ctx);
    if (ctx->device != vk->device) return MASP_HIP_E_INVALID_ARG;
    std::shared_lock<std::shared_mutex> lock(ctx->mu);  // concurrent with provers (and with verifications under other keys)
    std::lock_guard<std::mutex> vlock(vk->mu);
    hipSetDevice(ctx->device);
    hipStream_t s = vk->stream;
    int rc;
    if ((rc = prepare_each(ctx, vk))) return fail(ctx, rc);
    const uint32_t lds = vk->n_slots * 48, lds_fe = vk->fe.n_slots * 48;
    if (!vk->lds_ok || !vk->each_lds_ok || lds > 64 * 1024 || lds_fe > 64 * 1024) {
        last_hip_error() = "pairing interpreter: LDS configuration failed";
        return fail(ctx, MASP_HIP_E_HIP);
    }
    for (double& t : vk->each_ms) t = 0;
    for (size_t lo = 0; lo < n; lo += EACH_CHUNK) {
        const size_t m = std::min(EACH_CHUNK, n - lo);
        const uint32_t mm = (uint32_t)m;
        const Event* ev = vk->each_ev;
        HIP_TRY(hipEventRecord(ev[0], s));
        if ((rc = vk->d_proofs.upload(proofs + 192 * lo, 192 * m, s)) ||
            (rc = vk->d_inputs.upload(n_public ? public_inputs + 32 * (size_t)n_public * lo : nullptr, 32 * (size_t)n_public * m, s)) ||
            (rc = vk->d_status.reserve(m)) || (rc = vk->d_pp.reserve(3 * m)) || (rc = vk->d_qp.reserve(3 * m)) || (rc = vk->d_f.reserve(36 * m)) ||
            (rc = vk->d_pre.reserve(m)) || (rc = vk->d_verdict.reserve(m)))
            return fail(ctx, rc);
        HIP_TRY(hipMemsetAsync(vk->d_status.p, 0, sizeof(int) * m, s));
        MASP_LAUNCH(k_verify_decode, dim3((mm + 63) / 64, 3), dim3(64), 0, s, vk->d_proofs.p, mm, vk->d_gamma_delta.p, vk->d_pp.p, vk->d_qp.p, vk->d_status.p);
        HIP_TRY(hipEventRecord(ev[1], s));
        MASP_LAUNCH(k_verify_acc, dim3((mm + 63) / 64), dim3(64), 0, s, vk->d_inputs.p, mm, n_public, vk->d_ic.p, vk->d_ic.p + 1, vk->d_status.p, vk->d_pp.p,
                    vk->d_pre.p);
        HIP_TRY(hipEventRecord(ev[2], s));
        MASP_LAUNCH(k_miller_pairs, dim3(3 * mm), dim3(64), lds, s, vk->dbl, vk->add, vk->n_slots, vk->d_pp.p, vk->d_qp.p, vk->d_f.p);
        HIP_TRY(hipEventRecord(ev[3], s));
        MASP_LAUNCH(k_final_exp, dim3(mm), dim3(64), lds_fe, s, vk->fe, vk->d_f.p, 3u, vk->fe_consts.p + 15, vk->d_pre.p, (Fp*)nullptr, vk->d_verdict.p);
        HIP_TRY(hipEventRecord(ev[4], s));
        if (hipMemcpyAsync(verdicts + lo, vk->d_verdict.p, m, hipMemcpyDeviceToHost, s) != hipSuccess || hipEventRecord(ev[5], s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            last_hip_error() = std::string("per-proof verification failed: ") + hipGetErrorString(hipGetLastError());
            return fail(ctx, MASP_HIP_E_HIP);
        }
        if (launch_status() != MASP_HIP_OK) return fail(ctx, MASP_HIP_E_HIP);  // a refused launch: the bytes read back mean nothing
        (void)add_elapsed(ev, 5, vk->each_ms);
    }
    return MASP_HIP_OK;
}

int masp_hip_verify_each_last_timing(masp_hip_vk* vk, double ms[5]) {
    if (!vk || !ms) return MASP_HIP_E_INVALID_ARG;
    std::lock_guard<std::mutex> vlock(vk->mu);
    for (int k = 0; k < 5; ++k) ms[k] = vk->each_ms[k];
    return MASP_HIP_OK;
}

}  // extern "C"
