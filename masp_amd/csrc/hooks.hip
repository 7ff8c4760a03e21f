// libmasp_hip: the MSM / NTT building-block entry points, the resident-batch measurement hooks and the profiling getters
// (include/masp_hip.h): what tests, tools and bench.py drive next to masp_hip_prove_batch.
#include "pipeline.h"

using namespace masp;

// ---- building blocks ----------------------------------------------------------------------------
// np MSMs over ONE base set (how a batch of proofs uses the engine: gridDim.y = np, one launch per stage):
// scalars np x n x 32 B, out np x BYTES uncompressed.  window_bits 0 = the engine's own choice for n.
template <class O, int BYTES>
static int msm_multi(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits, uint8_t* out,
                     int block_bits = 0, size_t sub_lo = 0, size_t sub_hi = (size_t)-1, uint32_t* bucket0_entries = nullptr) {
    if (!ctx || !out || !np || np > 256 || !n || !bases || !scalars || n > (1u << 22) || window_bits < 0 || window_bits == 1 || window_bits > 16)
        return MASP_HIP_E_INVALID_ARG;
    if (block_bits != 0 && block_bits != 2 && block_bits != 3) return MASP_HIP_E_INVALID_ARG;
    sub_lo = std::min(sub_lo, n);
    sub_hi = std::min(sub_hi, n);
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    hipStream_t s = ctx->streams.main;
    for (size_t i = 0; i < n * np; ++i)
        if (!rs_in_range(scalars + 32 * i)) return call.done(MASP_HIP_E_SCALAR_RANGE);
    MsmBases<O, BYTES> B;
    MsmWorkspace<O> ws;
    ws.tree_levels = ctx->opt.bucket_tree_levels;
    ws.tree_sub = (uint32_t)ctx->opt.bucket_tree_sub_batch;
    ws.tree.own.limit = (size_t)ctx->opt.bucket_tree_scratch_mb << 20;
    // (what lack of tree scratch does to this call's own workspace is reported like the slots': masp_hip_ctx_get_options)
    struct Report {
        masp_hip_ctx* c;
        MsmWorkspace<O>& w;
        ~Report() {
            c->block_tree_fallbacks += w.tree_fallbacks;
            c->block_tree_sub = std::min<uint32_t>(c->block_tree_sub, std::min(w.tree_sub ? w.tree_sub : 256u, w.tree_sub_used));
        }
    } report{ctx, ws};
    DevBuf<Xyzz<O>> res;
    DevBuf<uint8_t> d_out;
    int rc;
    // (doubled window rows only where the context was told to use them behind every table, masp_hip_ctx_set_window_row_multiples(ctx, 1):
    // by default this building block keeps the plain geometry, whose bucket 0 is the digits of magnitude 1 — what bucket0_entries reports)
    if ((rc = B.load_host(bases, (uint32_t)n, s, 0xffffffffu, window_bits, block_bits, (uint32_t)sub_lo, (uint32_t)sub_hi, ctx->twin_rows_msm)))
        return call.done(rc);
    if (B.import_status & (PT_BAD_FLAGS | PT_NOT_CANONICAL)) return call.done(MASP_HIP_E_PARAMS_FORMAT);
    if ((rc = ctx->tmp_scalars.upload((const Fr*)scalars, n * np, s)) || (rc = res.reserve(np)) || (rc = d_out.reserve(BYTES * np)) ||
        (rc = msm_enqueue(s, B, ws, (const uint32_t*)ctx->tmp_scalars.p, n * 8, res.p, 1, (uint32_t)np)))
        return call.done(rc);
    // the sort's packed offsets: dense[p][1] = entries of proof p's bucket 0 (digits of magnitude 1, unit scalars, boolean blocks)
    if (bucket0_entries && (rc = HIP_RC(hipMemcpy2DAsync(bucket0_entries, sizeof(uint32_t), ws.sort.dense + 1, sizeof(uint32_t) * ((size_t)B.g.nb + 1),
                                                         sizeof(uint32_t), np, hipMemcpyDeviceToHost, s))))
        return call.done(rc);
    for (size_t p = 0; p < np; ++p) {
        if constexpr (BYTES == 96)
            launch_g1_export(s, res.p + p, d_out.p + BYTES * p);
        else
            launch_g2_export(s, res.p + p, d_out.p + BYTES * p);
    }
    std::vector<uint8_t> tmp(BYTES * np);
    if (hipMemcpyAsync(tmp.data(), d_out.p, tmp.size(), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("msm failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    memcpy(out, tmp.data(), tmp.size());
    return call.done(MASP_HIP_OK);
}
// one MSM of n points; `res`: the context's one-point scratch of this group
template <class O, int BYTES, class X>
static int msm_block(masp_hip_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out, DevBuf<X> masp_hip_ctx::*res_of) {
    if (!ctx || !out || (n && (!bases || !scalars)) || n > (1u << 26)) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    DevBuf<X>& res = ctx->*res_of;
    hipStream_t s = ctx->streams.main;
    for (size_t i = 0; i < n; ++i)
        if (!rs_in_range(scalars + 32 * i)) return call.done(MASP_HIP_E_SCALAR_RANGE);
    MsmBases<O, BYTES> B;
    MsmWorkspace<O> ws;
    int rc;
    if ((rc = B.load_host(bases, (uint32_t)n, s))) return call.done(rc);
    if (B.import_status & (PT_BAD_FLAGS | PT_NOT_CANONICAL)) return call.done(MASP_HIP_E_PARAMS_FORMAT);
    if ((rc = ctx->tmp_scalars.upload((const Fr*)scalars, n, s)) || (rc = res.reserve(1)) || (rc = ctx->tmp_out.reserve(BYTES)) ||
        (rc = msm_enqueue(s, B, ws, (const uint32_t*)ctx->tmp_scalars.p, 0, res.p, 1, 1)))
        return call.done(rc);
    if constexpr (BYTES == 96)
        launch_g1_export(s, res.p, ctx->tmp_out.p);
    else
        launch_g2_export(s, res.p, ctx->tmp_out.p);
    uint8_t tmp[BYTES];
    if (hipMemcpyAsync(tmp, ctx->tmp_out.p, BYTES, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("msm failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    memcpy(out, tmp, BYTES);
    return call.done(MASP_HIP_OK);
}
extern "C" {

// (a multi-device context runs the building blocks and the measurement hooks on its first device)

int masp_hip_msm_g1(masp_hip_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]) {
    return msm_block<FpOps, 96>(ctx, bases, scalars, n, out, &masp_hip_ctx::tmp_g1);
}
int masp_hip_msm_g2(masp_hip_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[192]) {
    return msm_block<Fp2Ops, 192>(ctx, bases, scalars, n, out, &masp_hip_ctx::tmp_g2);
}

int masp_hip_msm_g1_multi(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits, uint8_t* out) {
    return msm_multi<FpOps, 96>(ctx, bases, n, scalars, np, window_bits, out);
}
int masp_hip_msm_g2_multi(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits, uint8_t* out) {
    return msm_multi<Fp2Ops, 192>(ctx, bases, n, scalars, np, window_bits, out);
}

int masp_hip_msm_g1_multi_ex(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits, int block_bits,
                             size_t sub_lo, size_t sub_hi, uint8_t* out, uint32_t* bucket0_entries) {
    return msm_multi<FpOps, 96>(ctx, bases, n, scalars, np, window_bits, out, block_bits, sub_lo, sub_hi, bucket0_entries);
}
int masp_hip_msm_g2_multi_ex(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits, int block_bits,
                             size_t sub_lo, size_t sub_hi, uint8_t* out, uint32_t* bucket0_entries) {
    return msm_multi<Fp2Ops, 192>(ctx, bases, n, scalars, np, window_bits, out, block_bits, sub_lo, sub_hi, bucket0_entries);
}

int masp_hip_quotient_h(masp_hip_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* c, size_t nrows, uint32_t logm, uint8_t* h_out) {
    if (!ctx || !a || !b || !c || !h_out || logm == 0 || logm > 20 || nrows > ((size_t)1 << logm)) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    int rc;
    NttDomain* D;
    if ((rc = ensure_slots(ctx, 1)) || (rc = get_domain(ctx, logm, &D))) return call.done(rc);
    Slot& sl = *ctx->slots[0];
    if ((rc = sl.w.reserve(3 * nrows))) return call.done(rc);
    hipStream_t s = sl.stream;
    const uint8_t* src[3] = {a, b, c};
    const Fr* in[3];
    for (int i = 0; i < 3; ++i) {
        if ((rc = HIP_RC(hipMemcpyAsync(sl.w.p + i * nrows, src[i], 32 * nrows, hipMemcpyHostToDevice, s)))) return call.done(rc);
        in[i] = sl.w.p + i * nrows;
    }
    if ((rc = enqueue_quotient(sl, *D, in, 0, (uint32_t)nrows, false, 1))) return call.done(rc);
    size_t m = (size_t)1 << logm;
    if (hipMemcpyAsync(h_out, sl.h.p, 32 * (m - 1), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("quotient failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    return call.done(MASP_HIP_OK);
}

int masp_hip_ntt(masp_hip_ctx* ctx, uint8_t* data, uint32_t logm, int inverse) {
    if (!ctx || !data || logm == 0 || logm > 20) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    int rc;
    NttDomain* D;
    if ((rc = ensure_slots(ctx, 1)) || (rc = get_domain(ctx, logm, &D))) return call.done(rc);
    Slot& sl = *ctx->slots[0];
    uint32_t m = 1u << logm;
    hipStream_t s = sl.stream;
    if ((rc = sl.w.reserve(m)) || (rc = sl.x0.reserve(m)) || (rc = sl.x1.reserve(m)) ||
        (rc = HIP_RC(hipMemcpyAsync(sl.w.p, data, 32 * (size_t)m, hipMemcpyHostToDevice, s))))
        return call.done(rc);
    launch_ntt_load_bitrev(s, sl.w.p, (size_t)0, m, sl.x0.p, logm, 1);
    D->passes(s, sl.x0.p, inverse ? D->tw_inv.p : D->tw_fwd.p);
    if (inverse) {
        // 1/m scaling: coset_scale[0] = g^0 / m
        Fr* minv_tab = sl.x1.p;
        Fr minv = fe_inv(fr_from_u64_mont(m));
        launch_fr_powers(s, minv_tab, m, fe_one<FrCfg>(), minv, 0);
        launch_fr_scale(s, sl.x0.p, minv_tab, sl.x0.p, m, 1);
    }
    launch_fr_from_mont(s, sl.x0.p, sl.w.p, m);
    if (hipMemcpyAsync(data, sl.w.p, 32 * (size_t)m, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        last_hip_error() = std::string("ntt failed: ") + hipGetErrorString(hipGetLastError());
        return call.done(MASP_HIP_E_HIP);
    }
    return call.done(MASP_HIP_OK);
}

// ---- measurement hooks ----------------------------------------------------------------------------
// (returns the batch's handle, or minus the error code)
int masp_hip_batch_upload(masp_hip_ctx* ctx, size_t n, const masp_hip_job* jobs) {
    if (!ctx || !n || !jobs) return -MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    std::unique_ptr<ResidentBatch> B(new ResidentBatch);
    B->n = n;
    size_t total = 0;
    for (size_t j = 0; j < n; ++j) {
        if (jobs[j].circuit >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[jobs[j].circuit]) return -call.done(MASP_HIP_E_NOT_LOADED);
        if (!rs_in_range(jobs[j].r) || !rs_in_range(jobs[j].s)) return -call.done(MASP_HIP_E_SCALAR_RANGE);
        if (jobs[j].aux_form > MASP_HIP_AUX_MONTGOMERY || jobs[j].reserved != 0) return -call.done(MASP_HIP_E_INVALID_ARG);
    }
    for (uint32_t c = 0; c < MASP_HIP_MAX_CIRCUITS; ++c)
        for (size_t j = 0; j < n; ++j)
            if (jobs[j].circuit == c) {
                Circuit& C = *ctx->circ[c];
                B->circuit.push_back(c);
                B->order.push_back(j);
                B->w_off.push_back(total);
                total += (size_t)C.n_inputs + C.n_aux;
            }
    int rc;
    if ((rc = B->w.reserve(total)) || (rc = B->rs.reserve(16 * n))) return -call.done(rc);
    hipStream_t s = ctx->streams.main;
    for (size_t k = 0; k < n; ++k) {
        const masp_hip_job& J = jobs[B->order[k]];
        Circuit& C = *ctx->circ[J.circuit];
        if ((rc = HIP_RC(hipMemcpyAsync(B->w.p + B->w_off[k], J.inputs, 32 * (size_t)C.n_inputs, hipMemcpyHostToDevice, s))) ||
            (rc = HIP_RC(hipMemcpyAsync(B->w.p + B->w_off[k] + C.n_inputs, J.aux, 32 * (size_t)C.n_aux, hipMemcpyHostToDevice, s))) ||
            (rc = HIP_RC(hipMemcpyAsync(B->rs.p + 16 * k, J.r, 32, hipMemcpyHostToDevice, s))) ||
            (rc = HIP_RC(hipMemcpyAsync(B->rs.p + 16 * k + 8, J.s, 32, hipMemcpyHostToDevice, s))))
            return -call.done(rc);
        // resident assignments are proved repeatedly and proving converts a Montgomery aux part in place: the resident copy is made
        // canonical once, here
        if (J.aux_form == MASP_HIP_AUX_MONTGOMERY && C.n_aux)
            launch_fr_from_mont(s, B->w.p + B->w_off[k] + C.n_inputs, B->w.p + B->w_off[k] + C.n_inputs, C.n_aux);
        if ((rc = HIP_RC(hipStreamSynchronize(s)))) return -call.done(rc);
    }
    if ((rc = call.done(MASP_HIP_OK))) return -rc;
    size_t k = 0;
    while (k < ctx->batches.size() && ctx->batches[k]) ++k;
    if (k == ctx->batches.size()) ctx->batches.emplace_back();
    ctx->batches[k] = std::move(B);
    return (int)k;
}

int masp_hip_batch_free(masp_hip_ctx* ctx, int handle) {
    ctx = FIRST_DEVICE(ctx);
    if (!ctx || handle < 0 || (size_t)handle >= ctx->batches.size()) return MASP_HIP_E_INVALID_ARG;
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    ctx->batches[handle].reset();
    return MASP_HIP_OK;
}

// Proves every resident job of `handle` `steps` times (step k with the blinding scalars rs[k][job] = r | s, 64 bytes per job,
// or with the uploaded ones when rs is NULL): the whole launch sequence of all steps is enqueued on the slots' streams
// without any host synchronisation in between.  proofs_out: steps x n x 192 bytes, job order inside every step.
int masp_hip_batch_prove_resident_steps(masp_hip_ctx* ctx, int handle, size_t steps, const uint8_t* rs, uint8_t* proofs_out, float* elapsed_ms) {
    if (!ctx || handle < 0 || !proofs_out || !steps) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    if ((size_t)handle >= ctx->batches.size() || !ctx->batches[handle]) return call.done(MASP_HIP_E_INVALID_ARG);
    ResidentBatch& B = *ctx->batches[handle];
    if (rs)
        for (size_t i = 0; i < 2 * steps * B.n; ++i)
            if (!rs_in_range(rs + 32 * i)) return call.done(MASP_HIP_E_SCALAR_RANGE);
    // groups of consecutive same-circuit jobs (their assignments are contiguous: stride = n_vars): (first, count)
    std::vector<std::pair<size_t, size_t>> groups;
    for (size_t j = 0; j < B.n;) {
        size_t k = j + 1;
        while (k < B.n && B.circuit[k] == B.circuit[j]) ++k;
        for (auto& eg : even_groups(k - j, ctx->batch_cap)) groups.push_back({j + eg.first, eg.second});
        j = k;
    }
    size_t ns = std::min<size_t>(groups.size() * steps, (size_t)ctx->n_slots);
    int rc;
    DevBuf<uint8_t> d_proofs;
    DevBuf<uint32_t> d_rs;
    if ((rc = ensure_slots(ctx, ns)) || (rc = d_proofs.reserve(192 * B.n * steps))) return call.done(rc);
    hipStream_t ms = ctx->streams.main;
    if (rs) {  // step-major, STORAGE order of the jobs inside a step
        std::vector<uint8_t> tmp(64 * B.n * steps);
        for (size_t st = 0; st < steps; ++st)
            for (size_t k = 0; k < B.n; ++k) memcpy(&tmp[64 * (st * B.n + k)], rs + 64 * (st * B.n + B.order[k]), 64);
        if ((rc = d_rs.reserve(16 * B.n * steps)) || (rc = HIP_RC(hipMemcpyAsync(d_rs.p, tmp.data(), tmp.size(), hipMemcpyHostToDevice, ms))) ||
            (rc = HIP_RC(hipStreamSynchronize(ms))))
            return call.done(rc);
    }
    Event ev_start, ev_stop;
    if ((rc = ev_start.create()) || (rc = ev_stop.create())) return call.done(rc);
    for (size_t si = 0; si < ns && !rc; ++si) rc = HIP_RC(hipMemsetAsync(ctx->slots[si]->flags.p, 0, sizeof(int), ms));
    if (!rc) rc = HIP_RC(hipEventRecord(ev_start, ms));
    for (size_t si = 0; si < ns && !rc; ++si) rc = HIP_RC(hipStreamWaitEvent(ctx->slots[si]->stream, ev_start, 0));
    const Fr* none[3] = {nullptr, nullptr, nullptr};
    size_t turn = 0;
    for (size_t st = 0; st < steps && !rc; ++st)
        for (size_t gi = 0; gi < groups.size() && !rc; ++gi, ++turn) {
            const size_t first = groups[gi].first, count = groups[gi].second;
            Slot& sl = *ctx->slots[turn % ns];
            Circuit& C = *ctx->circ[B.circuit[first]];
            const uint32_t* grs = rs ? d_rs.p + 16 * (st * B.n + first) : B.rs.p + 16 * first;
            rc = enqueue_proofs(sl, C, (uint32_t)count, B.w.p + B.w_off[first], (size_t)C.n_inputs + C.n_aux, none, grs,
                                d_proofs.p + 192 * (st * B.n + first));
        }
    for (size_t si = 0; si < ns && !rc; ++si)
        if (!(rc = HIP_RC(hipEventRecord(ctx->slots[si]->done, ctx->slots[si]->stream)))) rc = HIP_RC(hipStreamWaitEvent(ms, ctx->slots[si]->done, 0));
    std::vector<uint8_t> stored(192 * B.n * steps);
    if (rc || (rc = HIP_RC(hipEventRecord(ev_stop, ms))) || (rc = HIP_RC(hipMemcpyAsync(stored.data(), d_proofs.p, stored.size(), hipMemcpyDeviceToHost, ms))) ||
        (rc = HIP_RC(hipStreamSynchronize(ms))))
        return call.done(rc);
    for (size_t st = 0; st < steps; ++st)
        for (size_t k = 0; k < B.n; ++k) memcpy(proofs_out + 192 * (st * B.n + B.order[k]), stored.data() + 192 * (st * B.n + k), 192);
    if (elapsed_ms && (rc = HIP_RC(hipEventElapsedTime(elapsed_ms, ev_start, ev_stop)))) return call.done(rc);
    int flags = 0;
    for (size_t si = 0; si < ns; ++si) {
        int f = 0;
        if ((rc = HIP_RC(hipMemcpy(&f, ctx->slots[si]->flags.p, sizeof(int), hipMemcpyDeviceToHost)))) return call.done(rc);
        flags |= f;
    }
    return call.done(flags ? MASP_HIP_E_SCALAR_RANGE : MASP_HIP_OK);
}

int masp_hip_batch_prove_resident(masp_hip_ctx* ctx, int handle, uint8_t* proofs_out, float* elapsed_ms) {
    return masp_hip_batch_prove_resident_steps(ctx, handle, 1, nullptr, proofs_out, elapsed_ms);
}

int masp_hip_profile_enable(masp_hip_ctx* ctx, int on) {
    if (!ctx) return MASP_HIP_E_INVALID_ARG;
    ctx = FIRST_DEVICE(ctx);
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    ctx->profiling = on != 0;
    for (auto& sl : ctx->slots) {
        sl->profiling = ctx->profiling;
        sl->prof.reset();
    }
    return MASP_HIP_OK;
}

int masp_hip_profile_read(masp_hip_ctx* ctx, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
    if (!ctx) return MASP_HIP_E_INVALID_ARG;
    ctx = FIRST_DEVICE(ctx);
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    double t = 0;
    uint64_t l = 0, b = 0;
    for (auto& sl : ctx->slots) {
        sl->prof.collect();
        t += sl->prof.total_ms;
        l += sl->prof.launches;
        b += sl->prof.alg_bytes;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = l;
    if (alg_bytes) *alg_bytes = b;
    return MASP_HIP_OK;
}

int masp_hip_profile_read_split(masp_hip_ctx* ctx, double ms[8]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    ctx = FIRST_DEVICE(ctx);
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    for (int i = 0; i < 8; ++i) ms[i] = 0;
    for (auto& sl : ctx->slots) {
        sl->prof.collect();
        for (int i = 0; i < MsmProfile::PH_N; ++i) ms[i] += sl->prof.split_ms[i];
    }
    return MASP_HIP_OK;
}

int masp_hip_profile_read_lone(masp_hip_ctx* ctx, double ms[12]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    ctx = FIRST_DEVICE(ctx);
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    for (int i = 0; i < Slot::N_LONE_MARKS; ++i) ms[i] = -1.0;
    for (auto& sl : ctx->slots) {
        if (!sl->lone_marked || !sl->ev_lone[0]) continue;
        for (int i = 0; i < Slot::N_LONE_MARKS; ++i) {
            float t = 0;
            if (sl->ev_lone[i] && hipEventElapsedTime(&t, sl->ev_lone[0], sl->ev_lone[i]) == hipSuccess) ms[i] = t;
        }
        (void)hipGetLastError();
        return MASP_HIP_OK;
    }
    return MASP_HIP_E_INVALID_ARG;   // no lone proof has run with profiling on
}

int masp_hip_bench_msm(masp_hip_ctx* ctx, int handle, size_t job, int which, int iters, float* avg_ms, uint32_t* n_bases) {
    if (!ctx || handle < 0 || which < 0 || which > 3 || iters <= 0 || !avg_ms) return MASP_HIP_E_INVALID_ARG;
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    ctx = call.ctx;
    if ((size_t)handle >= ctx->batches.size() || !ctx->batches[handle]) return call.done(MASP_HIP_E_INVALID_ARG);
    ResidentBatch& B = *ctx->batches[handle];
    if (job >= B.n) return call.done(MASP_HIP_E_INVALID_ARG);
    for (size_t k = 0; k < B.n; ++k)
        if (B.order[k] == job) {
            job = k;
            break;
        }
    int rc;
    if ((rc = ensure_slots(ctx, 1))) return call.done(rc);
    Slot& sl = *ctx->slots[0];
    Circuit& C = *ctx->circ[B.circuit[job]];
    const Fr* none[3] = {nullptr, nullptr, nullptr};
    Event e0, e1;
    // one full proof first so that sl.h / sl.sa / sl.sb hold this job's real scalars
    if ((rc = enqueue_proofs(sl, C, 1, B.w.p + B.w_off[job], 0, none, B.rs.p + 16 * job, sl.proof.p)) || (rc = HIP_RC(hipStreamSynchronize(sl.stream))) ||
        (rc = e0.create()) || (rc = e1.create()) || (rc = HIP_RC(hipEventRecord(e0, sl.stream))))
        return call.done(rc);
    const BasesG1* bases[4] = {&C.h, &C.l, &C.a, &C.b1};
    const uint32_t* scal[4] = {(const uint32_t*)sl.h.p, (const uint32_t*)(B.w.p + B.w_off[job] + C.n_inputs), (const uint32_t*)sl.sa.p,
                               (const uint32_t*)sl.sb.p};
    for (int it = 0; it < iters; ++it)
        if ((rc = msm_enqueue(sl.stream, *bases[which], sl.ws1, scal[which], 0, sl.res1.p + which, 4, 1))) return call.done(rc);
    float ms = 0;
    if ((rc = HIP_RC(hipEventRecord(e1, sl.stream))) || (rc = HIP_RC(hipStreamSynchronize(sl.stream))) || (rc = HIP_RC(hipEventElapsedTime(&ms, e0, e1))))
        return call.done(rc);
    *avg_ms = ms / iters;
    if (n_bases) *n_bases = bases[which]->n;
    return call.done(MASP_HIP_OK);
}

}  // extern "C"
