// libmasp_hip: the per-proof kernel pipeline — slot pool, launch sequences, masp_hip_prove_batch (include/masp_hip.h).
// Mirrors, on the GPU, what `create_random_proof(circuit, &Parameters, rng)` does after synthesis
// (masp_proofs/src/sapling/prover.rs:117,202,252 -> nam-bellperson):
//   witness -> a,b,c (static R1CS SpMV) -> quotient h (7 NTTs) -> MSMs H, L, A, B1 (G1), B2 (G2)
//   -> assembly with r, s -> 192-byte proof.
#include <chrono>

#include "pipeline.h"

using namespace masp;

// host-to-device copies of concurrent calls one batch after the other (masp_hip_ctx::upload_tail); 0: as they come (A/B builds)
#ifndef MASP_UPLOAD_CHAIN
#define MASP_UPLOAD_CHAIN 1
#endif

namespace masp {

std::vector<std::pair<size_t, size_t>> even_groups(size_t n, size_t cap) {
    std::vector<std::pair<size_t, size_t>> out;
    if (!n) return out;
    const size_t g = (n + cap - 1) / cap, base = n / g, extra = n % g;
    size_t lo = 0;
    for (size_t i = 0; i < g; ++i) {
        size_t cnt = base + (i < extra ? 1 : 0);
        out.push_back({lo, cnt});
        lo += cnt;
    }
    return out;
}

// a new slot on the context's next row of streams (slot_mu held; the caller has checked that the row exists)
static int add_slot(masp_hip_ctx* ctx, char busy) {
    std::unique_ptr<Slot> s(new Slot);
    int rc = s->init(ctx->streams.slot[ctx->slots.size()]);
    if (rc) return rc;
    s->profiling = ctx->profiling;
    s->quotient_schedule = &ctx->quotient_schedule;
    s->configure(ctx->opt);
    ctx->slots.push_back(std::move(s));
    ctx->slot_busy.push_back(busy);
    return MASP_HIP_OK;
}
int ensure_slots(masp_hip_ctx* ctx, size_t want) {
    std::lock_guard<std::mutex> g(ctx->slot_mu);
    want = std::min(want, ctx->streams.slot.size());
    while (ctx->slots.size() < want)
        if (int rc = add_slot(ctx, 0)) return rc;
    // (a slot is configured once, when it is created: its options never change, and a busy slot's workspaces are read by the
    // thread that owns it — the tree sub-batch may also have been halved there for lack of scratch)
    for (auto& sl : ctx->slots) sl->profiling = ctx->profiling;
    return MASP_HIP_OK;
}
// the first free slot, now busy, or slots.size() when every slot is busy (slot_mu held)
static size_t take_free_slot(masp_hip_ctx* ctx) {
    size_t i = 0;
    while (i < ctx->slots.size() && ctx->slot_busy[i]) ++i;
    if (i < ctx->slots.size()) ctx->slot_busy[i] = 1;
    return i;
}
// Slot pool for concurrent provers.  try: a free slot, or a new one while fewer than ctx->n_slots exist.
// Returns MASP_HIP_OK and *si, or -1 if every slot is busy, or an error code.
static int slot_try_acquire(masp_hip_ctx* ctx, size_t* si) {
    std::lock_guard<std::mutex> g(ctx->slot_mu);
    if ((*si = take_free_slot(ctx)) < ctx->slots.size()) return MASP_HIP_OK;
    if (ctx->slots.size() >= (size_t)ctx->n_slots) return -1;
    return add_slot(ctx, 1);   // (*si is already its index)
}
static size_t slot_acquire_blocking(masp_hip_ctx* ctx) {
    std::unique_lock<std::mutex> g(ctx->slot_mu);
    size_t si = 0;
    ctx->slot_cv.wait(g, [&] { return (si = take_free_slot(ctx)) < ctx->slots.size(); });
    return si;
}
static void slot_release(masp_hip_ctx* ctx, size_t si) {
    bool idle = true;
    {
        std::lock_guard<std::mutex> g(ctx->slot_mu);
        ctx->slot_busy[si] = 0;
        for (char b : ctx->slot_busy) idle = idle && !b;
    }
    ctx->slot_cv.notify_one();
    // nothing of this context is in flight: the moment to give back what its workspaces outgrew (util.h, dev_free)
    if (idle) dev_free_drain();
}
// Quotient for np proofs on slot buffers: in[i] + p * in_stride are Montgomery (mont_in) or canonical evaluation
// vectors of `nrows` entries on the device; result: sl.h + p * m = canonical coefficients h[0..m-1).
// h_out (stride h_stride elements per proof; NULL: sl.h, stride m).
int enqueue_quotient(Slot& sl, const NttDomain& D, const Fr* const in[3], size_t in_stride, uint32_t nrows, bool mont_in, uint32_t np, Fr* h_out,
                     size_t h_stride) {
    hipStream_t s = sl.stream;
    const uint32_t m = (uint32_t)D.m, logm = D.logm;
    // A batch goes through the six transforms in sub-batches whose six work buffers (sub x 6 x 32 m bytes: 192 MiB for
    // eight Spend proofs) stay in the 256 MiB Infinity Cache from pass to pass, instead of every pass streaming the whole
    // batch (np x 4 MiB per buffer) through HBM.  The work buffers are only sub proofs long; h is the per-batch result.
    const uint32_t sub_max = sl.ntt_sub;  // masp_hip_options::ntt_sub_batch (0 = the whole batch at once)
    const uint32_t sub = sub_max ? std::min(sub_max, np) : np;
    int rc;
    // a, b and c go through every pass TOGETHER: the three transforms of a sub-batch lie back to back in one buffer
    // ([a | b | c] x q proofs) and a pass is one launch over 3 q transforms — three times the workgroups per launch
    // (a lone proof: 384 instead of 128 on 256 CUs) and 12 instead of 22 launches per sub-batch
    if ((rc = sl.x0.reserve((size_t)3 * m * sub)) || (rc = sl.x1.reserve((size_t)2 * m * sub))) return rc;
    if (!h_out) {
        if ((rc = sl.h.reserve((size_t)m * np))) return rc;
        h_out = sl.h.p;
        h_stride = m;
    }
    Fr *x0 = sl.x0.p, *x1 = sl.x1.p;
    for (uint32_t p0 = 0; p0 < np; p0 += sub) {
        const uint32_t q = std::min(sub, np - p0);
        const size_t part = (size_t)q * m;  // one of a / b / c for the whole sub-batch
        for (int i = 0; i < 3; ++i) {
            const Fr* src = in[i] + (size_t)p0 * in_stride;
            if (mont_in)
                launch_ntt_copy_bitrev(s, src, in_stride, nrows, x0 + i * part, logm, q);
            else
                launch_ntt_load_bitrev(s, src, in_stride, nrows, x0 + i * part, logm, q);
        }
        D.passes(s, x0, D.tw_inv.p, 3 * q);                                     // m A, m B, m C (coefficients)
        launch_ntt_scale_bitrev(s, x0, D.coset_scale.p, x1, logm, 2 * q);       // A, B: * g^k / m
        D.passes(s, x1, D.tw_fwd.p, 2 * q);                                     // A, B on the coset g H
        launch_ntt_ab_bitrev(s, x1, x1 + part, x0, logm, q);
        D.passes(s, x0, D.tw_inv.p, q);                                         // m g^k ((g^m - 1) h + C)_k
        // h = (that * g^-k / m - C) / (g^m - 1); leaves Montgomery form
        launch_fr_scale_sub(s, x0, D.h_scale.p, x0 + 2 * part, D.c_scale, h_out + (size_t)p0 * h_stride, m, q, h_stride);
    }
    return MASP_HIP_OK;
}

// The quotient of a batch in EVALUATION form (Circuit::hl_eval): a and b only — to coefficients, onto the coset g H — and then their
// pointwise product E = a b / (g^m - 1), canonical, straight into the merged scalar buffer (e_out + p * e_stride); four transforms per
// proof.  in[0], in[1] + p * in_stride: Montgomery evaluation vectors of `nrows` entries.
// Where the domain allows it (ntt_fused_ok) a sub-batch is three launches over one work buffer: the inverse transforms as decimation in
// frequency straight from `in`, both transforms' low stages with the coset scale between them, the forward transforms' top stages with the
// product (device/ntt.hpp).  Otherwise, or with masp_hip_ctx_set_quotient_schedule(1): seven launches — two copies into bit-reversed order,
// the inverse passes, the scale with another permutation into a second buffer, the forward passes, the product.
static int enqueue_quotient_eval(Slot& sl, const NttDomain& D, const Fr* const in[2], size_t in_stride, uint32_t nrows, uint32_t np, Fr* e_out,
                                 size_t e_stride) {
    hipStream_t s = sl.stream;
    const uint32_t m = (uint32_t)D.m, logm = D.logm;
    const bool fused = ntt_fused_ok(logm) && D.coset_scale_rev.p && !(sl.quotient_schedule && sl.quotient_schedule->load(std::memory_order_relaxed));
    // as in enqueue_quotient: the work buffers stay in the Infinity Cache — sub x 4 x 32 m bytes for the separate passes; the three kernels
    // work in ONE buffer of [a | b] and take twice the proofs in the same bytes (16 Spend proofs: 128 MiB; measured against 8 in MEASUREMENTS.md)
    const uint32_t sub_max = fused ? 2 * sl.ntt_sub : sl.ntt_sub;
    const uint32_t sub = sub_max ? std::min(sub_max, np) : np;
    int rc;
    if ((rc = sl.x0.reserve((size_t)2 * m * sub)) || (!fused && (rc = sl.x1.reserve((size_t)2 * m * sub)))) return rc;
    Fr *x0 = sl.x0.p, *x1 = sl.x1.p;
    for (uint32_t p0 = 0; p0 < np; p0 += sub) {
        const uint32_t q = std::min(sub, np - p0);
        const size_t part = (size_t)q * m;  // one of a / b for the whole sub-batch
        if (fused) {
            launch_ntt_dif_top(s, in[0] + (size_t)p0 * in_stride, in[1] + (size_t)p0 * in_stride, in_stride, nrows, x0, D.tw_inv.p, logm, q);
            launch_ntt_mid(s, x0, D.tw_inv.p, D.coset_scale_rev.p, D.tw_fwd.p, logm, 2 * q);   // A, B on the coset g H but for the top stages
            launch_ntt_dit_top_ab(s, x0, part, D.tw_fwd.p, D.e_scale, e_out + (size_t)p0 * e_stride, e_stride, logm, q);
            continue;
        }
        for (int i = 0; i < 2; ++i) launch_ntt_copy_bitrev(s, in[i] + (size_t)p0 * in_stride, in_stride, nrows, x0 + i * part, logm, q);
        D.passes(s, x0, D.tw_inv.p, 2 * q);                                     // m A, m B (coefficients)
        launch_ntt_scale_bitrev(s, x0, D.coset_scale.p, x1, logm, 2 * q);       // * g^k / m
        D.passes(s, x1, D.tw_fwd.p, 2 * q);                                     // A, B on the coset g H, natural order
        launch_ntt_ab_eval(s, x1, x1 + part, D.e_scale, e_out + (size_t)p0 * e_stride, m, q, e_stride);
    }
    return MASP_HIP_OK;
}

// a, b (and c, n_mat = 3) = A w, B w, C w of np assignments in one launch: in[i] = sl.ev[i], Montgomery, read from sl.wm
static int enqueue_r1cs_eval(Slot& sl, Circuit& C, uint32_t np, int n_mat, const Fr* in[3]) {
    R1csMatrices M{};   // (the matrices beyond n_mat stay null)
    for (int i = 0; i < n_mat; ++i) {
        if (int rc = sl.ev[i].reserve((size_t)C.nrows * np)) return rc;
        M.rowptr[i] = C.rowptr[i].p;
        M.order[i] = C.row_order[i].p;
        M.n_long[i] = C.n_long_rows[i];
        M.col[i] = C.col[i].p;
        M.coef[i] = C.coef[i].p;
        M.out[i] = sl.ev[i].p;
        in[i] = sl.ev[i].p;
    }
    launch_r1cs_eval(sl.stream, M, sl.wm.p, C.n_inputs + C.n_aux, C.n_constraints, C.n_inputs, np, (uint32_t)n_mat);
    return MASP_HIP_OK;
}

// The rest of a lone proof's DAG (fewer than 8 proofs: too few to fill the chip one stage after the other), behind the fork and the
// R1CS evaluation that enqueue_proofs has queued: five streams, joined on the main one.  in, mont_in: as enqueue_quotient takes them.
static int enqueue_lone(Slot& sl, Circuit& C, uint32_t np, const Fr* d_w, size_t w_stride, const Fr* const in[3], bool mont_in,
                        const uint32_t* d_rs, uint8_t* d_proof) {
    hipStream_t s = sl.stream;
    int rc;
    // the four witness MSMs run on their own streams (forked above) while the main stream runs SpMV -> quotient -> H.
    // The pieces of the assembly start as soon as what they read exists: the fixed-base multiplications (r and s only)
    // right away, s*A and r*B1 behind their MSMs, g_b behind B2 — after the join only g_a / g_c are left.
    launch_groth16_fixed_g1(sl.aux[0], C.fb1.p, d_rs, 16, sl.asm1.p, np);
    launch_groth16_fixed_g2(sl.aux[0], C.fb2.p, d_rs, 16, sl.asm2.p, np);
    HIP_TRY(hipEventRecord(sl.ev_fixed, sl.aux[0]));  // s*delta2 is read by g_b on aux[3]
    // Enqueueing a lone proof takes the host ~3 ms (~250 launches) — as long as its longest chain runs, so whatever is
    // enqueued last starts 3 ms late: the chains go out longest first — A and B1 + B2 (an MSM followed by 2.3 ms of
    // variable-base multiplication; B2's G2 tails), then the quotient and H (the SpMV in front of them is 25 us), then L,
    // which only reads the witness and is the shortest.  (Helper threads enqueueing the chains side by side, and high-
    // priority streams for A / B1, were measured: every chain then starts within 0.5 ms, they slow each other down and the
    // proof takes the same 6.1 - 6.4 ms: profiles/r03x_same_box_ab_lone_threads.txt.)
    const bool own_b2 = C.b2_lone.n != 0;  // B2 on its own narrow windows: sorts for itself
    // (where the batch tables of a / b_g1 have doubled window rows, a lone proof has plain ones of its own: Circuit::a_lone)
    const BasesG1 &Al = C.a_lone.n ? C.a_lone : C.a, &B1l = C.b1_lone.n ? C.b1_lone : C.b1;
    const bool share_bl = C.nbq && msm_same_sort(B1l, C.b2);
    // A and s*A on aux[1]
    if (C.na) launch_gather_scalars(sl.aux[1], d_w, w_stride, C.a_var.p, C.na, sl.sa.p, np);
    if ((rc = msm_enqueue(sl.aux[1], Al, sl.ws_a, (const uint32_t*)sl.sa.p, (size_t)C.na * 8, sl.res1.p + 2, 4, np))) return rc;
    sl.lone_mark(sl.aux[1], 1);
    launch_groth16_var_mul(sl.aux[1], 0, sl.res1.p, d_rs, 16, sl.asm1.p, np, C.g1_endo);
    sl.lone_mark(sl.aux[1], 2);
    // B1 and r*B1 on aux[2]; B2 and g_b on aux[3]
    if (C.nbq) launch_gather_scalars(sl.aux[2], d_w, w_stride, C.b_var.p, C.nbq, sl.sb.p, np);
    HIP_TRY(hipEventRecord(sl.ev_sort_b, sl.aux[2]));  // B2 on aux[3] reads sb (and, without tables of its own, B1's sort) behind this
    if (share_bl) {
        if ((rc = msm_sort_enqueue(sl.aux[2], B1l.n, B1l.g, sl.ws_b.sort, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, np, 0, B1l.subset()))) return rc;
        if (!own_b2) HIP_TRY(hipEventRecord(sl.ev_sort_b, sl.aux[2]));
        if ((rc = msm_reduce_enqueue(sl.aux[2], B1l, sl.ws_b.sort, sl.ws_b, sl.res1.p + 3, 4))) return rc;
    } else if ((rc = msm_enqueue(sl.aux[2], B1l, sl.ws_b, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, sl.res1.p + 3, 4, np))) {
        return rc;
    }
    sl.lone_mark(sl.aux[2], 3);
    launch_groth16_var_mul(sl.aux[2], 1, sl.res1.p, d_rs, 16, sl.asm1.p, np, C.g1_endo);
    sl.lone_mark(sl.aux[2], 4);
    HIP_TRY(hipStreamWaitEvent(sl.aux[3], sl.ev_sort_b, 0));
    if (own_b2) {
        if ((rc = msm_enqueue(sl.aux[3], C.b2_lone, sl.ws2, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, sl.res2.p, 1, np))) return rc;
    } else if (share_bl) {
        if ((rc = msm_reduce_enqueue(sl.aux[3], C.b2, sl.ws_b.sort, sl.ws2, sl.res2.p, 1))) return rc;
    } else if ((rc = msm_enqueue(sl.aux[3], C.b2, sl.ws2, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, sl.res2.p, 1, np))) {
        return rc;
    }
    sl.lone_mark(sl.aux[3], 5);
    HIP_TRY(hipStreamWaitEvent(sl.aux[3], sl.ev_fixed, 0));
    launch_groth16_finish_b(sl.aux[3], C.vk.p, sl.asm2.p, sl.res2.p, d_proof, np);
    sl.lone_mark(sl.aux[3], 6);
    // (measured and dropped in round 5: the quotient first with the side chains' chip-filling kernels gated behind it — the quotient
    // then ends at 0.8 instead of 1.3 ms and MSM h, which now shares the chip with four accumulations, 0.3 ms LATER: a lone proof is
    // ~2.5 ms of chip-filling work, its chains can only trade places: profiles/r05_lone_proof_chains.txt)
    if ((rc = enqueue_quotient(sl, *C.dom, in, C.nrows, C.nrows, mont_in, np))) return rc;
    sl.lone_mark(s, 7);
    if ((rc = msm_enqueue(s, C.h, sl.ws1, (const uint32_t*)sl.h.p, C.m * 8, sl.res1.p + 0, 4, np, sl.profiling ? &sl.prof : nullptr))) return rc;
    sl.lone_mark(s, 8);
    if ((rc = msm_enqueue(sl.aux[0], C.l, sl.ws_l, (const uint32_t*)(d_w + C.n_inputs), w_stride * 8, sl.res1.p + 1, 4, np))) return rc;
    sl.lone_mark(sl.aux[0], 9);
    // g_a and all of g_c but H need L, s*A and r*B1 (aux[0..2]): summed on aux[0] behind those chains, while H is still being
    // computed (k_groth16_finish_ac_early); the main stream joins aux[0] and adds H.  g_b finishes on aux[3] by itself and is only
    // joined before the proof leaves
    for (int i = 1; i < Slot::N_AUX - 1; ++i) {
        HIP_TRY(hipEventRecord(sl.ev_join[i], sl.aux[i]));
        HIP_TRY(hipStreamWaitEvent(sl.aux[0], sl.ev_join[i], 0));
    }
    launch_groth16_finish_ac_early(sl.aux[0], C.vk.p, sl.asm1.p, sl.res1.p, d_proof, np);
    HIP_TRY(hipEventRecord(sl.ev_join[0], sl.aux[0]));
    HIP_TRY(hipStreamWaitEvent(s, sl.ev_join[0], 0));
    launch_groth16_finish_c_late(s, sl.asm1.p, sl.res1.p, d_proof, np);
    sl.lone_mark(s, 10);   // g_a / g_c written
    HIP_TRY(hipEventRecord(sl.ev_join[Slot::N_AUX - 1], sl.aux[Slot::N_AUX - 1]));
    HIP_TRY(hipStreamWaitEvent(s, sl.ev_join[Slot::N_AUX - 1], 0));
    sl.lone_mark(s, 11);   // ... and g_b: the proof is complete
    return MASP_HIP_OK;
}

// A batch (8 proofs or more), behind the R1CS evaluation: every stage one launch for all of them, one after the other on the slot's main
// stream.  eval_form: the quotient in evaluation form, over Circuit::hl_eval.
static int enqueue_batch(Slot& sl, Circuit& C, uint32_t np, const Fr* d_w, size_t w_stride, const Fr* const in[3], bool mont_in,
                         bool eval_form, const uint32_t* d_rs, uint8_t* d_proof) {
    hipStream_t s = sl.stream;
    int rc;
    MsmProfile* prof = sl.profiling ? &sl.prof : nullptr;
    // H and L as one MSM over the merged base set (Circuit::hl): the scalars of a proof are its m - 1 quotient coefficients
    // followed by its aux assignment (the quotient's m-th, unused, coefficient lands on the first aux slot and is then
    // overwritten by the copy)
    // In evaluation form (Circuit::hl_eval) the scalars are the m coset evaluations E, the aux assignment and the inputs C uses.
    const BasesG1& HL = eval_form ? C.hl_eval : C.hl;
    const size_t hl_stride = HL.n, aux_at = eval_form ? C.m : C.m - 1;
    if ((rc = sl.hl.reserve(hl_stride * np + 1))) return rc;
    if (eval_form) {
        if ((rc = enqueue_quotient_eval(sl, *C.dom, in, C.nrows, C.nrows, np, sl.hl.p, hl_stride))) return rc;
        if (C.n_eval_in) launch_gather_scalars(s, d_w, w_stride, C.eval_in_var.p, C.n_eval_in, sl.hl.p + C.m + C.n_aux, np, hl_stride);
    } else if ((rc = enqueue_quotient(sl, *C.dom, in, C.nrows, C.nrows, mont_in, np, sl.hl.p, hl_stride))) {
        return rc;
    }
    if (C.n_aux)
        HIP_TRY(hipMemcpy2DAsync(sl.hl.p + aux_at, hl_stride * sizeof(Fr), d_w + C.n_inputs, w_stride * sizeof(Fr), (size_t)C.n_aux * sizeof(Fr), np,
                                 hipMemcpyDeviceToDevice, s));
    // query scalars selected by density
    if (C.na) launch_gather_scalars(s, d_w, w_stride, C.a_var.p, C.na, sl.sa.p, np);
    if (C.nbq) launch_gather_scalars(s, d_w, w_stride, C.b_var.p, C.nbq, sl.sb.p, np);
    if ((rc = msm_enqueue(s, HL, sl.ws1, (const uint32_t*)sl.hl.p, hl_stride * 8, sl.res1.p + 0, 4, np, prof))) return rc;
    // L is inside H + L: its slot of every proof is the point at infinity (one strided fill, not np of them)
    HIP_TRY(hipMemset2DAsync(sl.res1.p + 1, 4 * sizeof(G1Xyzz), 0, sizeof(G1Xyzz), np, s));
    // (b_g2 on b_g1's window width is reduced from b_g1's sorted digit list; on a width of its own — masp_hip_options::window_bits_b2 — it sorts for itself)
    if ((rc = msm_enqueue(s, C.a, sl.ws1, (const uint32_t*)sl.sa.p, (size_t)C.na * 8, sl.res1.p + 2, 4, np, prof))) return rc;
    if ((rc = msm_enqueue(s, C.b1, sl.ws1, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, sl.res1.p + 3, 4, np, prof))) return rc;
    if (C.nbq && msm_same_sort(C.b1, C.b2)) {   // B2 runs over the same scalars as B1
        if ((rc = msm_reduce_enqueue(s, C.b2, sl.ws1.sort, sl.ws2, sl.res2.p, 1))) return rc;
    } else if ((rc = msm_enqueue(s, C.b2, sl.ws2, (const uint32_t*)sl.sb.p, (size_t)C.nbq * 8, sl.res2.p, 1, np))) {
        return rc;
    }
    launch_groth16_fixed_g1(s, C.fb1.p, d_rs, 16, sl.asm1.p, np);
    launch_groth16_fixed_g2(s, C.fb2.p, d_rs, 16, sl.asm2.p, np);
    launch_groth16_var_mul(s, 2, sl.res1.p, d_rs, 16, sl.asm1.p, np, C.g1_endo);
    launch_groth16_finish_b(s, C.vk.p, sl.asm2.p, sl.res2.p, d_proof, np);
    launch_groth16_finish_ac(s, C.vk.p, sl.asm1.p, sl.res1.p, d_proof, np);
    return MASP_HIP_OK;
}

// Enqueue np proofs of circuit C as one batch.  d_w + p * w_stride: n_vars canonical scalars on the device (inputs then
// aux).  d_abc[i] + p * nrows: canonical evaluation vectors on the device, or all NULL.  d_rs + p * 16: r | s limbs.
// d_proof + p * 192: output.
// aux_montgomery: the aux part of every assignment (d_w + p * w_stride + n_inputs ...) holds Montgomery residues
// (masp_hip_job::aux_form); it is converted to canonical form in place first (d_w must then be writable).
// This is the head both modes share — range check, R1CS evaluation, the query scalars' buffers; the rest is enqueue_lone or enqueue_batch.
int enqueue_proofs(Slot& sl, Circuit& C, uint32_t np, const Fr* d_w, size_t w_stride, const Fr* const d_abc[3], const uint32_t* d_rs,
                   uint8_t* d_proof, bool aux_montgomery) {
    hipStream_t s = sl.stream;
    const uint32_t nv = C.n_inputs + C.n_aux;
    int rc;
    if ((rc = sl.reserve_batch(np))) return rc;
    // (sl.flags accumulates: the caller clears it before the first batch it will read the flag for)
    if ((rc = sl.wm.reserve((size_t)nv * np))) return rc;
    const bool lone = np < 8;
    // range check (+ Montgomery copy used by the SpMV); an aux part that arrived as Montgomery residues becomes canonical here,
    // BEFORE anything reads it as scalars — in lone mode before the side streams fork, which read it; a canonical one is only
    // checked, so there the fork goes first and the side chains do not wait for the check
    if (aux_montgomery) launch_fr_split_forms(s, const_cast<Fr*>(d_w), w_stride, sl.wm.p, nv, C.n_inputs, np, sl.flags.p);
    if (lone) {
        // lone-proof mode: L, A, B1 and B2 only read the assignment (already on the device when this stream gets here), so
        // their streams fork NOW, before the range check and the SpMV are queued on the main stream
        sl.lone_mark(s, 0);
        HIP_TRY(hipEventRecord(sl.ev_fork, s));
        for (int i = 0; i < Slot::N_AUX; ++i) HIP_TRY(hipStreamWaitEvent(sl.aux[i], sl.ev_fork, 0));
    }
    if (!aux_montgomery) launch_fr_to_mont(s, d_w, w_stride, sl.wm.p, nv, np, sl.flags.p);
    // the quotient in evaluation form: a batch of the circuit's own a, b, c whose circuit has the derived bases (Circuit::hl_eval)
    const bool eval_form = !lone && !d_abc[0] && C.hl_eval.n != 0;
    // the caller's a, b, c (canonical), or the slot's own R1CS evaluation (Montgomery; c is folded into hl_eval: not evaluated there)
    const Fr* in[3] = {d_abc[0], d_abc[1], d_abc[2]};
    const bool mont_in = !d_abc[0];
    if (mont_in && (rc = enqueue_r1cs_eval(sl, C, np, eval_form ? 2 : 3, in))) return rc;
    if ((rc = sl.sa.reserve((size_t)C.na * np)) || (rc = sl.sb.reserve((size_t)C.nbq * np))) return rc;
    return lone ? enqueue_lone(sl, C, np, d_w, w_stride, in, mont_in, d_rs, d_proof)
                : enqueue_batch(sl, C, np, d_w, w_stride, in, mont_in, eval_form, d_rs, d_proof);
}

// enqueue_proofs for a batch of fewer than 8 proofs, replayed from a captured HIP graph once the same call has been seen
// twice.  A lone Spend proof is ~250 launches on five streams: the host needs ~3 ms to enqueue what the GPU runs in 5 - 6 ms,
// and the chain enqueued last starts that much late (profiles/r04z_lone_proof_timeline.txt); one hipGraphLaunch of the same
// DAG does not.  The key is everything the launches' arguments are derived from: the circuit, the proof count, the slot's
// buffers the caller passes and the form of the aux part; the workspaces inside (grown on demand) are covered by
// device_alloc_epoch().  First call with a key: plain enqueue (sizes every buffer).  Second: captured (nothing runs), then
// launched.  Any failure on the way — an allocation inside the capture, a runtime that refuses a node — marks the key dead
// and the call is enqueued the plain way: never an error of its own.
static int enqueue_proofs_graphed(Slot& sl, Circuit& C, uint32_t np, const Fr* d_w, size_t w_stride, const Fr* const d_abc[3], const uint32_t* d_rs,
                                  uint8_t* d_proof, bool aux_montgomery) {
    if (np >= 8 || !sl.lone_graph || sl.profiling) return enqueue_proofs(sl, C, np, d_w, w_stride, d_abc, d_rs, d_proof, aux_montgomery);
    const uint64_t epoch = device_alloc_epoch().load(std::memory_order_relaxed);
    if (epoch != sl.graph_epoch) {
        sl.drop_graphs();
        sl.graph_epoch = epoch;
    }
    Slot::LoneGraph* e = nullptr;
    for (auto& g : sl.graphs)
        if (g.circuit == &C && g.np == np && g.w == d_w && g.w_stride == w_stride && g.abc == d_abc[0] && g.rs == d_rs && g.proof == d_proof &&
            g.mont == aux_montgomery)
            e = &g;
    if (!e) {
        if (sl.graphs.size() >= 16) sl.drop_graphs();
        sl.graphs.push_back(Slot::LoneGraph{&C, d_w, d_abc[0], d_rs, d_proof, w_stride, np, aux_montgomery, 0, false, nullptr});
        e = &sl.graphs.back();
    }
    if (!e->exec) {   // not captured yet
        if (e->dead || e->runs == 0) {
            ++e->runs;
            return enqueue_proofs(sl, C, np, d_w, w_stride, d_abc, d_rs, d_proof, aux_montgomery);
        }
        bool ok = hipStreamBeginCapture(sl.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const int rc = enqueue_proofs(sl, C, np, d_w, w_stride, d_abc, d_rs, d_proof, aux_montgomery);
            hipGraph_t g = nullptr;
            const hipError_t ce = hipStreamEndCapture(sl.stream, &g);
            ok = rc == MASP_HIP_OK && ce == hipSuccess && g != nullptr && device_alloc_epoch().load(std::memory_order_relaxed) == epoch;
            if (ok) ok = hipGraphInstantiate(&e->exec, g, nullptr, nullptr, 0) == hipSuccess && e->exec != nullptr;
            if (g) hipGraphDestroy(g);
        }
        if (!ok) {
            (void)hipGetLastError();
            launch_error().clear();
            e->exec = nullptr;
            e->dead = true;
            sl.graph_epoch = device_alloc_epoch().load(std::memory_order_relaxed);
            return enqueue_proofs(sl, C, np, d_w, w_stride, d_abc, d_rs, d_proof, aux_montgomery);
        }
    }
    HIP_TRY(hipGraphLaunch(e->exec, sl.stream));
    ++sl.graph_launches;
    return MASP_HIP_OK;
}

bool rs_in_range(const uint8_t* x) {
    Fr v = fe_load_le<FrCfg>(x);
    return !fe_canonical_ge_mod(v);
}

// The jobs of a list bucketed by kind (circuit | aux form, a/b/c given) — whatever their order in the list — and every bucket cut into
// equal groups of at most cap(bucket size) proofs (256 Spends with a cap of 96: 86 + 85 + 85, not 96 + 96 + 64): each group's job indices
template <class Cap>
static std::vector<std::vector<size_t>> group_jobs(size_t n, const masp_hip_job* jobs, Cap cap) {
    std::map<std::pair<uint32_t, bool>, std::vector<size_t>> by_kind;
    for (size_t j = 0; j < n; ++j) by_kind[{jobs[j].circuit | (jobs[j].aux_form ? 0x100u : 0u), jobs[j].a != nullptr}].push_back(j);
    std::vector<std::vector<size_t>> groups;
    for (auto& kv : by_kind)
        for (auto& eg : even_groups(kv.second.size(), cap(kv.second.size())))
            groups.emplace_back(kv.second.begin() + eg.first, kv.second.begin() + eg.first + eg.second);
    return groups;
}

// A host stopwatch for measurement builds (-DMASP_ENQ_TIMING, tools/jobs): when masp_hip_prove_batch enqueued what, on stderr; else empty
struct EnqTimer {
#ifdef MASP_ENQ_TIMING
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    template <class... A> static void log(const char* fmt, A... a) { fprintf(stderr, fmt, a...); }
#else
    double ms() const { return 0; }
    template <class... A> static void log(const char*, A...) {}
#endif
};

// One group of a masp_hip_prove_batch call on its slot: np jobs of one kind, jobs[idx[p]], and where their bytes lie in the slot's pinned
// staging: [np][nv] witness | (a | b | c each [np][nrows]) | [np][16] r,s limbs | [np][n_inputs] the public inputs once more, packed
struct GroupRun {
    masp_hip_ctx* ctx;
    Slot& sl;
    Circuit& C;
    const masp_hip_job* jobs;
    const std::vector<size_t>& idx;
    const size_t np = idx.size(), nv = (size_t)C.n_inputs + C.n_aux;
    const bool has_abc = jobs[idx[0]].a != nullptr;
    const size_t w_bytes = 32 * nv * np, abc_bytes = has_abc ? 3 * 32 * (size_t)C.nrows * np : 0, rs_bytes = 64 * np, in_bytes = 32 * (size_t)C.n_inputs * np;
    const size_t abc_at = w_bytes, rs_at = abc_at + abc_bytes, in_at = rs_at + rs_bytes, stage_bytes = in_at + in_bytes;
    std::vector<char> direct;   // per job: its aux vector already sits in page-locked memory and goes to the device straight from there
    bool any_staged = false;
};

// step 1 of a group: the slot's buffers at the group's size, and the jobs' bytes in its staging
static int stage_group(GroupRun& G) {
    Slot& sl = G.sl;
    const Circuit& C = G.C;
    const size_t np = G.np, nv = G.nv, in_row = 32 * (size_t)C.n_inputs, abc_row = 32 * (size_t)C.nrows;
    int rc;
    if ((rc = sl.h_stage.reserve(G.stage_bytes)) || (rc = sl.w.reserve(nv * np)) || (rc = sl.inp.reserve((size_t)C.n_inputs * np)) ||
        (rc = sl.abc.reserve(G.has_abc ? 3 * (size_t)C.nrows * np : 1)) || (rc = sl.reserve_batch(np)))
        return rc;
    uint8_t* hs = sl.h_stage.p;
    G.direct.assign(np, 0);
    for (size_t p = 0; p < np; ++p) {
        const masp_hip_job& J = G.jobs[G.idx[p]];
        hipPointerAttribute_t attr;
        G.direct[p] = hipPointerGetAttributes(&attr, J.aux) == hipSuccess && attr.type == hipMemoryTypeHost;
        G.any_staged = G.any_staged || !G.direct[p];
        memcpy(hs + 32 * nv * p, J.inputs, in_row);
        memcpy(hs + G.in_at + in_row * p, J.inputs, in_row);
        if (!G.direct[p]) memcpy(hs + 32 * nv * p + in_row, J.aux, 32 * (size_t)C.n_aux);
        if (G.has_abc) {
            const uint8_t* src[3] = {J.a, J.b, J.c};
            for (int i = 0; i < 3; ++i) memcpy(hs + G.abc_at + abc_row * (np * i + p), src[i], abc_row);
        }
        memcpy(hs + G.rs_at + 64 * p, J.r, 32);
        memcpy(hs + G.rs_at + 64 * p + 32, J.s, 32);
    }
    (void)hipGetLastError();  // an unregistered pointer makes hipPointerGetAttributes report an error: expected
    return MASP_HIP_OK;
}

// step 2: the host-to-device copies, on the slot's main stream
static int upload_group(GroupRun& G) {
    Slot& sl = G.sl;
    const Circuit& C = G.C;
    const size_t np = G.np, nv = G.nv, in_row = 32 * (size_t)C.n_inputs;
    const uint8_t* hs = sl.h_stage.p;
    hipStream_t s = sl.stream;
    bool ok = true;
    // (see masp_hip_ctx::upload_tail; the lock covers wait + enqueue + record so that the chain has one order.)  Not with
    // lone_proof_graph: the tail is an event on ANOTHER slot's stream, and while that stream is being captured into a launch graph the
    // runtime refuses the wait ("dependency created on uncaptured work in another stream") although the event was recorded before the
    // capture began — 38 of 960 calls of three threads failed that way (profiles/r06_lone_graph_upload_chain_capture_isolation.txt)
    masp_hip_ctx* ctx = G.ctx;
    const bool chain = MASP_UPLOAD_CHAIN && ctx->opt.lone_proof_graph == 0;
    std::unique_lock<std::mutex> upload_turn(ctx->upload_mu, std::defer_lock);
    if (chain) upload_turn.lock();
    if (chain && ctx->upload_tail && ctx->upload_tail != sl.ev_uploaded) ok = hipStreamWaitEvent(s, ctx->upload_tail, 0) == hipSuccess;
    if (ok && G.any_staged) {
        ok = hipMemcpyAsync(sl.w.p, hs, G.w_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    } else if (ok) {
        // only the public inputs of each proof come from staging: ONE packed copy to the device and a strided copy on the
        // device instead of np small host-to-device copies (a strided host-to-device copy is the runtime's slow path)
        ok = hipMemcpyAsync(sl.inp.p, hs + G.in_at, G.in_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
             hipMemcpy2DAsync(sl.w.p, 32 * nv, sl.inp.p, in_row, in_row, np, hipMemcpyDeviceToDevice, s) == hipSuccess;
    }
    for (size_t p = 0; p < np && ok; ++p)
        if (G.direct[p])
            ok = hipMemcpyAsync(sl.w.p + nv * p + C.n_inputs, G.jobs[G.idx[p]].aux, 32 * (size_t)C.n_aux, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && (!G.has_abc || hipMemcpyAsync(sl.abc.p, hs + G.abc_at, G.abc_bytes, hipMemcpyHostToDevice, s) == hipSuccess) &&
         hipMemcpyAsync(sl.rs.p, hs + G.rs_at, G.rs_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    if (chain && ok && hipEventRecord(sl.ev_uploaded, s) == hipSuccess) ctx->upload_tail = sl.ev_uploaded;
    if (ok) return MASP_HIP_OK;
    last_hip_error() = std::string("H2D copy failed: ") + hipGetErrorString(hipGetLastError());
    return MASP_HIP_E_HIP;
}

// step 3: the range flag cleared, and the group's launch sequence
static int enqueue_group(GroupRun& G) {
    Slot& sl = G.sl;
    const Fr* abc[3] = {nullptr, nullptr, nullptr};
    if (G.has_abc)
        for (int i = 0; i < 3; ++i) abc[i] = sl.abc.p + (size_t)G.C.nrows * G.np * i;
    if (hipMemsetAsync(sl.flags.p, 0, sizeof(int), sl.stream) != hipSuccess) {
        last_hip_error() = "memset failed";
        return MASP_HIP_E_HIP;
    }
    EnqTimer t;   // how long the host takes to enqueue one group
    const int rc = enqueue_proofs_graphed(sl, G.C, (uint32_t)G.np, sl.w.p, G.nv, abc, sl.rs.p, sl.proof.p,
                                          G.jobs[G.idx[0]].aux_form == MASP_HIP_AUX_MONTGOMERY);
    t.log("[enq] %zu proofs: %.3f ms\n", G.np, t.ms());
    return rc;
}

// step 4: proofs and range flag to the slot's pinned buffers, and the event that retire_oldest waits for
static int download_group(GroupRun& G) {
    Slot& sl = G.sl;
    hipStream_t s = sl.stream;
    if (hipMemcpyAsync(sl.h_proof.p, sl.proof.p, 192 * G.np, hipMemcpyDeviceToHost, s) == hipSuccess &&
        hipMemcpyAsync(sl.h_flags.p, sl.flags.p, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipEventRecord(sl.done, s) == hipSuccess)
        return MASP_HIP_OK;
    last_hip_error() = "D2H copy failed";
    return MASP_HIP_E_HIP;
}

}  // namespace masp

extern "C" {

// What masp_hip_prove_batch refuses before it touches a device — the same tests for a single-device context and for the front of a
// multi-device one (there they must not be mistaken for a device's failure)
static int validate_jobs(const masp_hip_ctx* dev_ctx, size_t n, const masp_hip_job* jobs) {
    for (size_t j = 0; j < n; ++j) {
        const masp_hip_job& J = jobs[j];
        if (J.circuit >= MASP_HIP_MAX_CIRCUITS || !J.inputs || !J.aux) return MASP_HIP_E_INVALID_ARG;
        if (!dev_ctx->circ[J.circuit]) return MASP_HIP_E_NOT_LOADED;
        if ((J.a || J.b || J.c) && !(J.a && J.b && J.c)) return MASP_HIP_E_INVALID_ARG;
        if (J.reserved != 0) return MASP_HIP_E_INVALID_ARG;  // must be zero: a later revision of the struct can then give it a meaning
        if (J.aux_form > MASP_HIP_AUX_MONTGOMERY || (J.aux_form && J.a)) return MASP_HIP_E_INVALID_ARG;  // (a, b, c given: nothing reads aux as Montgomery)
        if (!rs_in_range(J.r) || !rs_in_range(J.s)) return MASP_HIP_E_SCALAR_RANGE;
    }
    return MASP_HIP_OK;
}

// Multi-device front (round 6: a queue instead of static shares).  The jobs of every kind (circuit, aux form, a/b/c mode) are cut into
// blocks of up to batch_cap proofs; the blocks wait on ONE queue, the most expensive first (constraints x proofs: a Spend block costs
// three Output blocks), and every device has `slots` host threads that each take the next block when their last one is done — a device
// that clocks lower, or shares its GPU, simply takes fewer.  A device whose call fails with a HIP error is taken OUT (for the life of
// the context: masp_hip_ctx_device_status), its block goes back on the queue and the other devices finish the list; the call fails only
// when no device is left, or for an error of the input (MASP_HIP_E_SCALAR_RANGE from the device's range check of an assignment), which
// no other device would cure.  Proofs are independent: there is no data-path exchange between devices; results are copied to the jobs'
// own positions.  (The reference's loop fails per description: /root/reference/masp_primitives/src/transaction/components/sapling/builder.rs:955-969.)
static int prove_batch_multi(masp_hip_ctx* ctx, size_t n, const masp_hip_job* jobs, uint8_t* proofs_out) {
    const size_t nd = ctx->children.size();
    auto alive = [&](size_t d) { return ctx->dev_status[d].load() == MASP_HIP_OK; };
    size_t n_alive = 0, first_alive = nd;
    for (size_t d = 0; d < nd; ++d)
        if (alive(d)) {
            ++n_alive;
            if (first_alive == nd) first_alive = d;
        }
    if (!n_alive) return MASP_HIP_E_HIP;   // (masp_hip_last_error: the text of the device that failed first)
    {
        std::shared_lock<std::shared_mutex> lock(ctx->children[first_alive]->mu);
        if (int rc = validate_jobs(ctx->children[first_alive], n, jobs)) return rc;
    }
    struct Block {
        std::vector<size_t> idx;
        uint64_t cost;
    };
    std::deque<Block> queue;
    {
        // at least one block per device when the list is long enough to give every device a useful batch
        auto cap = [&](size_t of_kind) { return std::min(ctx->batch_cap, std::max<size_t>((of_kind + n_alive - 1) / n_alive, 8)); };
        std::vector<Block> blocks;
        for (auto& idx : group_jobs(n, jobs, cap)) {
            const uint64_t cost = (uint64_t)ctx->children[first_alive]->circ[jobs[idx[0]].circuit]->nrows * idx.size();
            blocks.push_back({std::move(idx), cost});
        }
        std::stable_sort(blocks.begin(), blocks.end(), [](const Block& x, const Block& y) { return x.cost > y.cost; });
        for (auto& b : blocks) queue.push_back(std::move(b));
    }
    std::mutex mu;                 // queue, pending, fatal
    std::condition_variable cv;
    size_t pending = queue.size();  // blocks not yet proved (queued or in some worker's hands)
    int fatal = MASP_HIP_OK;
    auto worker = [&](size_t d) {
        masp_hip_ctx* ch = ctx->children[d];
        std::vector<masp_hip_job> mine;
        std::vector<uint8_t> out;
        for (;;) {
            Block b;
            {
                std::unique_lock<std::mutex> g(mu);
                // (an empty queue is not the end: a block in another worker's hands may come back when its device fails)
                cv.wait(g, [&] { return !queue.empty() || pending == 0 || fatal || !alive(d); });
                if (pending == 0 || fatal || !alive(d)) return;
                b = std::move(queue.front());
                queue.pop_front();
            }
            mine.resize(b.idx.size());
            for (size_t k = 0; k < mine.size(); ++k) mine[k] = jobs[b.idx[k]];
            out.resize(192 * mine.size());
            const int rc = masp_hip_prove_batch(ch, mine.size(), mine.data(), out.data());
            std::unique_lock<std::mutex> g(mu);
            if (rc == MASP_HIP_OK) {
                for (size_t k = 0; k < b.idx.size(); ++k) memcpy(proofs_out + 192 * b.idx[k], out.data() + 192 * k, 192);
                --pending;
            } else if (rc == MASP_HIP_E_HIP || rc == MASP_HIP_E_NO_DEVICE) {
                int ok = MASP_HIP_OK;
                ctx->dev_status[d].compare_exchange_strong(ok, rc);   // the device is out; its other workers leave at their next turn
                ctx->requeued += b.idx.size();
                queue.push_front(std::move(b));                      // (an expensive block that has already waited: first again)
                bool any = false;
                for (size_t e = 0; e < nd; ++e) any = any || alive(e);
                if (!any) fatal = rc;
            } else {
                fatal = rc;   // an error of the input: no other device would decide differently
            }
            cv.notify_all();
            if (rc != MASP_HIP_OK) return;
        }
    };
    std::vector<std::thread> th;
    for (size_t d = 0; d < nd; ++d) {
        if (!alive(d)) continue;
        // as many calls in flight per device as it has slots (masp_hip_prove_batch of a device context is re-entrant: each call's batches
        // take slots of its pool), but not more workers than there are blocks
        const size_t w = std::min<size_t>(std::max(ctx->children[d]->n_slots, 1), std::max<size_t>((queue.size() + n_alive - 1) / n_alive, 1));
        for (size_t k = 0; k < w; ++k) th.emplace_back(worker, d);
    }
    for (auto& t : th) t.join();
    if (fatal) return fatal;
    return pending == 0 ? MASP_HIP_OK : MASP_HIP_E_HIP;
}

int masp_hip_prove_batch(masp_hip_ctx* ctx, size_t n, const masp_hip_job* jobs, uint8_t* proofs_out) {
    const ApiLaunchScope api_scope;
    if (!ctx || (n && (!jobs || !proofs_out))) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return prove_batch_multi(ctx, n, jobs, proofs_out);
    std::shared_lock<std::shared_mutex> lock(ctx->mu);  // concurrent with other provers, exclusive with circuit loads
    if (int rc = validate_jobs(ctx, n, jobs)) return rc;
    // test hook (masp_hip_ctx_inject_fault): this call fails as a lost device's would, before anything is enqueued
    for (uint32_t left = ctx->fault_countdown.load(); left != 0;) {
        if (!ctx->fault_countdown.compare_exchange_weak(left, left - 1)) continue;
        if (left == 1) {
            last_hip_error() = "injected fault (masp_hip_ctx_inject_fault): this device context's call fails as a lost GPU's would";
            return fail(ctx, MASP_HIP_E_HIP);
        }
        break;
    }
    hipSetDevice(ctx->device);
    // equal batches of at most batch_cap proofs per kind of job; results go back to the jobs' own positions
    const std::vector<std::vector<size_t>> groups = group_jobs(n, jobs, [&](size_t) { return ctx->batch_cap; });
    // Each batch runs on a slot taken from the context's pool; this call keeps up to all of them in flight, and calls
    // from other host threads interleave with it slot by slot.
    struct Owned {
        size_t si, gi;
    };
    std::deque<Owned> owned;
    int result = MASP_HIP_OK, rc;
    auto retire_oldest = [&]() -> size_t {  // waits for the oldest batch in flight; the slot stays ours
        Owned o = owned.front();
        owned.pop_front();
        Slot& sl = *ctx->slots[o.si];
        const std::vector<size_t>& idx = groups[o.gi];
        if (hipEventSynchronize(sl.done) != hipSuccess) {
            last_hip_error() = "event sync failed";
            result = fail(ctx, MASP_HIP_E_HIP);
        } else if (*sl.h_flags.p) {
            result = MASP_HIP_E_SCALAR_RANGE;
        } else if (result == MASP_HIP_OK) {
            for (size_t p = 0; p < idx.size(); ++p) memcpy(proofs_out + 192 * idx[p], sl.h_proof.p + 192 * p, 192);
        }
        return o.si;
    };
    EnqTimer t_call;
    for (size_t gi = 0; gi < groups.size() && result == MASP_HIP_OK; ++gi) {
        EnqTimer t_slot;
        size_t si = 0;
        rc = slot_try_acquire(ctx, &si);
        if (rc > 0) {
            result = fail(ctx, rc);
            break;
        }
        if (rc < 0) si = owned.empty() ? slot_acquire_blocking(ctx) : retire_oldest();
        if (result) {
            slot_release(ctx, si);
            break;
        }
        const double waited_ms = t_slot.ms();
        EnqTimer t_work;
        Slot& sl = *ctx->slots[si];
        GroupRun G{ctx, sl, *ctx->circ[jobs[groups[gi][0]].circuit], jobs, groups[gi]};
        if ((rc = stage_group(G)) || (rc = upload_group(G)) || (rc = enqueue_group(G)) || (rc = download_group(G))) {
            result = fail(ctx, rc);
            for (int i = 0; i < Slot::N_AUX; ++i) hipStreamSynchronize(sl.aux[i]);
            hipStreamSynchronize(sl.stream);
            slot_release(ctx, si);
            break;
        }
        owned.push_back({si, gi});
        t_call.log("[grp] call %p t=%8.2f ms group %zu circuit %u np %zu slot %zu: waited %.2f ms for the slot, staged + enqueued in %.2f ms\n",
                   (void*)jobs, t_call.ms(), gi, jobs[groups[gi][0]].circuit, G.np, si, waited_ms, t_work.ms());
    }
    while (!owned.empty()) slot_release(ctx, retire_oldest());
    t_call.log("[call] %p done after %.2f ms (%zu jobs)\n", (void*)jobs, t_call.ms(), n);
    if (result == MASP_HIP_OK) ctx->proofs_done += n;
    // a launch the runtime refused on this thread (MASP_LAUNCH keeps the first: kernel, file:line, HIP's text)
    const int launch_rc = launch_status();
    if (launch_rc && result == MASP_HIP_OK) result = fail(ctx, launch_rc);
    if (hipGetLastError() != hipSuccess && result == MASP_HIP_OK) {
        last_hip_error() = "kernel launch failed";
        result = fail(ctx, MASP_HIP_E_HIP);
    }
    return result;
}

int masp_hip_prove(masp_hip_ctx* ctx, uint32_t slot, const uint8_t* inputs, const uint8_t* aux, const uint8_t* a, const uint8_t* b,
                   const uint8_t* c, const uint8_t r[32], const uint8_t s[32], uint8_t proof_out[192]) {
    if (!r || !s || !proof_out) return MASP_HIP_E_INVALID_ARG;
    masp_hip_job J;
    J.circuit = slot;
    J.inputs = inputs;
    J.aux = aux;
    J.a = a;
    J.b = b;
    J.c = c;
    J.aux_form = MASP_HIP_AUX_CANONICAL;
    J.reserved = 0;
    memcpy(J.r, r, 32);
    memcpy(J.s, s, 32);
    uint8_t tmp[192];
    int rc = masp_hip_prove_batch(ctx, 1, &J, tmp);
    if (rc == MASP_HIP_OK) memcpy(proof_out, tmp, 192);
    return rc;
}

}  // extern "C"
