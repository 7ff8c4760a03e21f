// Host-side types shared by the translation units of libmasp_hip (ctx.hip: context; circuit_load.hip: CRS loading; prove.hip: slot
// pool, launch sequences, masp_hip_prove_batch; hooks.hip: building blocks and measurement hooks; k_setup.hip: parameter generation).
// No kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "chunk_pipeline.h"
#include "column_call.h"
#include "host/eval_form.h"
#include "device/io.hpp"
#include "device/ntt_geom.h"
#include "launch.h"
#include "msm_host.h"
#include <atomic>
#include "util.h"

// block width (log2) of the subset rows behind the a, b and merged h + l window tables when a context is not told otherwise
// (masp_hip_ctx_set_boolean_block_bits, include/masp_hip.h): 0 = none, 2 or 3.  A compile-time default, so that two builds can be compared with bench.py.
// 2: blocks of four, + 1.6 % proofs/s for about 0.1 GB of tables per Spend circuit.  Blocks of eight measured + 2.2 % end to end, but take the
// Spend tables past the 3.5 GiB an XCD's gathers reach, and the kernel profile that shows the level-0 pass of h + l no slower is not yet
// taken (MEASUREMENTS.md "Boolean blocks"): 3 stays an option until it is.
#ifndef MASP_SUBSET_BITS
#define MASP_SUBSET_BITS 2
#endif
static_assert(MASP_SUBSET_BITS == 0 || MASP_SUBSET_BITS == 2 || MASP_SUBSET_BITS == 3, "subset blocks are 4 or 8 bases wide");
// Doubled window rows (msm_geom_twin, device/msm_geom.h) behind the tables that batches use, when a context is not told otherwise
// (masp_hip_ctx_set_window_row_multiples, include/masp_hip.h): bit 0 = the merged h + l sets, bit 1 = a, b_g1, b_g2.  A compile-time default,
// so that two builds can be compared with bench.py.  3, and with it 13-bit windows for a / b where the width is the loader's choice and
// would be 12: + 2.3 % proofs/s on Spend; h + l alone (+ 1.0 %) and every table at 12 bits (+ 0.7 %) did not clear the run-to-run spread
// (MEASUREMENTS.md "Doubled window rows").
#ifndef MASP_TWIN_ROWS
#define MASP_TWIN_ROWS 3
#endif
static_assert(MASP_TWIN_ROWS >= 0 && MASP_TWIN_ROWS <= 3, "bit 0: h + l, bit 1: a, b_g1, b_g2");
// Of a query's witness scalars that the R1CS does not prove boolean, the percentage taken to be full width where the bucket tree's scratch
// is sized (masp_hip_ctx_set_tree_entry_share, include/masp_hip.h).  MEASUREMENTS.md "Entry bound" has the shares observed over the three
// circuits: the largest, 98 %, with a quarter on top is past 100, so the default is every one of them.
#ifndef MASP_TREE_ENTRY_SHARE
#define MASP_TREE_ENTRY_SHARE 100
#endif
static_assert(MASP_TREE_ENTRY_SHARE >= 1 && MASP_TREE_ENTRY_SHARE <= 100, "a percentage");


namespace masp {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) dev_free(p);
        p = nullptr;
        cap = 0;
    }
    int reserve(size_t n) {
        if (n <= cap) return MASP_HIP_OK;
        release();
        HIP_TRY(dev_malloc(&p, sizeof(T) * std::max<size_t>(n, 1)));
        cap = n;
        return MASP_HIP_OK;
    }
    int upload(const T* h, size_t n, hipStream_t s) {
        int rc = reserve(n);
        if (rc) return rc;
        if (n) HIP_TRY(hipMemcpyAsync(p, h, sizeof(T) * n, hipMemcpyHostToDevice, s));
        return MASP_HIP_OK;
    }
};

// host-side Fr helpers (the device field code is __host__ __device__)
static inline Fr fr_from_u64_mont(uint64_t x) {
    Fr v = fe_zero<FrCfg>();
    v.v[0] = (uint32_t)x;
    v.v[1] = (uint32_t)(x >> 32);
    return fe_to_mont(v);
}
static inline Fr fr_const(const uint32_t* limbs) {
    Fr v;
    for (int i = 0; i < 8; ++i) v.v[i] = limbs[i];
    return v;
}

struct NttDomain {
    uint32_t logm = 0;
    size_t m = 0;
    DevBuf<Fr> tw_fwd, tw_inv, coset_scale, h_scale;
    DevBuf<Fr> coset_scale_rev;  // coset_scale in bit-reversed order: g^rev(i) / m (k_ntt_mid); only where ntt_fused_ok(logm)
    Fr c_scale;  // 1 / (m (g^m - 1)), plain form
    Fr e_scale;  // 1 / (g^m - 1), plain form (the evaluation form's only factor: k_ntt_ab_eval)
    int init(uint32_t logm_, hipStream_t s) {
        logm = logm_;
        m = (size_t)1 << logm;
        Fr omega = fr_const(FrCfg::ROOT_OF_UNITY);
        for (uint32_t i = logm; i < 32; ++i) omega = fe_sqr(omega);
        Fr omega_inv = fe_inv(omega);
        Fr minv = fe_inv(fr_from_u64_mont(m));
        Fr g = fr_const(FrCfg::GEN), ginv = fr_const(FrCfg::GEN_INV);
        uint32_t e[2] = {(uint32_t)m, (uint32_t)((uint64_t)m >> 32)};
        const Fr zinv = fe_inv(fe_sub(fe_pow(g, e, 2), fe_one<FrCfg>()));  // 1 / Z on the coset g H
        const Fr mzinv = fe_mul(minv, zinv);
        c_scale = fe_from_mont(mzinv);
        e_scale = fe_from_mont(zinv);
        Fr one = fe_one<FrCfg>();
        size_t half = std::max<size_t>(m / 2, 1);
        int rc;
        if ((rc = tw_fwd.reserve(half)) || (rc = tw_inv.reserve(half)) || (rc = coset_scale.reserve(m)) || (rc = h_scale.reserve(m))) return rc;
        launch_fr_powers(s, tw_fwd.p, (uint32_t)half, omega, one, 0);
        launch_fr_powers(s, tw_inv.p, (uint32_t)half, omega_inv, one, 0);
        launch_fr_powers(s, coset_scale.p, (uint32_t)m, g, minv, 0);
        launch_fr_powers(s, h_scale.p, (uint32_t)m, ginv, mzinv, 1);  // g^-k / (m (g^m - 1)), plain form
        if (ntt_fused_ok(logm)) {
            if ((rc = coset_scale_rev.reserve(m))) return rc;
            launch_fr_powers_bitrev(s, coset_scale_rev.p, logm, g, minv);
        }
        HIP_TRY(hipStreamSynchronize(s));
        return MASP_HIP_OK;
    }
    // np transforms at data + p * m
    void passes(hipStream_t s, Fr* data, const Fr* tw, uint32_t np = 1) const {
        for (uint32_t s0 = 0; s0 < logm;) {
            uint32_t nst = std::min<uint32_t>(NTT_LT, logm - s0);
            launch_ntt_pass(s, data, tw, logm, s0, nst, np);
            s0 += nst;
        }
    }
};

struct Circuit {
    uint32_t n_inputs = 0, n_aux = 0, n_constraints = 0, nrows = 0, logm = 0;
    size_t m = 0;
    DevBuf<uint32_t> rowptr[3], col[3];
    DevBuf<uint32_t> row_order[3];  // constraint rows by decreasing length: lanes of a wave get rows of similar length
    uint32_t n_long_rows[3] = {0, 0, 0};  // rows of >= R1CS_LONG_ROW terms (the head of row_order): a wave each
    DevBuf<Fr> coef[3];
    DevBuf<uint32_t> a_var, b_var;
    uint32_t na = 0, nbq = 0;
    DevBuf<VkDevice> vk;
    DevBuf<G1Xyzz> fb1;  // fixed-base tables of delta1, alpha1, beta1
    DevBuf<G2Xyzz> fb2;  // fixed-base table of delta2
    BasesG1 h, l, a, b1;
    // h and l as ONE base set (h's points, then l's) on h's windows: C only needs H + L, so a batch runs them as one MSM over
    // one bucket set — l's scalars then cost 16 window digits instead of 22 and its sort / bucket tails disappear
    BasesG1 hl;
    // The quotient in EVALUATION form: sum_k h_k H_k is linear in h, so the last inverse transform and all of c move into
    // the bases, once, when the circuit is loaded (k_setup.hip: build_eval_bases).  Points: [0, m) T'_i, the inverse DFT of g^-k H_k / m, in
    // the order the forward passes leave the coset evaluations; [m, m + n_aux) L'_j = L_j - Q_j / (g^m - 1) with Q = C^T (DFT of H);
    // then -Q_j / (g^m - 1) for the input columns C uses (eval_in_var).  A batch's scalars are E_i = a b / (g^m - 1) on the coset, its aux
    // assignment and those inputs.  n = 0: not built (masp_hip_ctx_set_quotient_form, or a derived point came out at infinity) — the
    // batch then runs the coefficient form on `hl`, as do jobs with caller-supplied a / b / c.
    BasesG1 hl_eval;
    DevBuf<uint32_t> eval_in_var;
    uint32_t n_eval_in = 0;
    std::vector<uint32_t> eval_inputs;   // eval_in_var on the host (masp_hip_circuit_eval_bases; the points are read back from hl_eval.tab)
    BasesG2 b2;
    // the same G2 points on narrow windows (128 buckets), for lone proofs only: B2's bucket tails are the longest chain of
    // a lone proof (every G2 addition is 40 dependent 384-bit products on one lane), and with 128 instead of 2 048 buckets
    // the gather / weighted-sum levels nearly vanish for 45 % more (chip-filling) accumulation work; n = 0: not built
    BasesG2 b2_lone;
    // a and b_g1 in the plain geometry, for lone proofs only, where the batch tables have doubled window rows: the class-wise weighted
    // sum of such a set has no quad-lane form (k_msm_twin_combine is one lane), and a lone proof waits for exactly those chains — with
    // the batch tables it took 4.0 instead of 3.8 ms.  n = 0: not built, lone proofs use a / b1.
    BasesG1 a_lone, b1_lone;
    // alpha_g1, beta_g1, delta_g1 and every point of the a / b_g1 queries lie in the prime-order subgroup (tested when the
    // circuit is loaded): s*A and r*B1 may then go through the endomorphism (k_groth16_var_mul).  A CRS with a curve point
    // outside the subgroup — the reference reads it unchecked — keeps the plain double-and-add, whose bytes are the reference's
    bool g1_endo = false;
    NttDomain* dom = nullptr;
};

// scratch for one batch of up to `ctx->batch_cap` proofs of the same circuit + a stream.  Every stage is ONE launch for the
// whole batch (gridDim.y = proofs); a few slots let the stages of different batches overlap on the device.
// A slot BORROWS its streams from its context's stream table (masp_hip_ctx::streams) and never creates or destroys one.
struct Slot {
    hipStream_t stream = nullptr;
    Event done;
    MsmWorkspace<FpOps> ws1;
    MsmWorkspace<Fp2Ops> ws2;
    // lone-proof mode (a batch too small to fill the chip): the five MSMs run side by side on their own streams, each
    // with its own workspace, next to the quotient pipeline on the main stream
    static constexpr int N_AUX = 4;
    hipStream_t aux[N_AUX] = {nullptr, nullptr, nullptr, nullptr};
    Event ev_fork, ev_sort_b, ev_fixed, ev_join[N_AUX];
    Event ev_uploaded;   // behind the host-to-device copies of this slot's batch (masp_hip_ctx::upload_tail)
    MsmWorkspace<FpOps> ws_l, ws_a, ws_b;
    DevBuf<Fr> w, inp, abc, wm, ev[3], x0, x1, h, hl, sa, sb;
    DevBuf<G1Xyzz> res1, asm1;  // asm1: the six G1 pieces of the assembly per proof, asm2: s*delta2
    DevBuf<G2Xyzz> res2, asm2;
    DevBuf<uint32_t> rs;
    DevBuf<uint8_t> proof;
    DevBuf<int> flags;
    MsmProfile prof;             // live HIP-event timing of k_msm_accumulate<G1> (bench roofline leg)
    bool profiling = false;
    // where a LONE proof's chains end, without a profiler in the way (rocprofv3 adds ~10 us per launch, which reorders five chains of
    // ~60 launches each): timing events recorded behind the stages of the last lone proof while profiling is on
    // (masp_hip_profile_read_lone).  Created on first use.
    static constexpr int N_LONE_MARKS = 12;
    Event ev_lone[N_LONE_MARKS];
    bool lone_marked = false;
    void lone_mark(hipStream_t st, int id) {
        if (!profiling) return;
        if (ev_lone[id].create() != MASP_HIP_OK) return;
        (void)hipEventRecord(ev_lone[id], st);
        if (id == N_LONE_MARKS - 1) lone_marked = true;
    }
    uint32_t ntt_sub = 8;        // masp_hip_options::ntt_sub_batch of the owning context (0 = whole batch)
    const std::atomic<int>* quotient_schedule = nullptr;  // the owning context's (masp_hip_ctx_set_quotient_schedule)
    PinnedBuf<uint8_t> h_stage;  // pinned staging for the assignment
    PinnedBuf<uint8_t> h_proof;  // batch_cap x 192
    PinnedBuf<int> h_flags;
    // Launch graphs of lone proofs (prove.hip: enqueue_proofs_graphed; opt-in).  The ~250 launches of one proof take the
    // host about as long to enqueue as the GPU takes to run them; captured once per (circuit, buffers, form) they replay as
    // one hipGraphLaunch.  A graph holds raw pointers into workspaces that grow on demand: `graph_epoch` is the value of
    // device_alloc_epoch() it was captured under, and any later allocation or release drops every graph of the slot.
    struct LoneGraph {
        const void *circuit, *w, *abc, *rs, *proof;
        size_t w_stride;
        uint32_t np;
        bool mont;
        int runs;                // ungraphed runs so far (the first one sizes every buffer)
        bool dead;               // capture failed once: not tried again
        hipGraphExec_t exec;
    };
    std::vector<LoneGraph> graphs;
    uint64_t graph_epoch = 0;
    bool lone_graph = false;     // masp_hip_options::lone_proof_graph
    std::atomic<uint64_t> graph_launches{0};
    void drop_graphs() {
        for (auto& g : graphs)
            if (g.exec) hipGraphExecDestroy(g.exec);
        graphs.clear();
    }
    ~Slot() { drop_graphs(); }
    // the options of the owning context that the slot's launch sequences depend on
    void configure(const masp_hip_options& o) {
        ntt_sub = (uint32_t)o.ntt_sub_batch;
        ws1.tree_levels = o.bucket_tree_levels;
        ws2.tree_levels = o.bucket_tree_levels_g2;
        ws1.tree_levels_shared = o.bucket_tree_levels_g2;  // B2 is reduced from B1's sort (ws1.sort): padded if either wants a tree
        ws1.tree_sub = ws2.tree_sub = (uint32_t)o.bucket_tree_sub_batch;   // (0: resolved per base set, msm_reduce_enqueue)
        ws2.tree.arena = &ws1.tree.own;   // the G1 and G2 MSMs of a batch follow each other on the slot's stream: one tree arena
        ws1.tree.own.limit = (size_t)o.bucket_tree_scratch_mb << 20;
        lone_graph = o.lone_proof_graph > 0;
    }
    // `streams`: this slot's row of the context's stream table (main, then the four side streams), borrowed for the slot's life.
    // (The side streams exist before the slot's first lone proof.  Creating them at that proof instead — so that a batch prover holds one
    // stream per slot — was measured in round 6: batch throughput equal, lone proofs 4.1 - 4.2 instead of 3.6 - 3.7 ms inside bench.py,
    // equal in the standalone tool; not understood, not kept: profiles/r06_second_context_root_cause.txt.)
    int init(const std::array<hipStream_t, 5>& streams) {
        stream = streams[0];
        for (int i = 0; i < N_AUX; ++i) aux[i] = streams[1 + i];
        int rc;
        for (Event* e : {&done, &ev_fork, &ev_uploaded, &ev_sort_b, &ev_fixed})
            if ((rc = e->create(hipEventDisableTiming))) return rc;
        if ((rc = create_events(ev_join, hipEventDisableTiming)) || (rc = h_flags.reserve(1)) || (rc = flags.reserve(1))) return rc;
        return reserve_batch(1);
    }
    int reserve_batch(size_t np) {
        int rc;
        if ((rc = res1.reserve(4 * np)) || (rc = res2.reserve(np)) || (rc = asm1.reserve(6 * np)) || (rc = asm2.reserve(np)) || (rc = rs.reserve(16 * np)) || (rc = proof.reserve(192 * np))) return rc;
        return h_proof.reserve(192 * np);
    }
};

struct ResidentBatch {
    size_t n = 0;
    std::vector<uint32_t> circuit;  // in STORAGE order: jobs are stored grouped by circuit so that batches are strided
    std::vector<size_t> order;      // storage position -> caller's job index
    std::vector<size_t> w_off;      // element offsets into w
    DevBuf<Fr> w;
    DevBuf<uint32_t> rs;        // n x 16
};

// Every stream of a device context, as plain handles (masp_hip_ctx::streams).  The table destroys each DISTINCT handle once, with the
// context; the only other place that destroys one is separate_main_streams, when it replaces a main stream in place.
struct StreamTable {
    hipStream_t main = nullptr;                     // the context's own
    std::vector<std::array<hipStream_t, 5>> slot;   // per slot: [0] main, [1..4] side streams (several rows may hold the same side streams)
    hipStream_t vk[2] = {nullptr, nullptr};         // the batch verifier's keys (masp_hip_vk_prepare hands them out in turn)
    std::vector<hipStream_t> distinct() const {
        std::vector<hipStream_t> out;
        auto add = [&](hipStream_t s) {
            if (s && std::find(out.begin(), out.end(), s) == out.end()) out.push_back(s);
        };
        add(main);
        for (const auto& row : slot)
            for (hipStream_t s : row) add(s);
        for (hipStream_t s : vk) add(s);
        return out;
    }
    ~StreamTable() {
        for (hipStream_t s : distinct()) (void)hipStreamDestroy(s);
    }
};

// A device table that is uploaded once per context by whichever call needs it first.  `fresh`: this call enqueued the upload and nothing has
// confirmed yet that it arrived; WalletState::settle_tables decides at the end of the call.
template <class T>
struct OnceTable : DevBuf<T> {
    bool fresh = false;
    int ensure(const T* h, size_t n, hipStream_t s) {
        if (this->p) return MASP_HIP_OK;
        fresh = true;
        return this->upload(h, n, s);
    }
};

// What the Jubjub entry points (k_redjubjub.hip: masp_hip_jubjub_msm, masp_hip_redjubjub_verify_batch, masp_hip_redjubjub_verify_each;
// k_bundle_check.hip: masp_hip_sapling_check_bundles) keep between calls.  They run next to proving calls on the verifier stream
// streams.vk[1], one at a time per context: `mu` guards every member but the timing record and is taken behind the context's.  The work
// buffers grow on demand and are kept.
struct JubjubState {
    std::mutex mu;
    DevBuf<uint8_t> points, scalars, partial;
    DevBuf<int> status;
    DevBuf<uint32_t> out;
    // the bundle pre-check: a call's arrays as they come, what its kernels hand each other, its results, and one chunk of proof bytes
    DevBuf<uint8_t> bc_in, bc_work, bc_out, bc_proofs;
    LastTiming<3> bc_timing;          // masp_hip_check_bundles_last_timing: upload, kernels, download
};

// What a per-item call (column_call.h, column_host.h) keeps between calls: a chunk's arrays as they come, the per-item state, the results
// as they leave with the status bytes last, and the pinned staging of the secret inputs if it has any (it, the uploaded inputs and the
// state are zeroed before such a call releases the lock).  Every buffer holds ColumnCall::n_pad items.
struct PerItemCall {
    DevBuf<uint8_t> in, state, out;
    PinnedBuf<uint8_t> stage;
    std::atomic<size_t> chunk{0};   // the call's configure: items per chunk, 0 = the default
    LastTiming<3> timing;           // the call's last_timing: upload, kernels, download
    // room for cc's chunks with state_bytes of state an item; cc gets the buffers
    int reserve(ColumnCall& cc, size_t state_bytes) {
        const size_t n = cc.n_pad;
        int rc;
        if ((rc = in.reserve(cc.iw.total * n)) || (rc = state.reserve(state_bytes * n)) || (rc = out.reserve(cc.ow.total * n)) || (rc = stage.reserve(cc.iw.stage_total * n)))
            return rc;
        cc.d_in = in.p, cc.d_out = out.p, cc.stage = stage.p;
        return MASP_HIP_OK;
    }
};

// What the wallet-side entry points of a device context keep between calls: the note scan (k_note_scan.hip), the compact note scan
// (k_note_scan_compact.hip), the output recovery scan (k_out_recovery.hip), the commitment trees (k_merkle.hip), the note nullifiers
// (k_nullifier.hip), the allowed conversions (k_conversion.hip), the output descriptions (k_output_build.hip) and the spend descriptions with their signatures (k_spend_build.hip).  One of these calls runs at a time per context: `mu` guards every member but the atomics and the timing records, and is
// taken by WalletCall alone.  The scans alternate their chunks between the two verifier streams (streams.vk), each with a buffer set of its
// own; the trees, the nullifiers, the conversions, the output and the spend descriptions run on streams.vk[0].  Every buffer grows on demand and is kept.
struct WalletState {
    std::mutex mu;
    struct NoteScanSet {
        DevBuf<uint8_t> epk, raw, ct, pts, status, hit_keys;
        DevBuf<uint32_t> count, hit_idx;
    };
    NoteScanSet ns[2];
    DevBuf<uint32_t> ns_digits;
    std::atomic<int> ns_signed_digits{1}, ns_inversion{0};   // masp_hip_note_scan_configure; the defaults are the measured winners (KERNELS.md)
    LastTiming<2> ns_timing;                                 // masp_hip_note_scan_last_timing: upload, kernels
    // the compact scan decodes the epks into ns[set].epk / pts / status; what it has beyond that: per set the cmus, the 84-byte rows, the
    // candidate list of stage 1 and the per-candidate state of stage 2 (sized for the launch's pair count), the survivor lists and the final hits
    struct NoteScanCompactSet {
        DevBuf<uint8_t> cmu, enc, cand, state, hit_idx, hit_data;
        DevBuf<uint32_t> count, list;
    };
    NoteScanCompactSet nsc[2];
    DevBuf<uint8_t> nsc_ivks;         // the ivks as they come: stage 2's per-lane scalars
    OnceTable<uint8_t> nsc_table;     // the Pedersen Niels table and G_ncr behind it (pedersen_table.h): the compact scan, the trees, the nullifiers, the conversions
    LastTiming<3> nsc_timing;         // masp_hip_note_scan_compact_last_timing: upload, stage 1, stage 2
    // output recovery: per set the rows as they come (cv, cmu, epk 32 bytes each, out_ciphertext 80), their eleven 16-byte columns, and the hits
    struct OutRecoverySet {
        DevBuf<uint8_t> cv, cmu, epk, cout, cols, hit_ocks;
        DevBuf<uint32_t> count, hit_idx;
    };
    OutRecoverySet orc[2];
    DevBuf<uint32_t> orc_ovks;        // the ovks, eight words each: the kernel's wave-uniform message words
    LastTiming<2> orc_timing;         // masp_hip_out_recovery_last_timing: upload, kernels
    // the trees: the node vector (eight words a node), the first bad input's index, the positions and their paths, empty_root(0..32)
    DevBuf<uint32_t> mt_nodes, mt_bad, mt_paths;
    OnceTable<uint32_t> mt_empties;
    DevBuf<uint64_t> mt_pos;
    LastTiming<3> mt_timing;          // masp_hip_merkle_last_timing: upload, kernels, download
    // the nullifiers: a table of their own beside nsc_table (nullifier_table.h: the windows of G_ncr and G_nf)
    OnceTable<uint8_t> nf_table;
    PerItemCall nf;
    std::atomic<int> nf_lanes{0};     // masp_hip_note_nullifiers_configure: lanes per note, 0 = by the number of notes
    // the allowed conversions (k_conversion.hip), on nsc_table's Pedersen points: a chunk's offsets, identifiers and values as they come, the
    // terms' points with their status bytes behind them, and generator | cmu | status
    DevBuf<uint8_t> cv_in, cv_terms, cv_out;
    std::atomic<int> cv_lanes{0};     // masp_hip_allowed_conversions_configure: lanes per conversion, 0 = by the number of conversions
    std::atomic<size_t> cv_chunk_conv{0}, cv_chunk_terms{0};   // ... and a chunk's limits, 0 = the defaults
    LastTiming<3> cv_timing;          // masp_hip_allowed_conversions_last_timing: upload, kernels, download
    // the output descriptions (k_output_build.hip), on nsc_table's Pedersen points and nf_table's G_ncr windows: G_vcr's windows
    // (output_table.h), the memos as they come and in columns, and the two ciphertexts in columns
    OnceTable<uint8_t> ob_table;
    PerItemCall ob;
    DevBuf<uint8_t> ob_memo, ob_cols;
    // the spend descriptions and the RedJubjub signatures (k_spend_build.hip), on the tables above: the windows of G_spend and G_pgk (spend_table.h)
    OnceTable<uint8_t> sb_table;
    PerItemCall sb, rs;
    // The end of a call that may have uploaded tables: one that failed with a HIP error cannot tell whether they arrived, so they are released
    // and the next call uploads them again; any other end confirms them.  A table of an earlier call is not marked and survives either way.
    void settle_tables(int rc) {
        auto settle = [rc](auto& t) {
            if (t.fresh && rc == MASP_HIP_E_HIP) t.release();
            t.fresh = false;
        };
        settle(nsc_table);
        settle(mt_empties);
        settle(nf_table);
        settle(ob_table);
        settle(sb_table);
    }
};

}  // namespace masp

using masp::Circuit;
using masp::DevBuf;
using masp::Fr;
using masp::G1Affine;
using masp::G1Xyzz;
using masp::G2Affine;
using masp::G2Xyzz;
using masp::NttDomain;
using masp::ResidentBatch;
using masp::Slot;

// Locking: `mu` is held SHARED by masp_hip_prove_batch (any number of host threads prove concurrently, each batch on
// its own slot = stream + scratch) and EXCLUSIVE by everything that changes circuits or uses the shared scratch.  The
// slot pool has its own small lock (`slot_mu`); `err` is read and written under it.  `slots` / `slot_busy` are reserved
// to MAX_SLOTS at creation and never reallocate, so a prover thread may keep indexing them while another one adds a slot.
struct masp_hip_ctx {
    static constexpr size_t MAX_SLOTS = 64;
    int device = 0;
    // multi-device front (masp_hip_ctx_create_multi): one full context per device; this object only shards and forwards
    std::vector<masp_hip_ctx*> children;
    masp_hip_options opt{};   // resolved at creation (ctx.hip: resolve_options); the library reads no environment
    // block width (log2) of the subset rows behind the tables of circuits loaded from now on, resolved: 0 = none, 2 or 3
    // (masp_hip_ctx_set_boolean_block_bits; the build's default is MASP_SUBSET_BITS)
    int boolean_block_bits = MASP_SUBSET_BITS;
    // which of the next loaded circuit's batch tables get doubled window rows: bit 0 = h + l, bit 1 = a, b_g1, b_g2
    // (masp_hip_ctx_set_window_row_multiples; the build's default is MASP_TWIN_ROWS)
    int twin_rows = MASP_TWIN_ROWS;
    // the building-block MSM entry points (masp_hip_msm_g1_multi ...) double their rows only when told so explicitly: set(ctx, 1)
    bool twin_rows_msm = false;
    // the quotient's form for circuits loaded from now on: 0 = evaluation form, 1 = coefficient form (masp_hip_ctx_set_quotient_form)
    int quotient_form = 0;
    // how a batch in evaluation form runs its transforms: 0 = the three fused kernels, 1 = the separate passes (masp_hip_ctx_set_quotient_schedule);
    // read when a batch is enqueued
    std::atomic<int> quotient_schedule{0};
    // of a query's witness scalars that the R1CS does not prove boolean, the percentage that the bucket tree's scratch takes to be full
    // width, for circuits loaded from now on (masp_hip_ctx_set_tree_entry_share; the default: MASP_TREE_ENTRY_SHARE)
    int tree_entry_share = MASP_TREE_ENTRY_SHARE;
    int n_slots = 4;          // = opt.slots
    size_t batch_cap = 256;   // = opt.batch_cap
    std::shared_mutex mu;
    mutable std::mutex slot_mu;
    std::condition_variable slot_cv;
    std::vector<char> slot_busy;
    std::string err;
    // Every stream the context uses, in one table: the context CREATES all of them when it is created (create_single), slot by slot, and
    // the table destroys them with it, after the slots (declared before them).  A slot borrows its row when it is created — a failed
    // attempt leaves the row as it was — and never creates or destroys a stream.  The main streams are then MEASURED and, where two share
    // a hardware queue, replaced in place (separate_main_streams): the runtime hands hardware queues to streams in creation order, so the
    // main streams — the ones that carry batches — get queues of their own whatever the process created before (round 6: with 21 streams
    // created slot by slot over 16 queues, a later context of a process could find two of its main streams on one queue: -3.5 % at 4 slots).
    // Slots 0 and 1 have side streams of their own; from slot 2 on a slot's row holds slot 1's (a lone proof takes the first free slot, so
    // three lone proofs must be in flight at once before two of them share side streams — they then interleave on them, each behind its own
    // events).  A default context so has 1 + 4 + 8 + 2 = 15 streams: one hardware queue each of the default 16, nothing shares.  (With
    // masp_hip_options::lone_proof_graph every slot has its own: a stream that is being captured cannot take another thread's launches.)
    // The verifier's two: a verification that shared a hardware queue with a slot's main stream waited behind a 185 ms batch (end to end -10 %).
    masp::StreamTable streams;
    std::unique_ptr<Circuit> circ[MASP_HIP_MAX_CIRCUITS];
    std::map<uint32_t, std::unique_ptr<NttDomain>> domains;
    std::vector<std::unique_ptr<Slot>> slots;
    std::vector<std::unique_ptr<ResidentBatch>> batches;
    bool profiling = false;
    std::atomic<uint64_t> proofs_done{0};   // proofs this device context has written (masp_hip_ctx_device_proofs)
    // multi-device front: MASP_HIP_OK or the error that took device context d out (prove_batch_multi), and the proofs it put back on the queue
    std::unique_ptr<std::atomic<int>[]> dev_status;
    std::atomic<uint64_t> requeued{0};
    // device context: the n-th masp_hip_prove_batch call from now fails before it touches the device (masp_hip_ctx_inject_fault; 0 = disarmed)
    std::atomic<uint32_t> fault_countdown{0};
    std::atomic<unsigned> vk_next{0};   // which verifier stream the next key gets
    int main_streams_concurrent = 0;   // of the 1 + slots streams that carry batches, how many ran at once when the context was created
    // Host-to-device copies of concurrent masp_hip_prove_batch calls go ONE BATCH AFTER THE OTHER: a batch's copies wait for the event
    // behind the previous batch's copies (whatever slot that was).  Three calls that start together (the beginning of a job list, of a
    // timed region) otherwise share the link, and none of them can start computing before all 3 x 820 MB have crossed it.
    std::mutex upload_mu;
    hipEvent_t upload_tail = nullptr;   // an event of some slot of this context (slots live as long as the context)
    // the building-block MSM entry points (masp_hip_msm_g1_multi ...) run on a workspace of their own: what lack of tree scratch did there
    std::atomic<uint64_t> block_tree_fallbacks{0};
    std::atomic<uint32_t> block_tree_sub{0xffffffffu};
    // scratch for the building-block entry points
    DevBuf<Fr> tmp_scalars;
    DevBuf<uint8_t> tmp_out;
    DevBuf<G1Xyzz> tmp_g1;
    DevBuf<G2Xyzz> tmp_g2;
    // fixed-base tables of the standard generators (parameter generation)
    DevBuf<G1Affine> fb_g1;
    DevBuf<G2Affine> fb_g2;
    masp::JubjubState jj;       // the Jubjub calls' state, under a lock of its own
    masp::WalletState wallet;   // the wallet-side calls' state, under a lock of its own
};

namespace masp {

static inline int fail(masp_hip_ctx* ctx, int rc) {
    if (rc == MASP_HIP_E_HIP) {
        std::lock_guard<std::mutex> g(ctx->slot_mu);
        ctx->err = last_hip_error();
    }
    return rc;
}

// the context a single-device entry point works on: a multi-device front's first device context
#define FIRST_DEVICE(ctx) ((ctx) && !(ctx)->children.empty() ? (ctx)->children[0] : (ctx))

// The opening of every entry point that launches kernels, in this order: the launch scope, the first device's context, its `mu` — SHARED
// next to provers, verifiers and wallet calls, EXCLUSIVE for what changes circuits or uses the shared scratch —, the device.  A second mutex
// (a key's, JubjubState::mu, WalletState::mu) is taken behind it.  Argument checks that need no lock stand in front; once the call is open,
// done(rc) is its only way out: success is reported only if no launch was refused (util.h: ApiLaunchScope), and this is the one place that
// calls fail().  Helpers return their rc to the entry point and never call fail() themselves.
enum class CtxLock { SHARED, EXCLUSIVE };
struct ApiCall {
    const ApiLaunchScope scope;
    masp_hip_ctx* const ctx;
    std::shared_lock<std::shared_mutex> shared;
    std::unique_lock<std::shared_mutex> exclusive;
    ApiCall(masp_hip_ctx* c, CtxLock kind) : ctx(FIRST_DEVICE(c)), shared(ctx->mu, std::defer_lock), exclusive(ctx->mu, std::defer_lock) {
        if (kind == CtxLock::SHARED)
            shared.lock();
        else
            exclusive.lock();
        hipSetDevice(ctx->device);
    }
    int done(int rc) {
        if (rc == MASP_HIP_OK) rc = launch_status();
        return rc ? fail(ctx, rc) : MASP_HIP_OK;
    }
};

// a wallet-side entry point: an ApiCall next to provers and verifiers, the wallet lock, and the uploaded-once tables settled on the way out
struct WalletCall : ApiCall {
    std::lock_guard<std::mutex> wlock;
    WalletState& w;
    explicit WalletCall(masp_hip_ctx* c) : ApiCall(c, CtxLock::SHARED), wlock(ctx->wallet.mu), w(ctx->wallet) {}
    int done(int rc) {
        rc = ApiCall::done(rc);
        w.settle_tables(rc);
        return rc;
    }
};

static inline int get_domain(masp_hip_ctx* ctx, uint32_t logm, NttDomain** out) {
    auto it = ctx->domains.find(logm);
    if (it == ctx->domains.end()) {
        std::unique_ptr<NttDomain> d(new NttDomain);
        int rc = d->init(logm, ctx->streams.main);
        if (rc) return rc;
        it = ctx->domains.emplace(logm, std::move(d)).first;
    }
    *out = it->second.get();
    return MASP_HIP_OK;
}

// The bases of the quotient's evaluation form for one circuit (Circuit::hl_eval), derived on the device from the h and l queries
// (uncompressed, m - 1 and n_aux points on the host) and the R1CS matrix C: two group-valued transforms over G1, the sparse combine, one
// normalisation.  d_raw: lay.n() uncompressed points on the device.  usable: none of them is the point at infinity.   [k_setup.hip]
struct EvalBases {
    DevBuf<uint8_t> d_raw;
    EvalLayout lay;
    bool usable = false;
};
int build_eval_bases(masp_hip_ctx* ctx, const NttDomain& D, const uint8_t* h_raw, const uint8_t* l_raw, const masp_hip_r1cs* cs, EvalBases& out);

// the note scan's limits (its geometry: chunk_pipeline.h) and the pieces its two units share (defined in k_note_scan.hip)
constexpr size_t NS_MAX_IVKS = 4096;
constexpr size_t NS_MAX_OUTPUTS = (size_t)1 << 26;
// the digit masks of the trial kernels for n_ivk ivks (16 words each); MASP_HIP_E_INVALID_ARG if one is not below r_J
int ns_recode_ivks(std::vector<uint32_t>& digits, size_t n_ivk, const uint8_t* ivks, bool signed_digits);
// k_ns_decode over n epks of 32 bytes: a status byte and the Niels form (96 bytes) per output
void launch_ns_decode(hipStream_t s, const uint8_t* epks, uint32_t n, uint8_t* status, uint8_t* pts);

static inline uint32_t log2_ceil(uint32_t n) {
    uint32_t k = 0;
    while ((1ull << k) < n) ++k;
    return k;
}

}  // namespace masp
