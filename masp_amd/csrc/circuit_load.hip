// libmasp_hip: CRS parsing and circuit loading — the bellman Parameters bytes and the static R1CS become the device tables a proof
// reads (masp_hip_circuit_load), and the queries about a loaded circuit.
#include "internal.h"

using namespace masp;

namespace {

// ---- what a witness can put into a digit list --------------------------------------------------------------------------------
// out[v] = 1 where the R1CS proves variable v boolean, by the constraints bellman's boolean gadgets leave:
//   ONE itself;
//   k v (c - c v) = 0, the C row empty (AllocatedBit::alloc): one of the A and B rows the single term v, the other ONE and v with
//     coefficients that cancel;
//   f(x) g(y) = z with f, g each t or 1 - t over variables already proven boolean (AllocatedBit::and, and_not, nor);
//   2 x y = x + y - z over such variables (AllocatedBit::xor).
// Such a scalar is 0 or 1 in every satisfying witness: at most one entry of a digit list, whatever the window width.  (Passes over the
// constraints until nothing changes: a gadget's operands are allocated before its result, so the second pass finds nothing new.)
static void r1cs_boolean_variables(const masp_hip_r1cs* cs, uint8_t* out) {
    // r, little-endian: two canonical non-zero coefficients cancel exactly when their sum as integers is r
    static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0x02, 0xa4, 0xbd, 0x53,
                                     0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8, 0x39, 0x33, 0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73};
    static const uint8_t ONE_LE[32] = {1};
    const uint32_t nv = cs->n_inputs + cs->n_aux, NONE = 0xffffffffu;
    memset(out, 0, nv);
    out[0] = 1;
    auto cancel = [&](const uint8_t* x, const uint8_t* y) {
        unsigned carry = 0;
        for (int i = 0; i < 32; ++i) {
            const unsigned t = (unsigned)x[i] + y[i] + carry;
            if ((uint8_t)t != R_LE[i]) return false;
            carry = t >> 8;
        }
        return carry == 0;
    };
    auto small = [&](const uint8_t* x, uint8_t k) {
        if (x[0] != k) return false;
        for (int i = 1; i < 32; ++i)
            if (x[i]) return false;
        return true;
    };
    auto minus_one = [&](const uint8_t* x) { return cancel(x, ONE_LE); };
    const uint32_t* rp[3] = {cs->a_rowptr, cs->b_rowptr, cs->c_rowptr};
    const uint32_t* cl[3] = {cs->a_col, cs->b_col, cs->c_col};
    const uint8_t* cf[3] = {cs->a_coef, cs->b_coef, cs->c_coef};
    auto len = [&](int mi, uint32_t i) { return rp[mi][i + 1] - rp[mi][i]; };
    auto col = [&](int mi, uint32_t i, uint32_t k) { return cl[mi][rp[mi][i] + k]; };
    auto coef = [&](int mi, uint32_t i, uint32_t k) { return cf[mi] + 32 * (size_t)(rp[mi][i] + k); };
    // row i of matrix mi as t or 1 - t: the variable t (not ONE), else NONE
    auto form = [&](int mi, uint32_t i) -> uint32_t {
        if (len(mi, i) == 1) return col(mi, i, 0) != 0 && small(coef(mi, i, 0), 1) ? col(mi, i, 0) : NONE;
        if (len(mi, i) != 2) return NONE;
        for (uint32_t k = 0; k < 2; ++k)
            if (col(mi, i, k) == 0 && col(mi, i, k ^ 1) != 0 && small(coef(mi, i, k), 1) && minus_one(coef(mi, i, k ^ 1))) return col(mi, i, k ^ 1);
        return NONE;
    };
    for (int pass = 0; pass < 8; ++pass) {
        bool changed = false;
        auto prove = [&](uint32_t v) {
            if (v < nv && !out[v]) {
                out[v] = 1;
                changed = true;
            }
        };
        for (uint32_t i = 0; i < cs->n_constraints; ++i) {
            if (len(2, i) == 0) {
                for (int one = 0; one < 2; ++one) {   // `one`: the matrix with the single term
                    const int two = one ^ 1;
                    if (len(one, i) != 1 || len(two, i) != 2) continue;
                    const uint32_t v = col(one, i, 0), x = col(two, i, 0), y = col(two, i, 1);
                    if (v == 0 || v >= nv || !((x == 0 && y == v) || (x == v && y == 0))) continue;
                    if (cancel(coef(two, i, 0), coef(two, i, 1))) prove(v);
                }
            } else if (len(2, i) == 1) {
                const uint32_t z = col(2, i, 0), x = form(0, i), y = form(1, i);
                if (z != 0 && small(coef(2, i, 0), 1) && x != NONE && y != NONE && x < nv && y < nv && out[x] && out[y]) prove(z);
            } else if (len(2, i) == 3 && len(0, i) == 1 && len(1, i) == 1) {
                const uint32_t x = col(0, i, 0), y = col(1, i, 0);
                if (x == 0 || y == 0 || x == y || x >= nv || y >= nv || !out[x] || !out[y] || !small(coef(0, i, 0), 2) || !small(coef(1, i, 0), 1)) continue;
                uint32_t z = NONE;
                bool ok = true, sx = false, sy = false;
                for (uint32_t k = 0; k < 3; ++k) {
                    const uint32_t v = col(2, i, k);
                    if (v == x && small(coef(2, i, k), 1)) sx = true;
                    else if (v == y && small(coef(2, i, k), 1)) sy = true;
                    else if (v != 0 && z == NONE && minus_one(coef(2, i, k))) z = v;
                    else ok = false;
                }
                if (ok && sx && sy && z != NONE) prove(z);
            }
        }
        if (!changed) break;
    }
}
// The entry bound of a base set of n points on windows of `window_bits` (MsmBases::ent_bound): n_witness of its scalars are witness values,
// n_boolean of those proven boolean, and of the rest share_percent in a hundred can be full width — like every scalar that is no witness value
static uint64_t tree_entry_bound(uint32_t n, int window_bits, uint32_t n_witness, uint32_t n_boolean, int share_percent) {
    n_witness = std::min(n_witness, n);
    n_boolean = std::min(n_boolean, n_witness);
    const uint64_t rest = n_witness - n_boolean;
    const uint64_t n_full = (n - n_witness) + (rest * (uint64_t)share_percent + 99) / 100;
    return BasesG1::entry_bound(n, msm_geom(window_bits), n_full);
}

struct ParamsLayout {
    const uint8_t *alpha_g1, *beta_g1, *beta_g2, *gamma_g2, *delta_g1, *delta_g2;
    const uint8_t *ic, *h, *l, *a, *b_g1, *b_g2;
    uint32_t n_ic, n_h, n_l, n_a, n_b1, n_b2;
};
static bool read_u32be(const uint8_t*& p, const uint8_t* end, uint32_t& v) {
    if (end - p < 4) return false;
    v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    p += 4;
    return true;
}
// bellman Parameters wire format; trailing bytes are ignored like lib.rs:343-347 does
static bool parse_params(const uint8_t* buf, size_t len, ParamsLayout& L) {
    const uint8_t *p = buf, *end = buf + len;
    if (len < 864) return false;
    L.alpha_g1 = p; p += 96;
    L.beta_g1 = p;  p += 96;
    L.beta_g2 = p;  p += 192;
    L.gamma_g2 = p; p += 192;
    L.delta_g1 = p; p += 96;
    L.delta_g2 = p; p += 192;
    struct { const uint8_t** ptr; uint32_t* n; size_t sz; } secs[6] = {
        {&L.ic, &L.n_ic, 96}, {&L.h, &L.n_h, 96}, {&L.l, &L.n_l, 96}, {&L.a, &L.n_a, 96}, {&L.b_g1, &L.n_b1, 96}, {&L.b_g2, &L.n_b2, 192}};
    for (auto& sec : secs) {
        if (!read_u32be(p, end, *sec.n)) return false;
        if ((size_t)(end - p) < (size_t)*sec.n * sec.sz) return false;
        *sec.ptr = p;
        p += (size_t)*sec.n * sec.sz;
    }
    return true;
}

}  // namespace

extern "C" {

int masp_hip_r1cs_boolean_variables(const masp_hip_r1cs* cs, uint8_t* out) {
    if (!cs || !out || cs->n_inputs == 0) return MASP_HIP_E_INVALID_ARG;
    r1cs_boolean_variables(cs, out);
    return MASP_HIP_OK;
}
uint64_t masp_hip_tree_entry_bound(uint32_t n, int32_t window_bits, uint32_t n_witness, uint32_t n_boolean, int32_t share_percent) {
    if (window_bits < 2 || window_bits > 16 || share_percent < 0 || share_percent > 100) return 0;
    return tree_entry_bound(n, window_bits, n_witness, n_boolean, share_percent == 0 ? (int)(MASP_TREE_ENTRY_SHARE) : share_percent);
}
int masp_hip_circuit_tree_entry_bounds(const masp_hip_ctx* ctx, uint32_t slot, uint64_t bounds[4], int32_t window_bits[4]) {
    if (!ctx || !bounds) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return masp_hip_circuit_tree_entry_bounds(ctx->children[0], slot, bounds, window_bits);
    std::shared_lock<std::shared_mutex> lock(const_cast<masp_hip_ctx*>(ctx)->mu);
    if (slot >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[slot]) return MASP_HIP_E_NOT_LOADED;
    const Circuit& C = *ctx->circ[slot];
    const BasesG1& HL = C.hl_eval.n ? C.hl_eval : C.hl;
    const uint64_t b[4] = {HL.ent_bound, C.a.ent_bound, C.b1.ent_bound, C.b2.ent_bound};
    const int c[4] = {HL.g.c, C.a.g.c, C.b1.g.c, C.b2.g.c};
    for (int i = 0; i < 4; ++i) {
        bounds[i] = b[i];
        if (window_bits) window_bits[i] = c[i];
    }
    return MASP_HIP_OK;
}

int masp_hip_circuit_load(masp_hip_ctx* ctx, uint32_t slot, const uint8_t* params, size_t params_len, const masp_hip_r1cs* cs) {
    if (!ctx || !params || !cs || slot >= MASP_HIP_MAX_CIRCUITS || cs->n_inputs == 0) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) {  // the CRS is replicated: every device builds its own window tables, side by side
        std::vector<int> rcs(ctx->children.size(), MASP_HIP_OK);
        std::vector<std::thread> th;
        for (size_t d = 0; d < ctx->children.size(); ++d)
            th.emplace_back([&, d] { rcs[d] = masp_hip_circuit_load(ctx->children[d], slot, params, params_len, cs); });
        for (auto& t : th) t.join();
        for (int rc : rcs)
            if (rc) return rc;
        return MASP_HIP_OK;
    }
    ApiCall call(ctx, CtxLock::EXCLUSIVE);
    hipStream_t s = ctx->streams.main;
    ParamsLayout L;
    if (!parse_params(params, params_len, L)) return call.done(MASP_HIP_E_PARAMS_FORMAT);
    std::unique_ptr<Circuit> C(new Circuit);
    C->n_inputs = cs->n_inputs;
    C->n_aux = cs->n_aux;
    C->n_constraints = cs->n_constraints;
    C->nrows = cs->n_constraints + cs->n_inputs;
    C->logm = log2_ceil(C->nrows);
    C->m = (size_t)1 << C->logm;
    // density lists from the static structure (bellperson DensityTracker)
    const uint32_t nv = cs->n_inputs + cs->n_aux;
    std::vector<uint8_t> a_dense(nv, 0), b_dense(nv, 0);
    const uint32_t* rp[3] = {cs->a_rowptr, cs->b_rowptr, cs->c_rowptr};
    const uint32_t* cl[3] = {cs->a_col, cs->b_col, cs->c_col};
    const uint8_t* cf[3] = {cs->a_coef, cs->b_coef, cs->c_coef};
    for (int mi = 0; mi < 3; ++mi) {
        uint32_t nnz = rp[mi][cs->n_constraints];
        for (uint32_t t = 0; t < nnz; ++t) {
            if (cl[mi][t] >= nv) return call.done(MASP_HIP_E_INVALID_ARG);
            if (mi == 0) a_dense[cl[mi][t]] = 1;
            if (mi == 1) b_dense[cl[mi][t]] = 1;
        }
    }
    std::vector<uint32_t> a_var, b_var;
    for (uint32_t i = 0; i < cs->n_inputs; ++i) a_var.push_back(i);  // inputs are always dense for A
    for (uint32_t v = cs->n_inputs; v < nv; ++v)
        if (a_dense[v]) a_var.push_back(v);
    for (uint32_t v = 0; v < nv; ++v)
        if (b_dense[v]) b_var.push_back(v);
    C->na = a_var.size();
    C->nbq = b_var.size();
    // length invariants
    if (L.n_ic != cs->n_inputs || L.n_h < C->m - 1 || L.n_l != cs->n_aux || L.n_a != C->na || L.n_b1 != C->nbq || L.n_b2 != C->nbq)
        return call.done(MASP_HIP_E_PARAMS_SHAPE);
    {
        // gamma_g2 and ic are the verifier's: no table is built from them, but a file whose encoding of them bellman's `Parameters::read`
        // refuses is refused here too (at most 8 + 1 points: decoded on the host).  Infinity is legal in both.
        G2Affine gamma;
        G1Affine ic;
        int st = g2_read_uncompressed(L.gamma_g2, gamma);
        for (uint32_t i = 0; i < L.n_ic; ++i) st |= g1_read_uncompressed(L.ic + 96 * (size_t)i, ic);
        if (st & (PT_BAD_FLAGS | PT_NOT_CANONICAL)) return call.done(MASP_HIP_E_PARAMS_FORMAT);
    }
    int rc;
    if ((rc = C->a_var.upload(a_var.data(), a_var.size(), s)) || (rc = C->b_var.upload(b_var.data(), b_var.size(), s))) return call.done(rc);
    // static R1CS -> device (coefficients to Montgomery form)
    DevBuf<int> d_flag;
    if ((rc = d_flag.reserve(1))) return call.done(rc);
    hipMemsetAsync(d_flag.p, 0, sizeof(int), s);
    for (int mi = 0; mi < 3; ++mi) {
        uint32_t nnz = rp[mi][cs->n_constraints];
        DevBuf<Fr> raw;
        std::vector<uint32_t> order(cs->n_constraints);
        for (uint32_t r = 0; r < cs->n_constraints; ++r) order[r] = r;
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t x, uint32_t y) { return rp[mi][x + 1] - rp[mi][x] > rp[mi][y + 1] - rp[mi][y]; });
        if ((rc = C->row_order[mi].upload(order.data(), order.size(), s))) return call.done(rc);
        C->n_long_rows[mi] = 0;
        for (uint32_t r : order) {
            if (rp[mi][r + 1] - rp[mi][r] < R1CS_LONG_ROW) break;
            ++C->n_long_rows[mi];
        }
        if ((rc = C->rowptr[mi].upload(rp[mi], cs->n_constraints + 1, s)) || (rc = C->col[mi].upload(cl[mi], nnz, s)) ||
            (rc = raw.upload((const Fr*)cf[mi], nnz, s)) || (rc = C->coef[mi].reserve(nnz)))
            return call.done(rc);
        if (nnz) launch_fr_to_mont(s, raw.p, (size_t)0, C->coef[mi].p, nnz, 1, d_flag.p);
        if (hipStreamSynchronize(s) != hipSuccess) return call.done(MASP_HIP_E_HIP);
    }
    // verifying-key points used by the prover
    if ((rc = C->vk.reserve(1))) return call.done(rc);
    {
        DevBuf<uint8_t> raw;
        if ((rc = raw.upload(params, 864, s))) return call.done(rc);
        DevBuf<int> st;
        if ((rc = st.reserve(1))) return call.done(rc);
        hipMemsetAsync(st.p, 0, sizeof(int), s);
        VkDevice* v = C->vk.p;
        launch_g1_import_one(s, raw.p + 0, &v->alpha_g1, st.p);
        launch_g1_import_one(s, raw.p + 96, &v->beta_g1, st.p);
        launch_g2_import_one(s, raw.p + 192, &v->beta_g2, st.p);
        launch_g1_import_one(s, raw.p + 576, &v->delta_g1, st.p);
        launch_g2_import_one(s, raw.p + 672, &v->delta_g2, st.p);
        int hst = 0, hflag = 0;
        if (hipMemcpyAsync(&hst, st.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(&hflag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            last_hip_error() = "vk import failed";
            return call.done(MASP_HIP_E_HIP);
        }
        if (hflag) return call.done(MASP_HIP_E_SCALAR_RANGE);
        if (hst & (PT_BAD_FLAGS | PT_NOT_CANONICAL)) return call.done(MASP_HIP_E_PARAMS_FORMAT);
        // fixed-base tables for the points every proof multiplies by r, s, rs
        DevBuf<G1Affine> p1;
        DevBuf<G2Affine> p2;
        if ((rc = p1.reserve(3)) || (rc = p2.reserve(1)) || (rc = C->fb1.reserve(3 * 32 * 255)) || (rc = C->fb2.reserve(32 * 255))) return call.done(rc);
        hipMemcpyAsync(p1.p + 0, &v->delta_g1, sizeof(G1Affine), hipMemcpyDeviceToDevice, s);
        hipMemcpyAsync(p1.p + 1, &v->alpha_g1, sizeof(G1Affine), hipMemcpyDeviceToDevice, s);
        hipMemcpyAsync(p1.p + 2, &v->beta_g1, sizeof(G1Affine), hipMemcpyDeviceToDevice, s);
        hipMemcpyAsync(p2.p, &v->delta_g2, sizeof(G2Affine), hipMemcpyDeviceToDevice, s);
        launch_fixed_table_g1(s, p1.p, C->fb1.p, 3);
        launch_fixed_table_g2(s, p2.p, C->fb2.p, 1);
        if (hipStreamSynchronize(s) != hipSuccess) {
            last_hip_error() = std::string("fixed-base tables failed: ") + hipGetErrorString(hipGetLastError());
            return call.done(MASP_HIP_E_HIP);
        }
        // delta at infinity -> bellperson's UnexpectedIdentity; alpha/beta at infinity are merely degenerate
        if ((params[576] & 0x40) || (params[672] & 0x40)) return call.done(MASP_HIP_E_UNEXPECTED_IDENTITY);
    }
    // query vectors + window tables
    // h scalars are uniform in Fr; the witness queries are mostly 0 / 1 (70 % of a Spend witness is
    // boolean-constrained), so their effective size for window selection is a fraction of their length
    const uint32_t pct = (uint32_t)ctx->opt.witness_nontrivial_percent;
    auto eff = [&](uint32_t n) { return (uint32_t)((uint64_t)n * pct / 100); };
    const int c_la = ctx->opt.window_bits_la, c_b = ctx->opt.window_bits_b;   // 0: chosen from the expected non-trivial scalars
    // b_g2 of a batch: its own width if asked for (masp_hip_options::window_bits_b2), else b_g1's — it is then reduced from b_g1's sorted
    // digit list instead of sorting for itself (enqueue_proofs: share_bq)
    const int c_b2 = ctx->opt.window_bits_b2 > 0 ? ctx->opt.window_bits_b2 : c_b;
    // h has uniform scalars: 16-bit windows from 48 k points (Spend 131 071, Convert 65 535), 15 bits below (Output 32 767)
    const uint32_t n_h = (uint32_t)(C->m - 1);
    const int c_h = ctx->opt.window_bits_h ? ctx->opt.window_bits_h : n_h >= 49152 ? 16 : n_h >= 16384 ? 15 : 0;
    // (h's own table serves lone proofs only: its window width is theirs to choose — masp_hip_options::window_bits_h_lone)
    const int c_h_lone = ctx->opt.window_bits_h_lone ? ctx->opt.window_bits_h_lone : c_h;
    // subset rows (MsmSubset, device/msm_geom.h) behind the tables whose scalars are witness values — a, b_g1, b_g2 and the l part of the merged
    // h + l —: a third of a witness is the scalar 1, and an aligned block of boolean scalars becomes one entry.  The tables that only lone
    // proofs use (h, l, b2_lone) have none.
    const int sub_bits = ctx->boolean_block_bits;
    // doubled window rows (msm_geom_twin, device/msm_geom.h) behind the tables that batches use: two thirds as many buckets.  b_g1 and b_g2
    // share a sort only with the same layout; a point at infinity in one of them (the circuit is refused below) leaves that one plain.
    const bool twin_hl = ctx->twin_rows & 1, twin_ab = ctx->twin_rows & 2;
    // (with doubled rows a / b take 13-bit windows where the width is the loader's choice: MsmBases::pick_geom)
    if ((rc = C->h.load_host(L.h, (uint32_t)(C->m - 1), s, 0xffffffffu, c_h_lone)) || (rc = C->l.load_host(L.l, L.n_l, s, eff(L.n_l), c_la)) ||
        (rc = C->a.load_host(L.a, L.n_a, s, eff(L.n_a), c_la, sub_bits, 0, 0xffffffffu, twin_ab)) ||
        (rc = C->b1.load_host(L.b_g1, L.n_b1, s, eff(L.n_b1), c_b, sub_bits, 0, 0xffffffffu, twin_ab)) ||
        (rc = C->b2.load_host(L.b_g2, L.n_b2, s, eff(L.n_b2), c_b2, sub_bits, 0, 0xffffffffu, twin_ab)))
        return call.done(rc);
    if (C->b1.sub.bits && C->b2.sub.bits && msm_same_sort(C->b1, C->b2)) {
        // b_g2 is reduced from b_g1's sorted digit list (enqueue_proofs: share_b): the two tables have the same row layout, and the sort
        // must leave alone every block that is bad in either — both bitmaps become their union
        const uint32_t words = C->b1.sub.bad_words();
        std::vector<uint32_t> w1(words), w2(words);
        if (hipMemcpyAsync(w1.data(), C->b1.sub.bad, 4 * (size_t)words, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(w2.data(), C->b2.sub.bad, 4 * (size_t)words, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return call.done(MASP_HIP_E_HIP);
        for (uint32_t i = 0; i < words; ++i) w1[i] |= w2[i];
        if (hipMemcpyAsync(C->b1.sub.bad, w1.data(), 4 * (size_t)words, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(C->b2.sub.bad, w1.data(), 4 * (size_t)words, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return call.done(MASP_HIP_E_HIP);
    }
    // plain tables of a / b_g1 for lone proofs where the batch tables were doubled (Circuit::a_lone)
    if (C->a.g.twin && (rc = C->a_lone.load_host(L.a, L.n_a, s, eff(L.n_a), c_la, sub_bits))) return call.done(rc);
    if (C->b1.g.twin && (rc = C->b1_lone.load_host(L.b_g1, L.n_b1, s, eff(L.n_b1), c_b, sub_bits))) return call.done(rc);
    {
        const int c_lone = ctx->opt.window_bits_b2_lone;  // 0 = lone proofs share the batch tables (and B1's sort)
        if (c_lone > 0 && L.n_b2 && (rc = C->b2_lone.load_host(L.b_g2, L.n_b2, s, eff(L.n_b2), c_lone))) return call.done(rc);
    }
    const int c_hl = c_h ? c_h : ctx->opt.window_bits_h_lone ? 0 : C->h.g.c;
    {
        const size_t nh = C->m - 1;
        std::vector<uint8_t> cat(96 * (nh + L.n_l));
        memcpy(cat.data(), L.h, 96 * nh);
        memcpy(cat.data() + 96 * nh, L.l, 96 * (size_t)L.n_l);
        // (subset rows over the l part only: the quotient's coefficients are uniform in Fr)
        if ((rc = C->hl.load_host(cat.data(), (uint32_t)(nh + L.n_l), s, 0xffffffffu, c_hl, sub_bits, (uint32_t)nh, 0xffffffffu, twin_hl))) return call.done(rc);
    }
    int st = C->h.import_status | C->l.import_status | C->a.import_status | C->b1.import_status | C->b2.import_status;
    if (st) return call.done(MASP_HIP_E_PARAMS_FORMAT);  // includes infinity inside a query vector, which bellman rejects
    {
        // may s*A and r*B1 use the endomorphism?  Only if everything A and B1 are sums of is in the subgroup (Circuit::g1_endo)
        DevBuf<int> out;
        if ((rc = out.reserve(1))) return call.done(rc);
        hipMemsetAsync(out.p, 0, sizeof(int), s);
        launch_g1_subgroup_flag(s, C->a.tab, sizeof(*C->a.tab), C->a.n, out.p);
        launch_g1_subgroup_flag(s, C->b1.tab, sizeof(*C->b1.tab), C->b1.n, out.p);
        launch_g1_subgroup_flag(s, &C->vk.p->alpha_g1, 0, 1, out.p);
        launch_g1_subgroup_flag(s, &C->vk.p->beta_g1, 0, 1, out.p);
        launch_g1_subgroup_flag(s, &C->vk.p->delta_g1, 0, 1, out.p);
        int outside = 1;
        if (hipMemcpyAsync(&outside, out.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
            launch_status() != MASP_HIP_OK)
            return call.done(MASP_HIP_E_HIP);
        C->g1_endo = outside == 0;
    }
    if ((rc = get_domain(ctx, C->logm, &C->dom))) return call.done(rc);
    if (ctx->quotient_form == 0) {
        // the quotient in evaluation form: the derived base set next to `hl` (which jobs with their own a / b / c keep using).  A derived
        // point at infinity — a toy CRS — is no error: the circuit silently keeps the coefficient form.
        masp::EvalBases E;
        if ((rc = build_eval_bases(ctx, *C->dom, L.h, L.l, cs, E))) return call.done(rc);
        if (E.usable) {
            const masp::EvalLayout& lay = E.lay;
            // (subset rows over the aux part only: the coset evaluations are as uniform in Fr as the coefficients were)
            if ((rc = C->hl_eval.load_device(E.d_raw.p, (uint32_t)lay.n(), s, 0xffffffffu, c_hl, sub_bits, (uint32_t)lay.aux_off(), (uint32_t)lay.in_off(), twin_hl)))
                return call.done(rc);
            if ((rc = C->eval_in_var.upload(lay.used_inputs.data(), lay.used_inputs.size(), s))) return call.done(rc);
            if (hipStreamSynchronize(s) != hipSuccess) return call.done(MASP_HIP_E_HIP);
            C->eval_inputs = lay.used_inputs;
            C->n_eval_in = (uint32_t)lay.used_inputs.size();
            if (C->hl_eval.import_status) {   // (cannot happen for points this library wrote; never prove on a table that failed its import)
                C->hl_eval.release();
                C->hl_eval.n = 0;
                C->eval_inputs.clear();
                C->n_eval_in = 0;
            }
        }
    }
    {
        // What a witness can put into a digit list (MsmBases::ent_bound): the scratch of the bucket tree is cut for it, not for n x W
        // entries.  Quotient values, coset evaluations and inputs count as full width; of the witness values, those the R1CS proves
        // boolean cost one entry, and of the others tree_entry_share in a hundred are taken to be full width.
        std::vector<uint8_t> is_bool(nv);
        r1cs_boolean_variables(cs, is_bool.data());
        const int share = ctx->tree_entry_share;
        auto count = [&](const uint32_t* vars, size_t k) {
            uint32_t nbool = 0;
            for (size_t i = 0; i < k; ++i) nbool += is_bool[vars ? vars[i] : cs->n_inputs + i];
            return nbool;
        };
        const uint32_t aux_bool = count(nullptr, cs->n_aux);
        auto bound = [&](auto& B, uint32_t n_wit, uint32_t n_bool) {
            if (B.n) B.ent_bound = tree_entry_bound(B.n, B.g.c, n_wit, n_bool, share);
        };
        bound(C->hl, cs->n_aux, aux_bool);
        bound(C->hl_eval, cs->n_aux, aux_bool);
        bound(C->a, (uint32_t)a_var.size(), count(a_var.data(), a_var.size()));
        bound(C->b1, (uint32_t)b_var.size(), count(b_var.data(), b_var.size()));
        bound(C->b2, (uint32_t)b_var.size(), count(b_var.data(), b_var.size()));
    }
    if ((rc = call.done(MASP_HIP_OK)) == MASP_HIP_OK) ctx->circ[slot] = std::move(C);   // (never a circuit behind a launch that was refused)
    return rc;
}

int masp_hip_circuit_flags(const masp_hip_ctx* ctx, uint32_t slot, uint32_t* flags) {
    if (!ctx || !flags) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return masp_hip_circuit_flags(ctx->children[0], slot, flags);
    std::shared_lock<std::shared_mutex> lock(const_cast<masp_hip_ctx*>(ctx)->mu);
    if (slot >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[slot]) return MASP_HIP_E_NOT_LOADED;
    *flags = ctx->circ[slot]->g1_endo ? MASP_HIP_CIRCUIT_G1_ENDOMORPHISM : 0u;
    return MASP_HIP_OK;
}

int masp_hip_circuit_quotient_form(const masp_hip_ctx* ctx, uint32_t slot, int32_t* form) {
    if (!ctx || !form) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return masp_hip_circuit_quotient_form(ctx->children[0], slot, form);
    std::shared_lock<std::shared_mutex> lock(const_cast<masp_hip_ctx*>(ctx)->mu);
    if (slot >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[slot]) return MASP_HIP_E_NOT_LOADED;
    *form = ctx->circ[slot]->hl_eval.n ? MASP_HIP_QUOTIENT_EVALUATION : MASP_HIP_QUOTIENT_COEFFICIENT;
    return MASP_HIP_OK;
}
int masp_hip_circuit_window_row_multiples(const masp_hip_ctx* ctx, uint32_t slot, int32_t* sets) {
    if (!ctx || !sets) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return masp_hip_circuit_window_row_multiples(ctx->children[0], slot, sets);
    std::shared_lock<std::shared_mutex> lock(const_cast<masp_hip_ctx*>(ctx)->mu);
    if (slot >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[slot]) return MASP_HIP_E_NOT_LOADED;
    const Circuit& C = *ctx->circ[slot];
    *sets = (C.hl.g.twin ? 1 : 0) | (C.hl_eval.n && C.hl_eval.g.twin ? 2 : 0) | (C.a.g.twin ? 4 : 0) | (C.b1.g.twin ? 8 : 0) | (C.b2.g.twin ? 16 : 0);
    return MASP_HIP_OK;
}
int masp_hip_circuit_eval_bases(const masp_hip_ctx* ctx, uint32_t slot, uint8_t* bases, size_t cap_points, size_t* n_points, uint32_t* input_cols,
                                size_t cap_inputs, size_t* n_input_cols) {
    if (!ctx || !n_points || !n_input_cols) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) return masp_hip_circuit_eval_bases(ctx->children[0], slot, bases, cap_points, n_points, input_cols, cap_inputs, n_input_cols);
    std::shared_lock<std::shared_mutex> lock(const_cast<masp_hip_ctx*>(ctx)->mu);
    if (slot >= MASP_HIP_MAX_CIRCUITS || !ctx->circ[slot]) return MASP_HIP_E_NOT_LOADED;
    const Circuit& C = *ctx->circ[slot];
    *n_points = C.hl_eval.n;
    *n_input_cols = C.eval_inputs.size();
    if (!bases && !input_cols) return MASP_HIP_OK;   // (sizes only)
    if (!bases || !input_cols || cap_points < *n_points || cap_inputs < *n_input_cols) return MASP_HIP_E_CAPACITY;
    // no copy of the points is kept for this call: they are read back from the table's first n rows, which hold the points themselves
    // (k_msm_import), and encoded here
    if (C.hl_eval.n) {
        std::vector<masp::TabRow<masp::FpOps>> rows(C.hl_eval.n);
        hipSetDevice(ctx->device);
        if (hipMemcpy(rows.data(), C.hl_eval.tab, sizeof(rows[0]) * rows.size(), hipMemcpyDeviceToHost) != hipSuccess) return MASP_HIP_E_HIP;
        for (size_t i = 0; i < rows.size(); ++i) masp::g1_write_uncompressed(rows[i].p, bases + 96 * i);
    }
    memcpy(input_cols, C.eval_inputs.data(), 4 * C.eval_inputs.size());
    return MASP_HIP_OK;
}

}  // extern "C"
