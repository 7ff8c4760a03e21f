// Test-only unit over the MSM's stages: the counting sort (k_msm_sort.hip), the batch-affine bucket tree (msm_tree_impl.hpp) and the bucket
// tails (msm_impl.hpp), each run on its own through the product's own drivers — msm_sort_enqueue, MsmBases::load_device, msm_tree_enqueue,
// msm_launch_accumulate, msm_launch_accumulate_pts, msm_tails_enqueue — so that tests/test_gpu_msm_*_stages.py can look at what lies between
// them.  No kernel is copied and no launch geometry restated here; where msm_reduce_enqueue (msm_impl.hpp) prepares something in front of
// a launch, the same is done here and the mirrored lines are named.
// Built once per curve (tests/msm_stages_shim.py): without MST_G2 the sort and G1, with it G2.
// Everything that crosses this boundary is plain integers (entry words, offsets, counts) and canonical bytes: scalars 32 bytes little-endian,
// points in the bellman uncompressed wire format (96 / 192 bytes, the identity 0x40 then zeros).  Never Montgomery limbs.
// Before a stage runs, every buffer it writes or uses as scratch is filled with the byte 0xA5 (above p and r as limbs, huge as a count or an
// offset, no row as an entry); only what the product's drivers themselves clear is cleared.  The sort buffers, the workspace and the tree's
// arena live as long as the library, as they do in the product: a call finds what the call before it left.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_TAILS_QUAD_UNIT  // (this unit instantiates the lone forms of msm_tails_enqueue itself)
#define MASP_TAILS_OCT_UNIT
#include "../../masp_amd/csrc/msm_impl.hpp"
#include "../../masp_amd/csrc/msm_acc_impl.hpp"
#include "../../masp_amd/csrc/msm_tree_impl.hpp"
#ifndef MST_G2
#include "../../masp_amd/csrc/k_msm_sort.hip"
#endif

using namespace masp;

namespace {

constexpr int POISON = 0xA5;

#ifdef MST_G2
typedef Fp2Ops CurveOps;
constexpr int WIRE = 192;
typedef Fp2PairOps BatchTails;
typedef Fp2OctOps LoneTails;
void write_unc(const G2Affine& p, uint8_t* out) { g2_write_uncompressed(p, out); }
#else
typedef FpOps CurveOps;
constexpr int WIRE = 96;
typedef FpOps BatchTails;
typedef FpQuadOps LoneTails;
void write_unc(const G1Affine& p, uint8_t* out) { g1_write_uncompressed(p, out); }
#endif
typedef CurveOps O;
typedef typename O::T F;
static_assert(std::is_same<BatchTails, typename TailLaneOps<O>::type>::value, "the batch form msm_reduce_enqueue takes");

// one stream for the life of the library; a call synchronises it exactly once, in finish()
hipStream_t stream() {
    static hipStream_t s = nullptr;
    if (!s && hipStreamCreate(&s) != hipSuccess) s = nullptr;
    return s;
}
int finish(hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return -3;
    if (launch_status() != MASP_HIP_OK || hipGetLastError() != hipSuccess) return -4;
    return 0;
}
#define MST_TRY(expr)                      \
    do {                                   \
        if ((expr) != hipSuccess) return -2; \
    } while (0)

// buffers of one call that are not the product's
struct Scope {
    std::vector<void*> bufs;
    ~Scope() {
        for (void* p : bufs) (void)hipFree(p);
    }
    template <class T>
    T* alloc(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return (T*)p;
    }
};

// the product's objects (never destroyed: the runtime may be gone by the time static destructors run; mst_release() frees them)
struct State {
    MsmWorkspace<O> ws;
};
State*& state() {
    static State* st = nullptr;
    if (!st) st = new State();
    return st;
}

__global__ void __launch_bounds__(64) k_mst_export(const Xyzz<O>* __restrict__ p, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<O> a = xyzz_to_affine<O>(p[i]);
#ifdef MST_G2
    g2_write_uncompressed(a, out + (size_t)WIRE * i);
#else
    g1_write_uncompressed(a, out + (size_t)WIRE * i);
#endif
}

// a hand-made digit list is checked on the host before any kernel sees it: offsets that grow and stay inside the proof's slice, runs that
// begin at multiples of 2^pad_log, entries that name a row of the table or are the padding entry
bool list_ok(const uint32_t* sorted, const uint32_t* start, uint32_t np, uint32_t nb, size_t ent_stride, uint32_t pad_log, uint64_t rows) {
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t* st = start + (size_t)p * (nb + 1);
        if (st[0] != 0 || st[nb] > ent_stride) return false;
        for (uint32_t b = 0; b < nb; ++b)
            if (st[b + 1] < st[b] || (st[b] & ((1u << pad_log) - 1u))) return false;
        for (uint32_t k = 0; k < st[nb]; ++k) {
            const uint32_t e = sorted[(size_t)p * ent_stride + k];
            if (e != MSM_PAD_ENTRY && (e & 0x7fffffffu) >= rows) return false;
        }
    }
    return true;
}

// what msm_reduce_enqueue does before its first launch: the workspace for this shape, n_heavy cleared, the LDS of the block reduction raised
// (msm_impl.hpp, "int rc = ws.reserve(n, g, np)" .. "HIP_TRY(hipMemsetAsync(ws.n_heavy, 0, 4 * np, s))") — and, not in the product, the poison
int prepare_workspace(hipStream_t s, MsmWorkspace<O>& ws, uint32_t n, const MsmGeom& g, uint32_t np) {
    if (ws.reserve(n, g, np)) return -5;
    if (hipFuncSetAttribute((const void*)k_xyzz_reduce_block<O>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(Xyzz<O>)) != hipSuccess) return -5;
    // the allocations of MsmWorkspace::reserve, by its capacities
    const size_t P = ws.cap_np, chunks = (ws.cap_nb + (1u << MsmWorkspace<O>::CS_LOG) - 1) >> MsmWorkspace<O>::CS_LOG, X = sizeof(Xyzz<O>);
    MST_TRY(hipMemsetAsync(ws.heavy, POISON, P * 4 * ws.cap_nb, s));
    MST_TRY(hipMemsetAsync(ws.part, POISON, X * ws.cap_part, s));
    MST_TRY(hipMemsetAsync(ws.bkt, POISON, P * X * ws.cap_nb, s));
    Xyzz<O>* small[] = {ws.S[0], ws.S[1], ws.T, ws.R[0], ws.R[1]};
    for (Xyzz<O>* b : small) MST_TRY(hipMemsetAsync(b, POISON, P * X * chunks, s));
    MST_TRY(hipMemsetAsync(ws.tsum, POISON, P * X * 32, s));
    MST_TRY(hipMemsetAsync(ws.startT, POISON, P * 4 * (ws.cap_nb + 1), s));
    MST_TRY(hipMemsetAsync(ws.hparts, POISON, std::min<size_t>(P, 7) * X * MSM_HEAVY_SLOTS, s));
    MST_TRY(hipMemsetAsync(ws.n_heavy, POISON, 4 * P, s));
    MST_TRY(hipMemsetAsync(ws.n_heavy, 0, 4 * np, s));  // as msm_reduce_enqueue clears it: the proofs of this launch, no more
    return 0;
}

// bkt (np x nb) and the results (np) as wire bytes
int export_points(hipStream_t s, Scope& sc, const Xyzz<O>* d, uint32_t n, uint8_t* out) {
    uint8_t* d_out = sc.alloc<uint8_t>((size_t)WIRE * n);
    if (!d_out) return -2;
    MASP_LAUNCH(k_mst_export, dim3((n + 63) / 64), dim3(64), 0, s, d, n, d_out);
    MST_TRY(hipMemcpyAsync(out, d_out, (size_t)WIRE * n, hipMemcpyDeviceToHost, s));
    return 0;
}

}  // namespace

#ifdef MST_G2
#define MST_NAME(f) mst_g2_##f
#else
#define MST_NAME(f) mst_g1_##f
#endif

extern "C" {

#ifndef MST_G2
// ---- the sort (curve-independent) -----------------------------------------------------------------------------------------------------
uint64_t mst_padded_entries(uint32_t n, int c, uint32_t pad_log) { return MsmSortBuf::padded_entries(n, msm_geom(c), pad_log); }
uint32_t mst_ranges_for(uint32_t n, uint32_t np) { return MsmSortBuf::ranges_for(n, np); }

static MsmSortBuf*& sort_buf() {
    static MsmSortBuf* sb = nullptr;
    if (!sb) sb = new MsmSortBuf();
    return sb;
}
void mst_sort_release() {
    delete sort_buf();
    sort_buf() = nullptr;
}
// scalars: np x n x 32 bytes.  sub_bits 0: no subset rows; else blocks [b_first, b_end) and their bad-block bitmap, uploaded here.
// poison: fill every buffer of the MsmSortBuf first (0: leave what the sort before this one left).
// -> start, dense: np x (nb + 1); sorted: np x mst_padded_entries(n, c, pad_log) words
int mst_sort(const uint8_t* scalars, uint32_t n, int c, uint32_t np, uint32_t pad_log, uint32_t sub_bits, uint32_t b_first, uint32_t b_end,
             const uint32_t* bad_words, int poison, uint32_t* start, uint32_t* dense, uint32_t* sorted) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0 || np == 0) return -1;
    const MsmGeom g = msm_geom(c);
    MsmSortBuf& sb = *sort_buf();
    Scope sc;
    uint32_t* d_scalars = sc.alloc<uint32_t>((size_t)np * n * 8);
    if (!d_scalars) return -2;
    MST_TRY(hipMemcpyAsync(d_scalars, scalars, (size_t)np * n * 32, hipMemcpyHostToDevice, s));
    MsmSubset sub;
    if (sub_bits) {
        sub.bits = sub_bits;
        sub.b_first = b_first;
        sub.b_end = b_end;
        sub.row0 = n * (uint32_t)g.W;
        sub.bad = sc.alloc<uint32_t>(sub.bad_words());
        if (!sub.bad) return -2;
        MST_TRY(hipMemcpyAsync(sub.bad, bad_words, 4 * (size_t)sub.bad_words(), hipMemcpyHostToDevice, s));
    }
    // the reservation msm_sort_enqueue will make (k_msm_sort.hip: "sb.reserve(n, g, np, pad_log, rows)"), so that its own keeps the allocation
    const uint64_t rows = (uint64_t)n * (uint32_t)g.W + sub.rows();
    if (sb.reserve(n, g, np, pad_log, rows)) return -5;
    if (poison) {
        const size_t ent = std::max<size_t>(sb.cap_ent, 1);
        MST_TRY(hipMemsetAsync(sb.sorted, POISON, sb.cap_np * 4 * ent, s));
        MST_TRY(hipMemsetAsync(sb.tmp, POISON, sb.cap_np * 4 * ent, s));
        if (sb.has_tmpf) MST_TRY(hipMemsetAsync(sb.tmpf, POISON, sb.cap_np * ent, s));
        MST_TRY(hipMemsetAsync(sb.hist_wg, POISON, 4 * sb.cap_hist, s));
        MST_TRY(hipMemsetAsync(sb.crel, POISON, 4 * sb.cap_crel, s));
        MST_TRY(hipMemsetAsync(sb.dense, POISON, sb.cap_np * 4 * (sb.cap_nb + 1), s));
        MST_TRY(hipMemsetAsync(sb.start, POISON, sb.cap_np * 4 * (sb.cap_nb + 1), s));
        MST_TRY(hipMemsetAsync(sb.btot, POISON, sb.cap_np * sizeof(uint2) * ((sb.cap_nb + 1023) / 1024), s));
    }
    const uint32_t* const sorted_before = sb.sorted;
    if (msm_sort_enqueue(s, n, g, sb, d_scalars, (size_t)n * 8, np, pad_log, sub)) return -6;
    if (sb.sorted != sorted_before) return -7;  // the driver's own reserve must have kept the poisoned allocation
    const size_t words = (size_t)g.nb + 1;
    MST_TRY(hipMemcpyAsync(start, sb.start, 4 * words * np, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(dense, sb.dense, 4 * words * np, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(sorted, sb.sorted, 4 * sb.ent_stride * np, hipMemcpyDeviceToHost, s));
    return finish(s);
}
#endif  // !MST_G2

void MST_NAME(release)() {
    delete state();
    state() = nullptr;
}

// lanes per proof of the tree's passes at level L, and the entries per proof its views hold, as msm_tree_enqueue computes them
uint32_t MST_NAME(tree_lanes)(uint32_t n, int c, uint32_t pad_log, uint64_t ent_bound, uint32_t L) {
    MsmBases<O, WIRE> B;
    B.n = n;
    B.g = msm_geom(c);
    B.ent_bound = ent_bound;
    const uint64_t E_ub = std::min<uint64_t>(MsmSortBuf::padded_entries(n, B.g, pad_log), B.tree_entries(pad_log));
    return tree_lanes(E_ub, (uint32_t)B.g.nb, L);
}
uint64_t MST_NAME(tree_entries)(uint32_t n, int c, uint32_t pad_log, uint64_t ent_bound) {
    MsmBases<O, WIRE> B;
    B.n = n;
    B.g = msm_geom(c);
    B.ent_bound = ent_bound;
    return B.tree_entries(pad_log);
}

// ---- the tree: T levels over a hand-made digit list, then the accumulation of level T's points and the tails ------------------------
// bases: n wire points; sorted: np x padded_entries(n, c, pad_log) words, start: np x (nb + 1), as the sort would leave them.
// ent_bound: MsmBases::ent_bound (0: the worst case, no proof can be over it).
// -> D, Q: (T + 1) x np x (nb + 1); keep, over_start: np x (nb + 1); over_count: the counter before and after;
//    pts: np x pts_stride points of level T in wire bytes (at most pts_cap per proof are written; *pts_stride is what the tree used); result: np points
int MST_NAME(tree)(const uint8_t* bases, uint32_t n, int c, const uint32_t* sorted, const uint32_t* start, uint32_t np, uint32_t pad_log, uint32_t T,
                   uint64_t ent_bound, uint32_t* D, uint32_t* Q, uint32_t* keep, uint32_t* over_start, uint32_t* over_count, uint8_t* pts, uint64_t pts_cap,
                   uint64_t* pts_stride, uint8_t* result) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0 || np == 0 || T == 0) return -1;
    MsmBases<O, WIRE> B;
    if (B.load_host(bases, n, s, n, c)) return -5;
    B.ent_bound = ent_bound;
    const MsmGeom g = B.g;
    const uint32_t nb = (uint32_t)g.nb;
    // the MsmSortBuf a sort of this shape would have left, its digit list made by hand
    MsmSortBuf sb;
    if (sb.reserve(n, g, np, pad_log)) return -5;
    sb.n = n;
    sb.np = np;
    sb.g = g;
    sb.pad_log = pad_log;
    sb.ent_stride = MsmSortBuf::padded_entries(n, g, pad_log);
    if (!list_ok(sorted, start, np, nb, sb.ent_stride, pad_log, B.rows())) return -10;
    MST_TRY(hipMemcpyAsync(sb.sorted, sorted, 4 * sb.ent_stride * np, hipMemcpyHostToDevice, s));
    MST_TRY(hipMemcpyAsync(sb.start, start, 4 * (size_t)(nb + 1) * np, hipMemcpyHostToDevice, s));
    MsmWorkspace<O>& ws = state()->ws;
    if (int rc = prepare_workspace(s, ws, n, g, np)) return rc;
    const uint32_t nchunks = ws.nchunks_for(n, g, np);  // msm_reduce_enqueue: "const uint32_t nchunks = ws.nchunks_for(n, g, np)"
    // msm_reduce_enqueue: "const bool bounded = sb.ent_stride > B.tree_entries(sb.pad_log); if (bounded && (rc = ws.reserve_tree_over(s)))" — the
    // counter is reserved in any case here, so that a proof wrongly taken for one over the bound shows in it
    if (ws.reserve_tree_over(s)) return -5;
    const bool bounded = sb.ent_stride > B.tree_entries(sb.pad_log);
    MST_TRY(hipMemcpyAsync(&over_count[0], ws.d_tree_over, 4, hipMemcpyDeviceToHost, s));
    // the arena with the arguments msm_tree_enqueue will use ("E_ub = min(sb.ent_stride, B.tree_entries(sb.pad_log)); tw.reserve(E_ub, nb, q, T)")
    MsmTreeWs<O>& tw = ws.tree;
    const uint64_t E_ub = std::min<uint64_t>(sb.ent_stride, B.tree_entries(sb.pad_log));
    if (tw.reserve(E_ub, nb, np, T)) return -5;
    const uint8_t* const arena_before = tw.arena->p;
    MST_TRY(hipMemsetAsync(tw.arena->p, POISON, tw.arena->cap, s));
    if (msm_tree_enqueue<O, WIRE>(s, B, sb, tw, 0, np, T, ws.startT, ws.d_tree_over)) return -6;
    if (tw.arena->p != arena_before) return -7;
    const size_t plan = (size_t)(T + 1) * np * (nb + 1), row = (size_t)np * (nb + 1), stride = tw.point_stride();
    *pts_stride = stride;
    MST_TRY(hipMemcpyAsync(D, tw.D, 4 * plan, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(Q, tw.Q, 4 * plan, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(keep, ws.startT, 4 * row, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(over_start, tw.over_start, 4 * row, hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(&over_count[1], ws.d_tree_over, 4, hipMemcpyDeviceToHost, s));
    std::vector<F> hx(stride * np), hy(stride * np);
    MST_TRY(hipMemcpyAsync(hx.data(), tw.points_x(), sizeof(F) * hx.size(), hipMemcpyDeviceToHost, s));
    MST_TRY(hipMemcpyAsync(hy.data(), tw.points_y(), sizeof(F) * hy.size(), hipMemcpyDeviceToHost, s));
    // msm_reduce_enqueue: "msm_launch_accumulate_pts<O>(s, ws.tree.points_x(), ..., ws.tree.plan_D(tree_T), nb, nchunks, ws.part + ..., q)", then
    // "if (bounded) msm_launch_accumulate<O>(s, B.tab, sb.sorted + ..., sb.ent_stride, ws.tree.over_start, nb, nchunks, ws.part + ..., q)", "start = ws.startT"
    msm_launch_accumulate_pts<O>(s, tw.points_x(), tw.points_y(), stride, tw.plan_D(T), nb, nchunks, ws.part, np);
    if (bounded) msm_launch_accumulate<O>(s, B.tab, sb.sorted, sb.ent_stride, tw.over_start, nb, nchunks, ws.part, np);
    Scope sc;
    Xyzz<O>* d_res = sc.alloc<Xyzz<O>>(np);
    if (!d_res) return -2;
    MST_TRY(hipMemsetAsync(d_res, POISON, sizeof(Xyzz<O>) * np, s));
    // a tree runs in batches only (msm_tree_levels): the batch form of the tails
    msm_tails_enqueue<O, BatchTails>(s, ws, ws.startT, nb, nchunks, np, false, d_res, 1);
    if (int rc = export_points(s, sc, d_res, np, result)) return rc;
    if (int rc = finish(s)) return rc;
    const size_t take = std::min<size_t>(stride, pts_cap);
    for (uint32_t p = 0; p < np; ++p)
        for (size_t i = 0; i < take; ++i) {
            const Affine<O> a{hx[p * stride + i], hy[p * stride + i]};
            write_unc(a, pts + ((size_t)p * pts_cap + i) * WIRE);
        }
    return 0;
}

// ---- the accumulation over a hand-made digit list with an nchunks of the caller's, then the tails ------------------------------------
// sorted: np x ent_stride words, start: np x (nb + 1) (packed runs: pad_log 0).  lone: the forms msm_reduce_enqueue takes for np < 8 (FpQuadOps /
// Fp2OctOps, heavy span 12, shared heavy buckets) or for a batch (FpOps / Fp2PairOps, k_msm_bucket_gather_split, span 8).
// -> bkt: np x nb points, result: np points, n_heavy: np counts
int MST_NAME(tails)(const uint8_t* bases, uint32_t n, int c, const uint32_t* sorted, const uint32_t* start, uint32_t np, uint64_t ent_stride,
                    uint32_t nchunks, int lone, uint8_t* bkt, uint8_t* result, uint32_t* n_heavy) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0 || np == 0 || nchunks == 0) return -1;
    MsmBases<O, WIRE> B;
    if (B.load_host(bases, n, s, n, c)) return -5;
    const MsmGeom g = B.g;
    const uint32_t nb = (uint32_t)g.nb;
    if (!list_ok(sorted, start, np, nb, ent_stride, 0, B.rows())) return -10;
    MsmWorkspace<O>& ws = state()->ws;
    if (int rc = prepare_workspace(s, ws, n, g, np)) return rc;
    // `part` is addressed with np x (nchunks + nb) (MsmWorkspace::reserve): the caller's nchunks must fit what reserve allocated
    if ((size_t)np * ((size_t)nchunks + nb) > ws.cap_part) return -11;
    Scope sc;
    uint32_t* d_sorted = sc.alloc<uint32_t>((size_t)np * ent_stride);
    uint32_t* d_start = sc.alloc<uint32_t>((size_t)np * (nb + 1));
    Xyzz<O>* d_res = sc.alloc<Xyzz<O>>(np);
    if (!d_sorted || !d_start || !d_res) return -2;
    MST_TRY(hipMemcpyAsync(d_sorted, sorted, 4 * (size_t)np * ent_stride, hipMemcpyHostToDevice, s));
    MST_TRY(hipMemcpyAsync(d_start, start, 4 * (size_t)np * (nb + 1), hipMemcpyHostToDevice, s));
    MST_TRY(hipMemsetAsync(d_res, POISON, sizeof(Xyzz<O>) * np, s));
    // msm_reduce_enqueue without a tree: "msm_launch_accumulate<O>(s, B.tab, sb.sorted, sb.ent_stride, sb.start, nb, nchunks, ws.part, np)", then the
    // tails in the form it picks by `lone`
    msm_launch_accumulate<O>(s, B.tab, d_sorted, ent_stride, d_start, nb, nchunks, ws.part, np);
    if (lone)
        msm_tails_enqueue<O, LoneTails>(s, ws, d_start, nb, nchunks, np, true, d_res, 1);
    else
        msm_tails_enqueue<O, BatchTails>(s, ws, d_start, nb, nchunks, np, false, d_res, 1);
    if (int rc = export_points(s, sc, ws.bkt, np * nb, bkt)) return rc;
    if (int rc = export_points(s, sc, d_res, np, result)) return rc;
    MST_TRY(hipMemcpyAsync(n_heavy, ws.n_heavy, 4 * np, hipMemcpyDeviceToHost, s));
    return finish(s);
}

}  // extern "C"
