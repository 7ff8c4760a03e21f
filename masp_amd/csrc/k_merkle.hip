// Frozen commitment trees on the GPU: the C ABI entry point masp_hip_merkle_tree_complete (include/masp_hip.h),
// FrozenCommitmentTree::complete, root and path of masp_primitives/src/merkle_tree.rs:177-251 over a row of nodes.  A tree over n leaves is
// n - 1 independent Pedersen hashes in ceil(log2 n) rows and 32 - ceil(log2 n) single hashes against empty_root above them.
//
//           k_mt_check      one lane per input node: canonical below the BLS12-381 scalar modulus, or the smallest offender's index through an
//                           atomic minimum; every later kernel leaves at once when there is one.
//           k_mt_level      one lane per parent of a row: two 32-byte children, or empty_root(level) for the padded right child of an odd row
//                           (which the lane also writes into the node vector), the Merkle hash (device/merkle.hpp) from the Niels table the
//                           compact scan uses, the parent's 32 canonical bytes into the next row's place.  One launch per row, on one stream.
//           k_mt_top        rows of at most MT_TOP_PARENTS parents: one wave loops over the remaining levels up to 32 in one launch.
//           k_mt_paths      one lane per (position, level): the sibling out of the node vector.
// masp_hip_merkle_tree_append hashes a block of leaves at an arbitrary offset of the depth-32 tree instead: the complete nodes whose last
// leaf lies in the block, which is all that a CommitmentTree and its IncrementalWitnesses need to advance by that block.
//           k_mt_append_level  one lane per parent of a level of the block; the first parent's left child is the old frontier's node of
//                              that level where the block starts at an odd index there.  No padding: an unpaired last node has no parent.
//           k_mt_append_top    at most MT_TOP_PARENTS parents: one wave loops up to level 32, the carry chain against the frontier included.
// Why the table is read from global memory, the inversion is one per lane and the hand-over is at one wave: KERNELS.md.
#include <mutex>

#include "device/merkle.hpp"
#include "internal.h"
#include "pedersen_table.h"

using namespace masp;

namespace {

constexpr uint32_t MT_BLOCK = 256;         // k_mt_check, k_mt_level, k_mt_paths: lanes per workgroup
constexpr uint32_t MT_TOP_PARENTS = 64;    // a row of at most this many parents goes to k_mt_top
constexpr uint32_t MT_NO_BAD = 0xffffffffu;
constexpr size_t MT_MAX_ROW = (size_t)1 << 22;

__global__ __launch_bounds__(MT_BLOCK) void k_mt_check(const uint32_t* __restrict__ row, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4 a = ((const uint4*)row)[2 * (size_t)i], b = ((const uint4*)row)[2 * (size_t)i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (!fr_is_canonical(w)) atomicMin(bad, i);
}

// parent j of the row of `width` nodes (before padding) that starts at node `start`; 2 j < width
__device__ __forceinline__ void mt_parent(uint32_t* nodes, const uint32_t* __restrict__ empties, const JNiels* __restrict__ table, uint64_t start,
                                          uint32_t width, uint32_t level, uint32_t j) {
    uint4* row = (uint4*)nodes + 2 * start;
    const bool pad = 2 * j + 1 >= width;   // the last parent of an odd row: its right child is the row's padding
    const uint4 a = row[4 * (size_t)j], b = row[4 * (size_t)j + 1];
    const uint4* rp = pad ? (const uint4*)empties + 2 * level : row + 4 * (size_t)j + 2;
    const uint4 c = rp[0], d = rp[1];
    if (pad) {
        row[4 * (size_t)j + 2] = c;
        row[4 * (size_t)j + 3] = d;
    }
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, r[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    uint32_t out[8];
    merkle_combine(out, table, level, l, r);
    uint4* dst = row + 2 * ((size_t)width + (width & 1u) + j);
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_level(uint32_t* nodes, const uint32_t* __restrict__ empties, const JNiels* __restrict__ table,
                                                       const uint32_t* __restrict__ bad, uint64_t start, uint32_t width, uint32_t level) {
    const uint32_t j = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (j >= (width + 1) / 2 || *bad != MT_NO_BAD) return;
    mt_parent(nodes, empties, table, start, width, level, j);
}

// one workgroup of one wave; width <= 2 MT_TOP_PARENTS.  A level's parents are the next level's children: a barrier between them.
__global__ __launch_bounds__(MT_TOP_PARENTS) void k_mt_top(uint32_t* nodes, const uint32_t* __restrict__ empties, const JNiels* __restrict__ table,
                                                           const uint32_t* __restrict__ bad, uint64_t start, uint32_t width, uint32_t level) {
    if (*bad != MT_NO_BAD) return;   // (the whole workgroup)
#pragma unroll 1
    for (; level < MT_DEPTH; ++level) {
        const uint32_t parents = (width + 1) / 2;
        if (threadIdx.x < parents) mt_parent(nodes, empties, table, start, width, level, threadIdx.x);
        __syncthreads();
        start += width + (width & 1u);
        width = parents;
    }
}

// paths[(p depth + i) 8 ..]: the sibling of position p's ancestor in row i, as FrozenCommitmentTree::path finds it
__global__ __launch_bounds__(MT_BLOCK) void k_mt_paths(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ empties,
                                                       const uint32_t* __restrict__ bad, uint32_t n, uint32_t height0,
                                                       const uint64_t* __restrict__ positions, uint32_t n_paths, uint32_t* __restrict__ paths) {
    const uint32_t depth = MT_DEPTH - height0;
    const uint64_t idx = (uint64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (idx >= (uint64_t)n_paths * depth || *bad != MT_NO_BAD) return;
    const uint32_t p = (uint32_t)(idx / depth), i = (uint32_t)(idx % depth);
    uint64_t start, width;
    mt_row(n, i, start, width);
    width += width & 1u;
    const uint64_t pos = positions[p], sib = (pos >> i) ^ 1u;
    if (pos >= n) return;   // (refused on the host)
    const uint4* src = sib < width ? (const uint4*)nodes + 2 * (start + sib) : (const uint4*)empties + 2 * (height0 + i);
    uint4* dst = (uint4*)paths + 2 * idx;
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---- a block appended at an arbitrary offset (masp_hip_merkle_tree_append) ----
// The buffer: frontier[0..32) | the row, leaves start .. end - 1 | level 1 | ... | level 32, level h being the nodes (h, i) for
// start >> h <= i < end >> h, the complete nodes whose last leaf is in the block.  Nothing is padded: an unpaired last node has no parent.
constexpr uint64_t MT_APPEND_ROW = MT_DEPTH;   // the row's first node in the buffer, behind the frontier

// parent t of one level: its children are nodes of `level` from nodes[src] on, the first of them node (level, c0).  c0 odd: that node is a
// RIGHT child, and its parent's left child is frontier[level], the complete subtree that ends just before the block.
__device__ __forceinline__ void mt_append_parent(uint32_t* nodes, const JNiels* __restrict__ table, uint64_t src, uint64_t dst, uint32_t odd,
                                                 uint32_t level, uint32_t t) {
    const uint4* row = (const uint4*)nodes + 2 * src;
    const size_t ri = 2 * (size_t)t + 1 - odd;   // the right child's place in the row; the left one is in front of it, or is the frontier's
    const uint4* lp = (odd && t == 0) ? (const uint4*)nodes + 2 * level : row + 2 * (ri - 1);
    const uint4 a = lp[0], b = lp[1], c = row[2 * ri], d = row[2 * ri + 1];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, r[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    uint32_t out[8];
    merkle_combine(out, table, level, l, r);
    uint4* o = (uint4*)nodes + 2 * (dst + t);
    o[0] = make_uint4(out[0], out[1], out[2], out[3]);
    o[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_append_level(uint32_t* nodes, const JNiels* __restrict__ table, const uint32_t* __restrict__ bad,
                                                              uint64_t src, uint64_t dst, uint32_t parents, uint32_t odd, uint32_t level) {
    const uint32_t t = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (t >= parents || *bad != MT_NO_BAD) return;
    mt_append_parent(nodes, table, src, dst, odd, level, t);
}

// one workgroup of one wave, from a level of at most MT_TOP_PARENTS parents up to level 32: above log2(n) a level has at most one parent,
// the carry chain against the frontier.  Every lane sees the same start, end and level: the loop and its barrier are uniform.
__global__ __launch_bounds__(MT_TOP_PARENTS) void k_mt_append_top(uint32_t* nodes, const JNiels* __restrict__ table,
                                                                  const uint32_t* __restrict__ bad, uint64_t start, uint64_t end, uint64_t src,
                                                                  uint32_t level) {
    if (*bad != MT_NO_BAD) return;   // (the whole workgroup)
#pragma unroll 1
    for (; level < MT_DEPTH; ++level) {
        const uint64_t c0 = start >> level, c1 = end >> level;
        const uint32_t width = (uint32_t)(c1 - c0), parents = (uint32_t)((c1 >> 1) - (c0 >> 1));
        if (parents == 0) break;   // (and none above)
        if (threadIdx.x < parents) mt_append_parent(nodes, table, src, src + width, (uint32_t)(c0 & 1u), level, threadIdx.x);
        __syncthreads();
        src += width;
    }
}

// the nodes of levels 1..32 that a block of n leaves at `start` completes
size_t mt_append_count(uint64_t start, uint64_t n) {
    size_t total = 0;
    for (uint32_t h = 1; h <= MT_DEPTH; ++h) total += (size_t)(((start + n) >> h) - (start >> h));
    return total;
}

// everything of one tree on the context's first verifier stream; the caller is a WalletCall
int run_tree(masp_hip_ctx* ctx, unsigned height0, size_t n, size_t total, const uint8_t* row, uint8_t* nodes_out, uint8_t root32[32],
             size_t n_paths, const uint64_t* positions, uint8_t* paths_out, int64_t* bad_index) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const uint32_t depth = MT_DEPTH - height0;
    const auto& empty = masp_host::merkle_empty_roots();
    int rc;
    if ((rc = w.mt_nodes.reserve(8 * total)) || (rc = w.mt_bad.reserve(1)) || (rc = w.mt_pos.reserve(n_paths)) ||
        (rc = w.mt_paths.reserve(8 * n_paths * depth)))
        return rc;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    if ((rc = pedersen_table_ensure(w, s)) || (rc = w.mt_empties.ensure((const uint32_t*)empty[0].data(), 8 * (MT_DEPTH + 1), s))) return rc;
    HIP_TRY(hipMemcpyAsync(w.mt_nodes.p, row, 32 * n, hipMemcpyHostToDevice, s));
    if (n_paths) HIP_TRY(hipMemcpyAsync(w.mt_pos.p, positions, 8 * n_paths, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.mt_bad.p, 0xff, sizeof(uint32_t), s));
    HIP_TRY(hipEventRecord(ev[1], s));
    uint32_t* nodes = w.mt_nodes.p;
    const uint32_t *empties = w.mt_empties.p, *bad = w.mt_bad.p;
    const JNiels* table = (const JNiels*)w.nsc_table.p;
    MASP_LAUNCH(k_mt_check, dim3((uint32_t)((n + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0, s, (const uint32_t*)nodes, (uint32_t)n,
                w.mt_bad.p);
    uint64_t start = 0;
    uint32_t width = (uint32_t)n, level = height0;
    for (; level < MT_DEPTH && (width + 1) / 2 > MT_TOP_PARENTS; ++level) {
        const uint32_t parents = (width + 1) / 2;
        MASP_LAUNCH(k_mt_level, dim3((parents + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, s, nodes, empties, table, bad, start, width, level);
        start += width + (width & 1u);
        width = parents;
    }
    if (level < MT_DEPTH) MASP_LAUNCH(k_mt_top, dim3(1), dim3(MT_TOP_PARENTS), 0, s, nodes, empties, table, bad, start, width, level);
    if (n_paths && depth)
        MASP_LAUNCH(k_mt_paths, dim3((uint32_t)((n_paths * depth + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0, s, (const uint32_t*)nodes, empties,
                    bad, (uint32_t)n, height0, (const uint64_t*)w.mt_pos.p, (uint32_t)n_paths, w.mt_paths.p);
    HIP_TRY(hipEventRecord(ev[2], s));
    uint32_t h_bad = MT_NO_BAD;
    uint8_t h_root[32];
    HIP_TRY(hipMemcpyAsync(&h_bad, w.mt_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_root, nodes + 8 * (total - 1), 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
    if (h_bad != MT_NO_BAD) {
        if (h_bad >= n) {
            last_hip_error() = "commitment tree: an index beyond the row";
            return MASP_HIP_E_HIP;
        }
        if (bad_index) *bad_index = (int64_t)h_bad;
        return MASP_HIP_E_INVALID_ARG;   // nothing written
    }
    if (nodes_out) HIP_TRY(hipMemcpyAsync(nodes_out, nodes, 32 * total, hipMemcpyDeviceToHost, s));
    if (n_paths && depth) HIP_TRY(hipMemcpyAsync(paths_out, w.mt_paths.p, 32 * n_paths * depth, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(root32, h_root, 32);
    double ms[3] = {0, 0, 0};   // (the download with the wait for the kernels' end when the host was ahead of them: stream time)
    if ((rc = add_elapsed(ev, 3, ms))) return rc;
    w.mt_timing.store(ms);
    return MASP_HIP_OK;
}

// a block of n >= 1 leaves at `start`, on the same stream and in the same scratch as run_tree; the caller is a WalletCall
int run_append(masp_hip_ctx* ctx, uint64_t start, const uint8_t* frontier, size_t n, size_t total, const uint8_t* row, uint8_t* nodes_out,
               int64_t* bad_index) {
    WalletState& w = ctx->wallet;
    hipStream_t s = ctx->streams.vk[0];
    const uint64_t end = start + n;
    int rc;
    if ((rc = w.mt_nodes.reserve(8 * (MT_APPEND_ROW + n + total))) || (rc = w.mt_bad.reserve(1))) return rc;
    Event ev[4];
    if ((rc = create_events(ev))) return rc;
    HIP_TRY(hipEventRecord(ev[0], s));
    if ((rc = pedersen_table_ensure(w, s))) return rc;
    uint32_t* nodes = w.mt_nodes.p;
    HIP_TRY(hipMemcpyAsync(nodes, frontier, 32 * MT_DEPTH, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(nodes + 8 * MT_APPEND_ROW, row, 32 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(w.mt_bad.p, 0xff, sizeof(uint32_t), s));
    HIP_TRY(hipEventRecord(ev[1], s));
    const uint32_t* bad = w.mt_bad.p;
    const JNiels* table = (const JNiels*)w.nsc_table.p;
    MASP_LAUNCH(k_mt_check, dim3((uint32_t)((n + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0, s, (const uint32_t*)(nodes + 8 * MT_APPEND_ROW),
                (uint32_t)n, w.mt_bad.p);
    uint64_t src = MT_APPEND_ROW;
    uint32_t level = 0;
    for (; level < MT_DEPTH; ++level) {
        const uint64_t c0 = start >> level, c1 = end >> level;
        const uint32_t parents = (uint32_t)((c1 >> 1) - (c0 >> 1));
        if (parents <= MT_TOP_PARENTS) break;
        MASP_LAUNCH(k_mt_append_level, dim3((parents + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0, s, nodes, table, bad, src, src + (c1 - c0),
                    parents, (uint32_t)(c0 & 1u), level);
        src += c1 - c0;
    }
    if (level < MT_DEPTH && (end >> (level + 1)) > (start >> (level + 1)))
        MASP_LAUNCH(k_mt_append_top, dim3(1), dim3(MT_TOP_PARENTS), 0, s, nodes, table, bad, start, end, src, level);
    HIP_TRY(hipEventRecord(ev[2], s));
    uint32_t h_bad = MT_NO_BAD;
    HIP_TRY(hipMemcpyAsync(&h_bad, w.mt_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (launch_status() != MASP_HIP_OK) return MASP_HIP_E_HIP;   // a refused launch: the buffers mean nothing
    if (h_bad != MT_NO_BAD) {
        if (h_bad >= n) {
            last_hip_error() = "commitment tree: an index beyond the row";
            return MASP_HIP_E_HIP;
        }
        if (bad_index) *bad_index = (int64_t)h_bad;
        return MASP_HIP_E_INVALID_ARG;   // nothing written
    }
    if (total) HIP_TRY(hipMemcpyAsync(nodes_out, nodes + 8 * (MT_APPEND_ROW + n), 32 * total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    double ms[3] = {0, 0, 0};
    if ((rc = add_elapsed(ev, 3, ms))) return rc;
    w.mt_timing.store(ms);
    return MASP_HIP_OK;
}

}  // namespace

extern "C" {

int masp_hip_merkle_tree_complete(masp_hip_ctx* ctx, unsigned height0, size_t n, const uint8_t* row, uint8_t* nodes_out, size_t nodes_capacity,
                                  size_t* n_nodes, uint8_t root32[32], size_t n_paths, const uint64_t* positions, uint8_t* paths_out,
                                  int64_t* bad_index) {
    if (bad_index) *bad_index = -1;
    if (!ctx || height0 > MT_DEPTH || !root32 || (n && !row) || n > MT_MAX_ROW || n > ((uint64_t)1 << (MT_DEPTH - height0)) ||
        n_paths > MT_MAX_ROW || (n_paths && !positions) || (n_paths && height0 < MT_DEPTH && !paths_out))
        return MASP_HIP_E_INVALID_ARG;
    for (size_t p = 0; p < n_paths; ++p)
        if (positions[p] >= n) return MASP_HIP_E_INVALID_ARG;
    size_t total = 0;
    if (n) {
        uint64_t start, width;
        mt_row(n, MT_DEPTH - height0, start, width);
        total = (size_t)(start + width);   // (the last row is the one node of level 32)
    }
    if (n_nodes) *n_nodes = total;
    if (nodes_out && nodes_capacity < total) return MASP_HIP_E_CAPACITY;   // nothing written: the caller comes back with room for *n_nodes
    if (n == 0) {
        memcpy(root32, masp_host::merkle_empty_roots()[MT_DEPTH].data(), 32);
        return MASP_HIP_OK;
    }
    (void)pedersen_table_bytes();   // built outside the locks
    WalletCall call(ctx);
    const int rc = run_tree(call.ctx, height0, n, total, row, nodes_out, root32, n_paths, positions, paths_out, bad_index);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[0]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_merkle_tree_append(masp_hip_ctx* ctx, uint64_t start, const uint8_t frontier[32 * 32], size_t n, const uint8_t* row,
                                uint8_t* nodes_out, size_t nodes_capacity, size_t* n_nodes, int64_t* bad_index) {
    if (bad_index) *bad_index = -1;
    constexpr uint64_t full = (uint64_t)1 << MT_DEPTH;
    if (!ctx || start > full || n > MT_MAX_ROW || start + n > full || (n && !row) || (n && start && !frontier)) return MASP_HIP_E_INVALID_ARG;
    const size_t total = mt_append_count(start, n);
    if (n_nodes) *n_nodes = total;
    if (!nodes_out) return MASP_HIP_OK;                                   // the count alone
    if (nodes_capacity < total) return MASP_HIP_E_CAPACITY;               // nothing written: the caller comes back with room for *n_nodes
    if (n == 0) return MASP_HIP_OK;
    uint8_t no_frontier[32 * MT_DEPTH] = {0};   // start = 0 reads none of it
    if (!frontier) frontier = no_frontier;
    for (uint32_t h = 0; h < MT_DEPTH; ++h) {   // the 32 nodes of the frontier are the host's to check: bit h of start set, entry h is used
        uint32_t w[8];
        memcpy(w, frontier + 32 * h, 32);
        if (((start >> h) & 1u) && !fr_is_canonical(w)) {
            if (bad_index) *bad_index = -2 - (int64_t)h;
            return MASP_HIP_E_INVALID_ARG;
        }
    }
    (void)pedersen_table_bytes();   // built outside the locks
    WalletCall call(ctx);
    const int rc = run_append(call.ctx, start, frontier, n, total, row, nodes_out, bad_index);
    if (rc == MASP_HIP_E_HIP) (void)hipStreamSynchronize(call.ctx->streams.vk[0]);   // nothing of this call stays in flight
    return call.done(rc);
}

int masp_hip_merkle_last_timing(masp_hip_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return MASP_HIP_E_INVALID_ARG;
    FIRST_DEVICE(ctx)->wallet.mt_timing.load(ms);
    return MASP_HIP_OK;
}

}  // extern "C"
