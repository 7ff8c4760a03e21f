// Window geometry of one MSM (shared by the kernels and the host-side drivers).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace masp {

struct MsmGeom {
    int c;        // window width in bits (signed digits)
    int W;        // windows of a 256-bit scalar: ceil(256 / c) — also the number of tables of a base set (table j holds 2^(c j) P)
    int nb;       // buckets = 2^(c-1)  (|digit| in 1..2^(c-1)); twin: msm_twin_buckets(c), rounded up to whole sorting bins
    int twin;     // 1: every window has a second table of doubled rows (table W + j holds 2 * 2^(c j) P) and only the digit magnitudes
                  // of even 2-adic valuation have a bucket (msm_geom_twin below); 0: none
    __host__ __device__ int tables() const { return twin ? 2 * W : W; }
};
static inline MsmGeom msm_geom(int c) {
    MsmGeom g;
    g.c = c;
    g.W = (256 + c - 1) / c;
    g.nb = 1 << (c - 1);
    g.twin = 0;
    return g;
}
// Doubled window rows.  A digit magnitude v = 2^t o (o odd, 1 <= v <= H = 2^(c-1)) is the entry (row multiple 2^(t & 1), bucket value
// v >> (t & 1)): the bucket values are B = { 4^s o <= H }, |B| = (2 H + 1) / 3 rounded down (21 845 of 32 768 at c = 16).  B is laid out by CLASS s = t >> 1: class s holds the values
// 4^s (2 k + 1), k = 0 .. size - 1, at the bucket ids off + k — dense odd weights, so that the weighted sum of a class is
// 4^s (2 V(B_s, 0) + sum B_s).  The sizes are H / 2, H / 8, ... (powers of two; the last class is the single value 4^s = H where c - 1 is
// even), so every class starts at a multiple of four times its size and the value 1 keeps bucket id 0.
struct MsmTwinClass {
    uint32_t off, size, weight;  // first bucket id, buckets, 4^s
};
__host__ __device__ static inline uint32_t msm_twin_classes(int c) { return (uint32_t)(c - 1) / 2u + 1u; }  // the s with 4^s <= 2^(c-1)
__host__ __device__ static inline MsmTwinClass msm_twin_class(int c, uint32_t s) {
    const uint32_t H = 1u << (c - 1), sz = H >> (2u * s + 1u);
    MsmTwinClass k;
    k.off = 2u * (H - (H >> (2u * s))) / 3u;  // = H / 2 + H / 8 + ... (s terms)
    k.size = sz ? sz : 1u;
    k.weight = 1u << (2u * s);
    return k;
}
__host__ __device__ static inline uint32_t msm_twin_buckets(int c) { return ((2u << (c - 1)) + 1u) / 3u; }  // |B| = 2 H / 3 rounded to the nearest integer
// digit magnitude v (1 .. 2^(c-1)) -> bucket id; mult: 0 = the window's own row, 1 = its doubled row
__host__ __device__ static inline uint32_t msm_twin_bucket(int c, uint32_t v, uint32_t& mult) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = (uint32_t)__builtin_ctz(v);
#else
    uint32_t t = 0;
    while (!((v >> t) & 1u)) ++t;
#endif
    mult = t & 1u;
    return msm_twin_class(c, t >> 1).off + ((v >> t) >> 1);
}
// nb: |B|, in whole bins of 128 buckets where the sort places in two passes (MSM_FINE, device/msm_sort.hpp); the buckets behind |B| stay empty
static inline MsmGeom msm_geom_twin(int c) {
    MsmGeom g = msm_geom(c);
    const uint32_t nbk = msm_twin_buckets(c);
    g.nb = (int)(nbk < 128u ? nbk : (nbk + 127u) & ~127u);
    g.twin = 1;
    return g;
}
// digits a scalar that is neither 0 nor 1 is expected to have (x 16: fixed point)
static inline uint32_t msm_mean_digits_x16(const MsmGeom& g) { return (uint32_t)g.W * 16; }

// entries per lane of the accumulation kernel (the gather / heavy-bucket kernels derive the same value)
__host__ __device__ static inline uint32_t msm_chunk_len(uint32_t total, uint32_t nchunks) {
    uint32_t k = (total + nchunks - 1) / nchunks;
    return k < 4 ? 4 : k;  // at least 4 additions per lane: fewer partials to gather
}

// Subset rows behind the window tables of a base set (MsmBases, msm_host.h): for every aligned block of k = 2^bits consecutive bases that
// lies wholly inside [lo, hi), the 2^k - 1 sums of its non-empty subsets.  Block b = scalars k b .. k b + k - 1 by absolute index; the row of
// pattern p != 0 (bit t: base k b + t) is  row0 + (b - b_first)(2^k - 1) + p - 1.  A block of scalars that are all 0 or 1 is then ONE entry
// of bucket 0 instead of up to k (device/msm_sort.hpp: msm_unit_lanes).  bad: one bit per covered block, set where a subset sums to the
// point at infinity (P and -P in one block, a base at infinity): such a block is treated as not covered, so no entry names a row at infinity.
struct MsmSubset {
    uint32_t bits = 0;              // log2 of the block width: 0 = none, else 2 or 3 (blocks tile a 64-lane wave)
    uint32_t b_first = 0, b_end = 0;  // covered blocks [b_first, b_end)
    uint32_t row0 = 0;              // the first subset row = W n (2 W n behind doubled window rows: MsmGeom::tables)
    uint32_t* bad = nullptr;        // [bad_words()] device words (written at load time only)
    __host__ __device__ uint32_t bad_words() const { return (b_end - b_first + 31) / 32; }
    __host__ __device__ uint32_t patterns() const { return (1u << (1u << bits)) - 1u; }
    __host__ __device__ uint64_t rows() const { return bits ? (uint64_t)(b_end - b_first) * patterns() : 0; }
};
// scalars per range (= sorting workgroup) of a proof: a multiple of 64, so that lane l of every wave holds a scalar whose index is l mod 64
// and an aligned block of scalars is an aligned group of lanes
__host__ __device__ static inline uint32_t msm_range_len(uint32_t n, uint32_t ng) { return ((n + ng - 1) / ng + 63u) & ~63u; }

// weighted-sum geometry (k_msm_wsum_level): 128 lanes per workgroup, 2^G_LOG buckets per lane
static constexpr unsigned WSUM_L_LOG = 7, WSUM_L = 1u << WSUM_L_LOG;
static constexpr unsigned WSUM_G_LOG_MIN = 2;
// a lone proof's heavy buckets are shared by MSM_HEAVY_SPLIT workgroups each (device/msm.hpp k_msm_bucket_heavy): slots for their shares
static constexpr unsigned MSM_HEAVY_SPLIT = 8, MSM_HEAVY_SLOTS = 2048;
static constexpr unsigned MSM_SORT_THREADS = 1024;
// the entry that fills the gap behind a bucket's run when runs are aligned (MsmSortBuf::pad_log): the point at infinity
static constexpr uint32_t MSM_PAD_ENTRY = 0xffffffffu;

}  // namespace masp
