// Test-only unit over the MSM's stages on a base set with doubled window rows (msm_geom_twin, masp_amd/csrc/device/msm_geom.h): the counting
// sort, the table the loader builds, the accumulation and the bucket tails — each through the product's own drivers (msm_sort_enqueue,
// MsmBases::load_host, msm_launch_accumulate, msm_tails_enqueue), as tests/native/msm_stages_dev.hip runs them for the plain geometry.  No
// kernel is copied here.  Built once per curve (tests/msm_twin_shim.py): without MTW_G2 the sort and G1, with it G2.
// Everything that crosses this boundary is plain integers and canonical bytes: scalars 32 bytes little-endian, points in the bellman
// uncompressed wire format (the identity 0x40 then zeros).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_TAILS_QUAD_UNIT  // (this unit instantiates what it uses of msm_tails_enqueue itself)
#define MASP_TAILS_OCT_UNIT
#include "../../masp_amd/csrc/msm_impl.hpp"
#include "../../masp_amd/csrc/msm_acc_impl.hpp"
#ifndef MTW_G2
#include "../../masp_amd/csrc/k_msm_sort.hip"
#endif

using namespace masp;

namespace {

constexpr int POISON = 0xA5;

#ifdef MTW_G2
typedef Fp2Ops O;
constexpr int WIRE = 192;
#else
typedef FpOps O;
constexpr int WIRE = 96;
#endif
typedef typename TailLaneOps<O>::type Tails;

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
#define MTW_TRY(expr)                        \
    do {                                     \
        if ((expr) != hipSuccess) return -2; \
    } while (0)

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

__global__ void __launch_bounds__(64) k_mtw_export_xyzz(const Xyzz<O>* __restrict__ p, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<O> a = xyzz_to_affine<O>(p[i]);
#ifdef MTW_G2
    g2_write_uncompressed(a, out + (size_t)WIRE * i);
#else
    g1_write_uncompressed(a, out + (size_t)WIRE * i);
#endif
}
__global__ void __launch_bounds__(64) k_mtw_export_rows(const TabRow<O>* __restrict__ tab, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#ifdef MTW_G2
    g2_write_uncompressed(tab[i].p, out + (size_t)WIRE * i);
#else
    g1_write_uncompressed(tab[i].p, out + (size_t)WIRE * i);
#endif
}

}  // namespace

#ifdef MTW_G2
#define MTW_NAME(f) mtw_g2_##f
#else
#define MTW_NAME(f) mtw_g1_##f
#endif

extern "C" {

#ifndef MTW_G2
uint64_t mtw_padded_entries(uint32_t n, int c, uint32_t pad_log) { return MsmSortBuf::padded_entries(n, msm_geom_twin(c), pad_log); }

// scalars: np x n x 32 bytes.  sub_bits 0: no subset rows; else blocks [b_first, b_end) and their bad-block bitmap, behind the doubled tables.
// -> start, dense: np x (nb + 1); sorted: np x mtw_padded_entries(n, c, pad_log) words.  Every buffer of the sort holds 0xA5 first.
int mtw_sort(const uint8_t* scalars, uint32_t n, int c, uint32_t np, uint32_t pad_log, uint32_t sub_bits, uint32_t b_first, uint32_t b_end,
             const uint32_t* bad_words, uint32_t* start, uint32_t* dense, uint32_t* sorted) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0 || np == 0) return -1;
    const MsmGeom g = msm_geom_twin(c);
    MsmSortBuf sb;
    Scope sc;
    uint32_t* d_scalars = sc.alloc<uint32_t>((size_t)np * n * 8);
    if (!d_scalars) return -2;
    MTW_TRY(hipMemcpyAsync(d_scalars, scalars, (size_t)np * n * 32, hipMemcpyHostToDevice, s));
    MsmSubset sub;
    if (sub_bits) {
        sub.bits = sub_bits;
        sub.b_first = b_first;
        sub.b_end = b_end;
        sub.row0 = n * (uint32_t)g.tables();
        sub.bad = sc.alloc<uint32_t>(sub.bad_words());
        if (!sub.bad) return -2;
        MTW_TRY(hipMemcpyAsync(sub.bad, bad_words, 4 * (size_t)sub.bad_words(), hipMemcpyHostToDevice, s));
    }
    const uint64_t rows = (uint64_t)n * (uint32_t)g.tables() + sub.rows();
    if (sb.reserve(n, g, np, pad_log, rows)) return -5;
    const size_t ent = std::max<size_t>(sb.cap_ent, 1);
    MTW_TRY(hipMemsetAsync(sb.sorted, POISON, sb.cap_np * 4 * ent, s));
    MTW_TRY(hipMemsetAsync(sb.tmp, POISON, sb.cap_np * 4 * ent, s));
    MTW_TRY(hipMemsetAsync(sb.hist_wg, POISON, 4 * sb.cap_hist, s));
    MTW_TRY(hipMemsetAsync(sb.crel, POISON, 4 * sb.cap_crel, s));
    MTW_TRY(hipMemsetAsync(sb.dense, POISON, sb.cap_np * 4 * (sb.cap_nb + 1), s));
    MTW_TRY(hipMemsetAsync(sb.start, POISON, sb.cap_np * 4 * (sb.cap_nb + 1), s));
    if (msm_sort_enqueue(s, n, g, sb, d_scalars, (size_t)n * 8, np, pad_log, sub)) return -6;
    const size_t words = (size_t)g.nb + 1;
    MTW_TRY(hipMemcpyAsync(start, sb.start, 4 * words * np, hipMemcpyDeviceToHost, s));
    MTW_TRY(hipMemcpyAsync(dense, sb.dense, 4 * words * np, hipMemcpyDeviceToHost, s));
    MTW_TRY(hipMemcpyAsync(sorted, sb.sorted, 4 * sb.ent_stride * np, hipMemcpyDeviceToHost, s));
    return finish(s);
}
#endif  // !MTW_G2

// The table MsmBases::load_host builds when asked for doubled rows.  -> rows: the window rows and whatever lies behind them up to
// B.rows() (at most rows_cap), as wire bytes; info: twin (0: the set kept the plain geometry), W, nb, rows, the first subset row, import status
int MTW_NAME(table)(const uint8_t* bases, uint32_t n, int c, int sub_bits, uint8_t* rows, uint64_t rows_cap, uint32_t info[6]) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0) return -1;
    MsmBases<O, WIRE> B;
    if (B.load_host(bases, n, s, n, c, sub_bits, 0, 0xffffffffu, true)) return -5;
    info[0] = (uint32_t)B.g.twin;
    info[1] = (uint32_t)B.g.W;
    info[2] = (uint32_t)B.g.nb;
    info[3] = (uint32_t)B.rows();
    info[4] = B.sub.row0;
    info[5] = (uint32_t)B.import_status;
    if (B.rows() > rows_cap) return -11;
    Scope sc;
    const uint32_t nr = (uint32_t)B.rows();
    uint8_t* d_out = sc.alloc<uint8_t>((size_t)WIRE * nr);
    if (!d_out) return -2;
    MASP_LAUNCH(k_mtw_export_rows, dim3((nr + 63) / 64), dim3(64), 0, s, B.tab, nr, d_out);
    MTW_TRY(hipMemcpyAsync(rows, d_out, (size_t)WIRE * nr, hipMemcpyDeviceToHost, s));
    return finish(s);
}

// The accumulation over a hand-made digit list (packed runs) on the doubled tables, then the tails as msm_reduce_enqueue takes them for
// such a set: the one-lane / lane-pair form, for a lone proof too.  sorted: np x ent_stride words, start: np x (nb + 1).
// -> bkt: np x nb points, result: np points
int MTW_NAME(tails)(const uint8_t* bases, uint32_t n, int c, const uint32_t* sorted, const uint32_t* start, uint32_t np, uint64_t ent_stride,
                    uint32_t nchunks, int lone, uint8_t* bkt, uint8_t* result) {
    const ApiLaunchScope api_scope;
    hipStream_t s = stream();
    if (!s || n == 0 || np == 0 || nchunks == 0) return -1;
    MsmBases<O, WIRE> B;
    if (B.load_host(bases, n, s, n, c, 0, 0, 0xffffffffu, true)) return -5;
    if (!B.g.twin) return -9;
    const MsmGeom g = B.g;
    const uint32_t nb = (uint32_t)g.nb;
    // the list is checked before any kernel sees it: offsets that grow inside the proof's slice, entries that name a row of the table
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t* st = start + (size_t)p * (nb + 1);
        if (st[0] != 0 || st[nb] > ent_stride) return -10;
        for (uint32_t b = 0; b < nb; ++b)
            if (st[b + 1] < st[b]) return -10;
        for (uint32_t k = 0; k < st[nb]; ++k)
            if ((sorted[(size_t)p * ent_stride + k] & 0x7fffffffu) >= B.rows()) return -10;
    }
    MsmWorkspace<O> ws;
    if (ws.reserve(n, g, np)) return -5;
    if ((size_t)np * ((size_t)nchunks + nb) > ws.cap_part) return -11;
    if (hipFuncSetAttribute((const void*)k_xyzz_reduce_block<O>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(Xyzz<O>)) != hipSuccess) return -5;
    const size_t P = ws.cap_np, chunks = (ws.cap_nb + (1u << MsmWorkspace<O>::CS_LOG) - 1) >> MsmWorkspace<O>::CS_LOG, X = sizeof(Xyzz<O>);
    MTW_TRY(hipMemsetAsync(ws.part, POISON, X * ws.cap_part, s));
    MTW_TRY(hipMemsetAsync(ws.bkt, POISON, P * X * ws.cap_nb, s));
    Xyzz<O>* small[] = {ws.S[0], ws.S[1], ws.T};
    for (Xyzz<O>* b : small) MTW_TRY(hipMemsetAsync(b, POISON, P * X * chunks, s));
    MTW_TRY(hipMemsetAsync(ws.n_heavy, 0, 4 * np, s));
    Scope sc;
    uint32_t* d_sorted = sc.alloc<uint32_t>((size_t)np * ent_stride);
    uint32_t* d_start = sc.alloc<uint32_t>((size_t)np * (nb + 1));
    Xyzz<O>* d_res = sc.alloc<Xyzz<O>>(np);
    uint8_t* d_bkt = sc.alloc<uint8_t>((size_t)WIRE * np * nb);
    uint8_t* d_out = sc.alloc<uint8_t>((size_t)WIRE * np);
    if (!d_sorted || !d_start || !d_res || !d_bkt || !d_out) return -2;
    MTW_TRY(hipMemcpyAsync(d_sorted, sorted, 4 * (size_t)np * ent_stride, hipMemcpyHostToDevice, s));
    MTW_TRY(hipMemcpyAsync(d_start, start, 4 * (size_t)np * (nb + 1), hipMemcpyHostToDevice, s));
    MTW_TRY(hipMemsetAsync(d_res, POISON, sizeof(Xyzz<O>) * np, s));
    msm_launch_accumulate<O>(s, B.tab, d_sorted, ent_stride, d_start, nb, nchunks, ws.part, np);
    msm_tails_enqueue<O, Tails>(s, ws, d_start, nb, nchunks, np, lone != 0, d_res, 1, g.c);
    MASP_LAUNCH(k_mtw_export_xyzz, dim3((np * nb + 63) / 64), dim3(64), 0, s, ws.bkt, np * nb, d_bkt);
    MASP_LAUNCH(k_mtw_export_xyzz, dim3((np + 63) / 64), dim3(64), 0, s, d_res, np, d_out);
    MTW_TRY(hipMemcpyAsync(bkt, d_bkt, (size_t)WIRE * np * nb, hipMemcpyDeviceToHost, s));
    MTW_TRY(hipMemcpyAsync(result, d_out, (size_t)WIRE * np, hipMemcpyDeviceToHost, s));
    return finish(s);
}

}  // extern "C"
