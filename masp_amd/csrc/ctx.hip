// libmasp_hip: the context — option resolution, the hardware-queue probe and its stream repair, creation and destruction, the
// context's getters and setters, pinned host memory (include/masp_hip.h).
// There is deliberately NO CPU fallback: without a usable HIP device every entry point fails with MASP_HIP_E_NO_DEVICE.
#include "internal.h"

using namespace masp;

namespace {

// options of a context (include/masp_hip.h: masp_hip_options) with every "0 = default" resolved; no environment is read
static masp_hip_options resolve_options(const masp_hip_options* in) {
    masp_hip_options o;
    memset(&o, 0, sizeof o);
    if (in) memcpy(&o, in, std::min<size_t>(in->struct_size ? in->struct_size : sizeof o, sizeof o));
    o.struct_size = sizeof o;
    // (round 4: with the passes of the bucket tree no longer waiting on memory, three batches in flight keep the chip as busy as
    // four did — 1 227 vs 1 220 proofs/s — and leave their scratch to larger tree sub-batches: 3 x 86 proofs, 1 251 proofs/s, in the
    // ~100 GB that 4 x 64 took; profiles/r04_same_box_sweep_slots_tree_sub.txt)
    // (round 6: FOUR — +1.5 ... 1.7 % host to host over three at the default 16 hardware queues: a batch uploads while three compute;
    // five are not faster, and the measurements of round 5 that made four look no better were taken at 24 queues, in the runtime's
    // oversubscribed regime: profiles/r06_slots_3_4_5_at_16_hardware_queues.txt)
    o.slots = o.slots > 0 ? std::min<int>(o.slots, (int)masp_hip_ctx::MAX_SLOTS) : 4;
    // proofs per batched launch sequence (upper bound: a list of n same-circuit jobs is cut into ceil(n / cap) equal groups);
    // scratch memory follows the batches actually formed
    o.batch_cap = o.batch_cap > 0 ? std::min<int>(o.batch_cap, 256) : 256;
    o.ntt_sub_batch = o.ntt_sub_batch > 0 ? o.ntt_sub_batch : o.ntt_sub_batch < 0 ? 0 : 8;   // resolved: 0 = whole batch
    o.window_bits_b2_lone = o.window_bits_b2_lone > 0 ? o.window_bits_b2_lone : o.window_bits_b2_lone < 0 ? 0 : 8;  // resolved: 0 = not built
    // ~30 % of a MASP witness is neither 0 nor 1; measured +3..5 % throughput vs 100
    o.witness_nontrivial_percent = o.witness_nontrivial_percent > 0 ? std::min<int>(o.witness_nontrivial_percent, 100) : 30;
    o.bucket_tree_levels = o.bucket_tree_levels > 0 ? std::min<int>(o.bucket_tree_levels, 12) : o.bucket_tree_levels < 0 ? -1 : 0;  // resolved: 0 = automatic
    // resolved: 0 = automatic — every base set in as few equal sub-batches as its bounded scratch allows (MsmWorkspace::tree_sub); a value caps them all
    o.bucket_tree_sub_batch = o.bucket_tree_sub_batch > 0 ? std::min<int>(o.bucket_tree_sub_batch, 256) : 0;
    o.bucket_tree_levels_g2 = o.bucket_tree_levels_g2 > 0 ? std::min<int>(o.bucket_tree_levels_g2, 12) : o.bucket_tree_levels_g2 < 0 ? -1 : o.bucket_tree_levels;
    o.bucket_tree_scratch_mb = std::max(o.bucket_tree_scratch_mb, 0);
    o.bucket_tree_fallback_proofs = 0;   // output only
    o.hw_queues = 0;                     // output only (measured when a device context is created)
    o.window_bits_h_lone = o.window_bits_h_lone > 0 ? std::min<int>(o.window_bits_h_lone, 16) : 0;   // resolved: 0 = as window_bits_h
    o.lone_proof_graph = o.lone_proof_graph > 0 ? 1 : 0;   // off unless asked for: measured slower with ROCm 7.2's graph launch
    o.digit_recoding = 0;   // (round 5's NAF digits over per-bit tables were removed in round 6: the field is reserved, must be 0 on input)
    // b_g2's batch tables on a window width of their own (2..16); 0 / -1 resolved where the circuit is loaded (masp_hip_circuit_load)
    o.window_bits_b2 = o.window_bits_b2 > 0 ? std::max(2, std::min<int>(o.window_bits_b2, 16)) : o.window_bits_b2 < 0 ? -1 : 0;
    return o;
}
// `set` on the context and, for a multi-device front, on each of its device contexts, every one under its exclusive lock
template <class F>
static void set_on_all(masp_hip_ctx* ctx, F set) {
    auto locked = [&](masp_hip_ctx* c) {
        std::unique_lock<std::shared_mutex> lock(c->mu);
        set(c);
    };
    locked(ctx);
    for (masp_hip_ctx* c : ctx->children) locked(c);
}

}  // namespace

extern "C" {

const char* masp_hip_strerror(int code) {
    switch (code) {
        case MASP_HIP_OK: return "ok";
        case MASP_HIP_E_INVALID_ARG: return "invalid argument";
        case MASP_HIP_E_PARAMS_FORMAT: return "Parameters bytes are malformed";
        case MASP_HIP_E_PARAMS_SHAPE: return "Parameters do not match the circuit shape";
        case MASP_HIP_E_NO_DEVICE: return "no usable HIP device (there is no CPU fallback)";
        case MASP_HIP_E_HIP: return "HIP runtime error";
        case MASP_HIP_E_UNEXPECTED_IDENTITY: return "delta is the identity, or the toxic waste would put the identity into h (UnexpectedIdentity)";
        case MASP_HIP_E_NOT_LOADED: return "circuit slot is empty";
        case MASP_HIP_E_SCALAR_RANGE: return "scalar is not a canonical field element";
        case MASP_HIP_E_POINT_ENCODING: return "a Jubjub point encoding does not decode";
        case MASP_HIP_E_CAPACITY: return "an output buffer is too small";
        default: return "unknown error";
    }
}

// The text is copied under the lock into a buffer of the calling thread: concurrent provers that fail at the same time
// each read a consistent message, and the pointer stays valid until this thread asks again.
const char* masp_hip_last_error(const masp_hip_ctx* ctx) {
    static thread_local std::string copy;
    if (!ctx) return "";
    if (!ctx->children.empty()) {
        for (const masp_hip_ctx* ch : ctx->children) {
            const char* e = masp_hip_last_error(ch);
            if (e[0]) return e;
        }
        return "";
    }
    std::lock_guard<std::mutex> g(ctx->slot_mu);
    copy = ctx->err;
    return copy.c_str();
}

int masp_hip_device_count(void) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && count > 0 ? count : 0;
}

int masp_hip_device_pci_bus_id(int device, char* out, size_t cap) {
    if (!out || cap < 13) return MASP_HIP_E_INVALID_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return MASP_HIP_E_NO_DEVICE;
    return hipDeviceGetPCIBusId(out, (int)std::min<size_t>(cap, 64), device) == hipSuccess ? MASP_HIP_OK : MASP_HIP_E_HIP;
}

int masp_hip_runtime_prepare(int hw_queues, int overwrite) {
    char v[16];
    // (never more than 20: the runtime creates a hardware queue per new stream up to this number and never gives one back, and a process
    // that holds 24 / 32 of them dispatches every kernel 7 / 21 % slower — profiles/r06_second_context_root_cause.txt)
    snprintf(v, sizeof v, "%d", hw_queues > 0 ? std::min(hw_queues, (int)MASP_HIP_MAX_USEFUL_HW_QUEUES) : 16);
    setenv("GPU_MAX_HW_QUEUES", v, overwrite ? 1 : 0);
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    return e ? atoi(e) : 0;
}
// (see masp_hip_runtime_prepare in include/masp_hip.h: the one thing the library does to the environment)
__attribute__((constructor)) static void masp_hip_on_load() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

void masp_hip_options_default(masp_hip_options* opt) {
    if (!opt) return;
    memset(opt, 0, sizeof *opt);   // every field: 0 = the default (resolved when a context is created)
    opt->struct_size = sizeof *opt;
}

// ---- how many hardware queues do this process's streams really get?  (masp_hip_options::hw_queues) -------------------------------
// One single-wave kernel per stream, all launched at once, each spinning for 2 ms of the constant wall clock and leaving its
// [start, end): the largest number of them that overlapped = the hardware queues the streams were spread over (streams that share a
// queue run one after the other).
static __global__ void k_hwq_spin(unsigned long long* out, int idx, long long ticks) {
    const long long t0 = wall_clock64();
    // (bounded: a clock that does not advance must not hang the context's creation — 2^22 polls are ~100 ms)
    for (int it = 0; it < (1 << 22) && wall_clock64() - t0 < ticks; ++it) {
    }
    out[2 * idx] = (unsigned long long)t0;
    out[2 * idx + 1] = (unsigned long long)wall_clock64();
}
// ticks of wall_clock64() per millisecond on the current device (hipDeviceAttributeWallClockRate, kHz: 100 000 on gfx950); 0 if unknown
static long long wall_clock_per_ms() {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
}
// The probe on the streams `ss`: *concurrent = the largest number of them that ran their kernel at the same time, *intervals = every
// stream's [start, end).  The intervals are read back on ss[0], the probe's own stream: the probe waits for no other context's work.
// MASP_HIP_E_HIP and last_hip_error() if it failed (nothing written then).
static int measure_streams(const std::vector<hipStream_t>& ss, int* concurrent, std::vector<unsigned long long>* intervals = nullptr) {
    const int n = (int)ss.size();
    const long long ms = wall_clock_per_ms();
    unsigned long long* d = nullptr;
    HIP_TRY(dev_malloc(&d, 16 * n));
    (void)hipGetLastError();   // (what an earlier call of this thread left behind is not the probe's failure)
    bool ok = ms > 0;
    for (int r = 0; r < 2 && ok; ++r) {  // (the first round loads the code object and creates the queues)
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_hwq_spin, dim3(1), dim3(64), 0, ss[i], d, i, r ? 2 * ms : ms / 100);
        for (int i = 0; i < n; ++i) ok = hipStreamSynchronize(ss[i]) == hipSuccess && ok;
    }
    std::vector<unsigned long long> h(2 * n);
    ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(h.data(), d, 16 * n, hipMemcpyDeviceToHost, ss[0]) == hipSuccess &&
         hipStreamSynchronize(ss[0]) == hipSuccess;
    (void)dev_free(d);
    if (!ok) {
        last_hip_error() = "stream concurrency probe failed";
        return MASP_HIP_E_HIP;
    }
    int best = 0;
    for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int j = 0; j < n; ++j) c += h[2 * j] <= h[2 * i] && h[2 * i] < h[2 * j + 1];
        best = std::max(best, c);
    }
    *concurrent = best;
    if (intervals) *intervals = std::move(h);
    return MASP_HIP_OK;
}
// The probe on temporary streams, created and destroyed BEFORE the context creates its own; 0 if it failed.
// Measured ONCE per (process, device) and remembered: the runtime fixes its queue count at the process's first HIP call, so a second
// context has nothing new to learn — and its probe would wait behind, and share the chip with, whatever the first context is running
// (ADVICE r05).  The probe synchronises its own streams only, and its buffer goes through dev_malloc / dev_free like every other.
static int measure_hw_queues(int device, int streams) {
    static std::mutex mu;
    static std::map<int, int> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    // (at most one more than MASP_HIP_MAX_USEFUL_HW_QUEUES: every stream created here makes the runtime create a hardware queue that it
    // keeps for the life of the process — the probe must not itself walk the pool into the slow regime; 21 says "more than 20")
    const int n = std::max(1, std::min(streams, (int)MASP_HIP_MAX_USEFUL_HW_QUEUES + 1));
    std::vector<hipStream_t> ss;
    for (int i = 0; i < n; ++i) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
        ss.push_back(s);
    }
    int best = 0;
    if ((int)ss.size() == n) (void)measure_streams(ss, &best);
    for (hipStream_t s : ss) (void)hipStreamDestroy(s);
    (void)hipGetLastError();
    if (best > 0) known[device] = best;
    return best;
}

// The streams that work side by side — the context's own, every slot's main stream (the ones that carry batches) and the verifier's
// two —, as places in the stream table
static std::vector<hipStream_t*> main_streams_of(StreamTable& t) {
    std::vector<hipStream_t*> at{&t.main};
    for (auto& row : t.slot) at.push_back(&row[0]);
    for (hipStream_t& v : t.vk) at.push_back(&v);
    return at;
}
// The same measurement on a context's OWN streams (mains_only: main_streams_of; else every distinct one): how many of them run a kernel at
// the same time.  Fewer than there are streams = two of them share a hardware queue, and kernels that could overlap wait for each other.
static int measure_own_streams(masp_hip_ctx* ctx, bool mains_only, int* n_streams, int* concurrent) {
    std::vector<hipStream_t> ss;
    if (mains_only)
        for (hipStream_t* p : main_streams_of(ctx->streams)) ss.push_back(*p);
    else
        ss = ctx->streams.distinct();
    const int rc = measure_streams(ss, concurrent);
    if (rc == MASP_HIP_OK) *n_streams = (int)ss.size();
    return rc;
}

// The streams that carry batches — the context's own and every slot's main stream — must each sit on a hardware queue of its own: two
// of them on one queue run their batches one after the other (a later context of a process at 4 slots: -6 %, profiles/
// r06_second_context_root_cause.txt).  Which queue the runtime gives a new stream depends on everything the process has created before and
// cannot be asked, so it is MEASURED: a 2 ms single-wave kernel on each of them at once; a stream that starts a millisecond late shares its
// queue with the one that ended when it started.  Such a stream is replaced — the new one is created BEFORE the old one is destroyed, so
// that it cannot get the same queue back — and the measurement repeated, a few times at most.  Nothing has been launched on these streams
// yet.  Slot 0's main stream is never the one replaced (a lone proof runs 0.4 ms longer when its main stream was not created right in
// front of its side streams: profiles/r06_slot_streams_creation_order.txt).
static int separate_main_streams(masp_hip_ctx* ctx) {
    const unsigned long long ms = (unsigned long long)wall_clock_per_ms();
    for (int attempt = 0; attempt < 8; ++attempt) {
        const std::vector<hipStream_t*> at = main_streams_of(ctx->streams);   // (the verifier's streams work next to the batches: the same rule)
        std::vector<hipStream_t> ss;
        for (hipStream_t* p : at) ss.push_back(*p);
        const int n = (int)ss.size();
        int conc = 0;
        std::vector<unsigned long long> h;
        if (int rc = measure_streams(ss, &conc, &h)) return rc;
        ctx->main_streams_concurrent = conc;
        if (conc >= n) return MASP_HIP_OK;
        unsigned long long t0 = ~0ull;
        for (int i = 0; i < n; ++i) t0 = std::min(t0, h[2 * i]);
        bool replaced = false;
        for (int i = 0; i < n; ++i) {
            if (h[2 * i] - t0 < ms) continue;                  // started with the others (within 1 ms)
            int partner = -1;                                  // the stream whose kernel ended when this one's began
            unsigned long long bestd = ~0ull;
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                const unsigned long long d = h[2 * j + 1] > h[2 * i] ? h[2 * j + 1] - h[2 * i] : h[2 * i] - h[2 * j + 1];
                if (d < bestd) bestd = d, partner = j;
            }
            const int victim = i == 1 && partner >= 0 ? partner : i;   // (index 1 = slot 0's main stream)
            if (victim == 1) continue;
            hipStream_t fresh = nullptr;
            if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) return MASP_HIP_E_HIP;
            (void)hipStreamDestroy(*at[victim]);
            *at[victim] = fresh;
            replaced = true;
        }
        if (!replaced) return MASP_HIP_OK;
    }
    return MASP_HIP_OK;   // (still shared after eight rounds: a process with fewer queues than main streams — reported, not an error)
}

static int create_single(int device, const masp_hip_options& opt, masp_hip_ctx** out) {
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return MASP_HIP_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return MASP_HIP_E_NO_DEVICE;
    std::unique_ptr<masp_hip_ctx> ctx(new masp_hip_ctx);
    ctx->device = device;
    ctx->opt = opt;
    ctx->n_slots = opt.slots;
    ctx->batch_cap = (size_t)opt.batch_cap;
    ctx->slots.reserve(masp_hip_ctx::MAX_SLOTS);      // never reallocates: see the locking note on masp_hip_ctx
    ctx->slot_busy.reserve(masp_hip_ctx::MAX_SLOTS);
    ctx->opt.hw_queues = measure_hw_queues(device, 5 * opt.slots);   // (a slot has up to five streams)
    // Every stream of the context (masp_hip_ctx::streams; on failure the table destroys what was created), in this order: the context's
    // own; slot by slot, a slot's main stream right in front of its side streams (a lone proof takes the first free slot, i.e. slot 0, and
    // runs 0.3 - 0.4 ms longer when its side streams were not created right behind its main stream — measured three ways, not understood:
    // profiles/r06_slot_streams_creation_order.txt); the verifier's two.  From slot 2 on a slot's side streams are slot 1's, unless lone
    // proofs are replayed from captured graphs.  That the main streams then do not share hardware queues is measured and repaired:
    // separate_main_streams
    StreamTable& t = ctx->streams;
    bool ok = hipStreamCreateWithFlags(&t.main, hipStreamNonBlocking) == hipSuccess;
    t.slot.assign((size_t)opt.slots, std::array<hipStream_t, 5>{});
    for (size_t si = 0; si < t.slot.size(); ++si)
        for (int j = 0; j < 5; ++j) {
            if (j > 0 && si >= 2 && !opt.lone_proof_graph)
                t.slot[si][j] = t.slot[1][j];
            else
                ok = ok && hipStreamCreateWithFlags(&t.slot[si][j], hipStreamNonBlocking) == hipSuccess;
        }
    for (hipStream_t& v : t.vk) ok = ok && hipStreamCreateWithFlags(&v, hipStreamNonBlocking) == hipSuccess;
    if (!ok || separate_main_streams(ctx.get()) != MASP_HIP_OK) return MASP_HIP_E_NO_DEVICE;
    *out = ctx.release();
    return MASP_HIP_OK;
}

// a multi-device front: one device context per entry of `devices`
static int create_front(const int* devices, int n_devices, const masp_hip_options& opt, masp_hip_ctx** out) {
    std::unique_ptr<masp_hip_ctx> front(new masp_hip_ctx);
    front->device = devices[0];
    front->opt = opt;
    front->n_slots = opt.slots;
    front->batch_cap = (size_t)opt.batch_cap;
    for (int i = 0; i < n_devices; ++i) {
        masp_hip_ctx* ch = nullptr;
        if (int rc = create_single(devices[i], opt, &ch)) {
            for (masp_hip_ctx* c : front->children) masp_hip_ctx_destroy(c);
            return rc;
        }
        front->children.push_back(ch);
    }
    front->dev_status.reset(new std::atomic<int>[n_devices]);
    for (int i = 0; i < n_devices; ++i) front->dev_status[i] = MASP_HIP_OK;
    *out = front.release();
    return MASP_HIP_OK;
}

int masp_hip_ctx_create_ex(const int* devices, int n_devices, const masp_hip_options* opt_in, masp_hip_ctx** out) {
    if (!out || !devices || n_devices <= 0 || n_devices > 64) return MASP_HIP_E_INVALID_ARG;
    if (opt_in && opt_in->struct_size != 0 && opt_in->struct_size < 4 * sizeof(int32_t)) return MASP_HIP_E_INVALID_ARG;
    *out = nullptr;
    const masp_hip_options opt = resolve_options(opt_in);
    return n_devices == 1 ? create_single(devices[0], opt, out) : create_front(devices, n_devices, opt, out);
}

int masp_hip_ctx_get_options(const masp_hip_ctx* ctx, masp_hip_options* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    const masp_hip_ctx* c = ctx->children.empty() ? ctx : ctx->children[0];
    // `out->struct_size` on entry = the size of the CALLER's struct (0: this header's): a binding built against an older, shorter
    // masp_hip_options gets only the bytes its struct has room for (the plain assignment wrote sizeof(new struct) into it)
    const size_t room = out->struct_size ? std::min<size_t>(out->struct_size, sizeof(masp_hip_options)) : sizeof(masp_hip_options);
    if (room < 4 * sizeof(int32_t)) return MASP_HIP_E_INVALID_ARG;
    masp_hip_options full = c->opt, *const caller_out = out;
    out = &full;
    // what lack of tree scratch has changed since the context was created: the smallest sub-batch any slot works with now, and
    // the proofs whose bucket runs went through the XYZZ accumulation instead (all device contexts)
    // (bucket_tree_sub_batch automatic: the smallest sub-batch any MSM has gone through the tree with, 256 before the first)
    uint64_t fb = 0;
    int sub = out->bucket_tree_sub_batch ? out->bucket_tree_sub_batch : 256;
    auto scan = [&](const masp_hip_ctx* d) {
        std::lock_guard<std::mutex> g(d->slot_mu);
        for (const auto& sl : d->slots) {
            // (tree_over: proofs with more entries than the tree's views were cut for, counted on the device — exact once the calls
            // that proved them have returned)
            fb += sl->ws1.tree_fallbacks + sl->ws2.tree_fallbacks + sl->ws1.tree_over() + sl->ws2.tree_over();
            for (const uint32_t v : {sl->ws1.tree_sub, sl->ws2.tree_sub, sl->ws1.tree_sub_used, sl->ws2.tree_sub_used})
                if (v) sub = std::min<int>(sub, (int)std::min<uint32_t>(v, 256u));
        }
    };
    if (ctx->children.empty())
        scan(ctx);
    else
        for (const masp_hip_ctx* d : ctx->children) scan(d);
    fb += c->block_tree_fallbacks.load();
    if (c->block_tree_sub.load() != 0xffffffffu) sub = std::min<int>(sub, (int)c->block_tree_sub.load());
    out->bucket_tree_sub_batch = sub;
    out->bucket_tree_fallback_proofs = (int32_t)std::min<uint64_t>(fb, 0x7fffffff);
    full.struct_size = (uint32_t)room;   // the bytes written
    memcpy(caller_out, &full, room);
    return MASP_HIP_OK;
}

int masp_hip_ctx_set_boolean_block_bits(masp_hip_ctx* ctx, int32_t bits) {
    if (!ctx || (bits != 0 && bits != -1 && bits != 2 && bits != 3)) return MASP_HIP_E_INVALID_ARG;
    const int resolved = bits == 0 ? (int)(MASP_SUBSET_BITS) : bits < 0 ? 0 : bits;
    set_on_all(ctx, [&](masp_hip_ctx* c) { c->boolean_block_bits = resolved; });
    return MASP_HIP_OK;
}
int masp_hip_ctx_get_boolean_block_bits(const masp_hip_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = (ctx->children.empty() ? ctx : ctx->children[0])->boolean_block_bits;
    return MASP_HIP_OK;
}

int masp_hip_ctx_set_window_row_multiples(masp_hip_ctx* ctx, int32_t v) {
    if (!ctx || v < -1 || v > 2) return MASP_HIP_E_INVALID_ARG;
    const int resolved = v == 0 ? (int)(MASP_TWIN_ROWS) : v < 0 ? 0 : v == 1 ? 3 : 1;
    set_on_all(ctx, [&](masp_hip_ctx* c) { c->twin_rows = resolved; c->twin_rows_msm = v == 1; });
    return MASP_HIP_OK;
}
int masp_hip_ctx_get_window_row_multiples(const masp_hip_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = (ctx->children.empty() ? ctx : ctx->children[0])->twin_rows;
    return MASP_HIP_OK;
}

int masp_hip_ctx_set_quotient_form(masp_hip_ctx* ctx, int32_t form) {
    if (!ctx || (form != MASP_HIP_QUOTIENT_EVALUATION && form != MASP_HIP_QUOTIENT_COEFFICIENT)) return MASP_HIP_E_INVALID_ARG;
    set_on_all(ctx, [&](masp_hip_ctx* c) { c->quotient_form = form; });
    return MASP_HIP_OK;
}
int masp_hip_ctx_get_quotient_form(const masp_hip_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = (ctx->children.empty() ? ctx : ctx->children[0])->quotient_form;
    return MASP_HIP_OK;
}

int masp_hip_ctx_set_quotient_schedule(masp_hip_ctx* ctx, int32_t schedule) {
    if (!ctx || (schedule != MASP_HIP_QUOTIENT_FUSED && schedule != MASP_HIP_QUOTIENT_SEPARATE)) return MASP_HIP_E_INVALID_ARG;
    ctx->quotient_schedule.store(schedule, std::memory_order_relaxed);
    for (masp_hip_ctx* c : ctx->children) c->quotient_schedule.store(schedule, std::memory_order_relaxed);
    return MASP_HIP_OK;
}
int masp_hip_ctx_get_quotient_schedule(const masp_hip_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = (ctx->children.empty() ? ctx : ctx->children[0])->quotient_schedule.load(std::memory_order_relaxed);
    return MASP_HIP_OK;
}

int masp_hip_ctx_set_tree_entry_share(masp_hip_ctx* ctx, int32_t percent) {
    if (!ctx || percent < 0 || percent > 100) return MASP_HIP_E_INVALID_ARG;
    const int resolved = percent == 0 ? (int)(MASP_TREE_ENTRY_SHARE) : percent;
    set_on_all(ctx, [&](masp_hip_ctx* c) { c->tree_entry_share = resolved; });
    return MASP_HIP_OK;
}
int masp_hip_ctx_get_tree_entry_share(const masp_hip_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = (ctx->children.empty() ? ctx : ctx->children[0])->tree_entry_share;
    return MASP_HIP_OK;
}

int masp_hip_ctx_create(int device, masp_hip_ctx** out) {
    if (!out) return MASP_HIP_E_INVALID_ARG;
    return masp_hip_ctx_create_ex(&device, 1, nullptr, out);
}

// (a list of ONE device still gives the multi-device front: its callers test the sharding path with the same GPU listed twice
// or once)
int masp_hip_ctx_create_multi(const int* devices, int n_devices, masp_hip_ctx** out) {
    if (!out || !devices || n_devices <= 0 || n_devices > 64) return MASP_HIP_E_INVALID_ARG;
    *out = nullptr;
    return create_front(devices, n_devices, resolve_options(nullptr), out);
}

int masp_hip_ctx_device_proofs(const masp_hip_ctx* ctx, uint64_t* counts, int cap) {
    if (!ctx || !counts || cap < 0) return MASP_HIP_E_INVALID_ARG;
    if (ctx->children.empty()) {
        if (cap >= 1) counts[0] = ctx->proofs_done.load();
        return MASP_HIP_OK;
    }
    for (size_t d = 0; d < ctx->children.size() && (int)d < cap; ++d) counts[d] = ctx->children[d]->proofs_done.load();
    return MASP_HIP_OK;
}
int masp_hip_ctx_device_status(const masp_hip_ctx* ctx, int32_t* status, int cap, uint64_t* requeued) {
    if (!ctx || !status || cap < 0) return MASP_HIP_E_INVALID_ARG;
    if (requeued) *requeued = ctx->requeued.load();
    if (ctx->children.empty()) {
        if (cap >= 1) status[0] = MASP_HIP_OK;
        return MASP_HIP_OK;
    }
    for (size_t d = 0; d < ctx->children.size() && (int)d < cap; ++d) status[d] = ctx->dev_status[d].load();
    return MASP_HIP_OK;
}
int masp_hip_ctx_inject_fault(masp_hip_ctx* ctx, int device, uint32_t nth) {
    if (!ctx || device < 0) return MASP_HIP_E_INVALID_ARG;
    if (ctx->children.empty()) {
        if (device != 0) return MASP_HIP_E_INVALID_ARG;
        ctx->fault_countdown = nth;
        return MASP_HIP_OK;
    }
    if ((size_t)device >= ctx->children.size()) return MASP_HIP_E_INVALID_ARG;
    ctx->children[device]->fault_countdown = nth;
    return MASP_HIP_OK;
}
int masp_hip_ctx_stream_concurrency(masp_hip_ctx* ctx, int mains_only, int* n_streams, int* concurrent) {
    if (!ctx || !n_streams || !concurrent) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) ctx = ctx->children[0];
    std::unique_lock<std::shared_mutex> lock(ctx->mu);
    hipSetDevice(ctx->device);
    if (hipDeviceSynchronize() != hipSuccess) return fail(ctx, MASP_HIP_E_HIP);
    return fail(ctx, measure_own_streams(ctx, mains_only != 0, n_streams, concurrent));
}
int masp_hip_ctx_lone_graph_launches(const masp_hip_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return MASP_HIP_E_INVALID_ARG;
    *out = 0;
    if (!ctx->children.empty()) {
        for (const masp_hip_ctx* ch : ctx->children) {
            uint64_t v = 0;
            masp_hip_ctx_lone_graph_launches(ch, &v);
            *out += v;
        }
        return MASP_HIP_OK;
    }
    std::lock_guard<std::mutex> g(ctx->slot_mu);
    for (const auto& sl : ctx->slots) *out += sl->graph_launches.load();
    return MASP_HIP_OK;
}
int masp_hip_ctx_device_count(const masp_hip_ctx* ctx) { return !ctx ? 0 : ctx->children.empty() ? 1 : (int)ctx->children.size(); }

void masp_hip_ctx_destroy(masp_hip_ctx* ctx) {
    if (!ctx) return;
    if (!ctx->children.empty()) {
        for (masp_hip_ctx* c : ctx->children) masp_hip_ctx_destroy(c);
        delete ctx;
        return;
    }
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    ctx->batches.clear();
    ctx->slots.clear();
    for (auto& c : ctx->circ) c.reset();
    ctx->domains.clear();
    delete ctx;   // (and with it every stream: masp_hip_ctx::streams)
    dev_free_drain();  // the context's buffers
}

void* masp_hip_host_alloc(masp_hip_ctx* ctx, size_t bytes) {
    if (!ctx || !bytes) return nullptr;
    hipSetDevice(ctx->device);
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {  // portable: every device of a multi-device context may read it
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void masp_hip_host_free(masp_hip_ctx* ctx, void* ptr) {
    if (!ctx || !ptr) return;
    hipSetDevice(ctx->device);
    hipHostFree(ptr);
}

int masp_hip_sync(masp_hip_ctx* ctx) {
    if (!ctx) return MASP_HIP_E_INVALID_ARG;
    if (!ctx->children.empty()) {
        for (masp_hip_ctx* c : ctx->children)
            if (int rc = masp_hip_sync(c)) return rc;
        return MASP_HIP_OK;
    }
    hipSetDevice(ctx->device);
    return hipDeviceSynchronize() == hipSuccess ? MASP_HIP_OK : MASP_HIP_E_HIP;
}

}  // extern "C"
