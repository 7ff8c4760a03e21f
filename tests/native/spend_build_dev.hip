// Test-only shim over the spend descriptions' and signatures' device code: masp_amd/csrc/device/spend_build.hpp on the host (the header is
// __host__ __device__), stage by stage over one block of memory that holds everything the kernels hand each other, and the product's own
// kernels (masp_amd/csrc/k_spend_build.hip, its kernel half) on the GPU over the same block, one kernel alone or all of them, without a
// context.  The tables are the product's (spend_table.h, output_table.h, nullifier_table.h, pedersen_table.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_SB_KERNELS_ONLY
#include "../../masp_amd/csrc/k_spend_build.hip"
#include "../../masp_amd/csrc/spend_table.h"

using namespace masp;

namespace {

// rows as they come, copied where the device code reads words
std::vector<uint32_t> words(const uint8_t* src, size_t bytes) {
    std::vector<uint32_t> v(bytes / 4 + 1, 0);
    if (src) memcpy(v.data(), src, bytes);
    return v;
}

struct Parts {
    size_t o = 0;
    size_t part(size_t b) {
        const size_t at = o;
        o += (b + 15) / 16 * 16;
        return at;
    }
};

size_t padded(size_t n) { return (n + SB_BLOCK - 1) / SB_BLOCK * SB_BLOCK; }

// the signatures' block: state | status | vk | sig for n items (n_pad = n rounded up to the workgroup)
struct RsBlock {
    size_t n, n_pad, state, status, vk, sig, bytes;
    explicit RsBlock(size_t n_) : n(n_), n_pad(padded(n_)) {
        Parts p;
        state = p.part(sizeof(RsState) * n_pad);
        status = p.part(n_pad);
        vk = p.part(32 * n_pad);
        sig = p.part(64 * n_pad);
        bytes = p.o;
    }
    void point(RsArgs& a, uint8_t* base) const {
        a.state = (RsState*)(base + state);
        a.status = base + status;
        a.vks = (uint32_t*)(base + vk);
        a.sigs = (uint32_t*)(base + sig);
        a.n = (uint32_t)n;
    }
};

// the spends' block: state | status | cv | rk | nf | cmu | nk
struct SbBlock {
    size_t n, n_pad, state, status, cv, rk, nf, cmu, nk, bytes;
    explicit SbBlock(size_t n_) : n(n_), n_pad(padded(n_)) {
        Parts p;
        state = p.part(sizeof(SbState) * n_pad);
        status = p.part(n_pad);
        cv = p.part(32 * n_pad);
        rk = p.part(32 * n_pad);
        nf = p.part(32 * n_pad);
        cmu = p.part(32 * n_pad);
        nk = p.part(32 * n_pad);
        bytes = p.o;
    }
    void point(SbArgs& a, uint8_t* base) const {
        a.state = (SbState*)(base + state);
        a.status = base + status;
        a.cvs = (uint32_t*)(base + cv);
        a.rks = (uint32_t*)(base + rk);
        a.nfs = (uint32_t*)(base + nf);
        a.cmus = (uint32_t*)(base + cmu);
        a.nks = (uint32_t*)(base + nk);
        a.n = (uint32_t)n;
    }
};

// the eight lanes' shares folded in nf_fold's order, as lane 0 ends with them
template <class F>
JExt folded(F share) {
    JExt p[SB_LANES];
    for (int l = 0; l < SB_LANES; ++l) p[l] = share(l);
    for (int m = 1; m < SB_LANES; m <<= 1)
        for (int l = 0; l < SB_LANES; l += 2 * m) p[l] = jj_add(p[l], p[l + m]);
    return p[0];
}

RsTables host_tables() { return {{spend_table().data(), output_table().data()}}; }

// what kernel `stage` (1 key, 2 nonce_hash, 3 nonce_point, 4 finish) does, over the block
void rs_stage_host(int stage, const RsArgs& a) {
    for (uint32_t i = 0; i < a.n; ++i) {
        RsState& st = a.state[i];
        if (stage == 1) {
            rs_key(st, a.in, a.tab, i);
        } else if (stage == 4) {
            a.status[i] = (uint8_t)st.status;
            if (st.status == RS_OK) rs_finish(st, a.in, i, a.sigs + 16 * (size_t)i, a.vks + 8 * (size_t)i);
        } else if (st.status != RS_OK) {
            continue;
        } else if (stage == 2) {
            rs_nonce_hash(st, a.in, i);
        } else {
            rs_nonce_point(st, a.in, a.tab, i);
        }
    }
}

// what kernel `stage` (1 parse, 2 keys, 3 commit, 4 cv, 5 finish) does, over the block
void sb_stage_host(int stage, const SbArgs& a) {
    for (uint32_t i = 0; i < a.n; ++i) {
        SbState& st = a.state[i];
        if (stage == 1) {
            for (int y = 0; y < 3; ++y) sb_parse(st, a.in, i, y);
        } else if (stage == 2) {
            for (int y = 0; y < 3; ++y) sb_keys(st, a.in, a.sbt, i, y);
        } else if (stage == 3) {
            a.status[i] = sb_status(st);
            if (a.status[i] != SB_OK) continue;
            uint32_t cmu[8];
            nf_commit_finish(st.ob.nf, folded([&](int l) { return nf_commit_partial(st.ob.nf, a.ped, a.nft, l, SB_LANES); }), cmu);
            memcpy(a.cmus + 8 * (size_t)i, cmu, 32);
        } else if (a.status[i] != SB_OK) {
            continue;
        } else if (stage == 4) {
            uint32_t cv[8];
            ob_value_commitment(cv, st.ob, a.vcr, a.in.rcvs + 8 * (size_t)i);
            memcpy(a.cvs + 8 * (size_t)i, cv, 32);
            memcpy(a.rks + 8 * (size_t)i, st.rk, 32);
            memcpy(a.nks + 8 * (size_t)i, st.nk, 32);
        } else {
            uint32_t nf[8];
            nf_finish(nf, folded([&](int l) { return nf_rho_partial(st.ob.nf, a.nft + NF_NCR_TABLE, a.in.note.positions[i], l, SB_LANES); }), st.nk);
            memcpy(a.nfs + 8 * (size_t)i, nf, 32);
        }
    }
}

struct DevMem {
    std::vector<void*> all;
    ~DevMem() {
        for (void* p : all) (void)hipFree(p);
    }
    template <class T>
    T* put(const void* src, size_t bytes, bool& ok) {
        void* p = nullptr;
        ok = ok && hipMalloc(&p, bytes ? bytes : 1) == hipSuccess;
        if (ok) all.push_back(p);
        if (ok && src) ok = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && !src) ok = hipMemset(p, 0, bytes ? bytes : 1) == hipSuccess;
        return (T*)p;
    }
};

}  // namespace

extern "C" {

size_t sbd_sign_block_bytes(uint32_t n) { return RsBlock(n).bytes; }
// where a block's parts start: state, status, vk, sig, and sizeof(RsState), n_pad
void sbd_sign_block_layout(uint32_t n, uint64_t out[6]) {
    const RsBlock b(n);
    const uint64_t v[6] = {b.state, b.status, b.vk, b.sig, sizeof(RsState), b.n_pad};
    memcpy(out, v, sizeof v);
}
size_t sbd_spend_block_bytes(uint32_t n) { return SbBlock(n).bytes; }
// state, status, cv, rk, nf, cmu, nk, and sizeof(SbState), n_pad
void sbd_spend_block_layout(uint32_t n, uint64_t out[9]) {
    const SbBlock b(n);
    const uint64_t v[9] = {b.state, b.status, b.cv, b.rk, b.nf, b.cmu, b.nk, sizeof(SbState), b.n_pad};
    memcpy(out, v, sizeof v);
}

// [k] G from the fixed-base table `which` (0 G_spend, 1 G_pgk, 2 G_vcr; 63 windows: k below 2^252) -> the point's encoding
int sbd_table_mul_host(int which, const uint8_t k32[32], uint8_t out32[32]) {
    if (which < 0 || which > 2) return -1;
    uint32_t k[8], w[8];
    memcpy(k, k32, 32);
    const JNiels* t = which == 2 ? output_table().data() : spend_table().data() + (which == 1 ? SB_BASE_TABLE : 0);
    jj_encode(w, fixed_base_mul(t, k));
    memcpy(out32, w, 32);
    return 0;
}

// rj_reduce_wide: the 64 little-endian bytes mod r_J
void sbd_reduce_wide_host(const uint8_t in64[64], uint8_t out32[32]) {
    uint32_t in[16], out[8];
    memcpy(in, in64, 64);
    rj_reduce_wide(out, in);
    memcpy(out32, out, 32);
}

// rj_mul_add: r + c k mod r_J
void sbd_mul_add_host(const uint8_t r32[32], const uint8_t c32[32], const uint8_t k32[32], uint8_t out32[32]) {
    uint32_t r[8], c[8], k[8], out[8];
    memcpy(r, r32, 32);
    memcpy(c, c32, 32);
    memcpy(k, k32, 32);
    rj_mul_add(out, r, c, k);
    memcpy(out32, out, 32);
}

// stage 1..4 of the signing steps on the host over `block` (sbd_sign_block_bytes(n) bytes, in place); stage 0: all four
int sbd_sign_stage_host(int stage, uint32_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes, const uint8_t* kinds,
                        const uint8_t* randoms, uint8_t* block) {
    if (stage < 0 || stage > 4) return -1;
    const std::vector<uint32_t> sk = words(sks, 32 * (size_t)n), al = words(alphas, 32 * (size_t)n), sh = words(sighashes, 32 * (size_t)n),
                                rnd = words(randoms, 80 * (size_t)n);
    RsArgs a;
    a.in = {sk.data(), alphas ? al.data() : nullptr, sh.data(), kinds, rnd.data()};
    a.tab = host_tables();
    RsBlock(n).point(a, block);
    for (int s = stage ? stage : 1; s <= (stage ? stage : 4); ++s) rs_stage_host(s, a);
    return 0;
}

// the product's kernel `stage` alone (1..4), or all four in the product's order (0), over `block` on the GPU: uploaded, run on the null
// stream, downloaded in place.  n >= 1.
int sbd_sign_stage_gpu(int stage, uint32_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes, const uint8_t* kinds,
                       const uint8_t* randoms, uint8_t* block) {
    if (n == 0 || stage < 0 || stage > 4) return -1;
    const std::vector<JNiels>&sbt = spend_table(), &vcr = output_table();
    const RsBlock b(n);
    DevMem m;
    bool ok = true;
    RsArgs a;
    a.in.sks = m.put<uint32_t>(sks, 32 * (size_t)n, ok);
    a.in.alphas = alphas ? m.put<uint32_t>(alphas, 32 * (size_t)n, ok) : nullptr;
    a.in.sighashes = m.put<uint32_t>(sighashes, 32 * (size_t)n, ok);
    a.in.kinds = m.put<uint8_t>(kinds, n, ok);
    a.in.randoms = m.put<uint32_t>(randoms, 80 * (size_t)n, ok);
    a.tab.base[0] = m.put<JNiels>(sbt.data(), sizeof(JNiels) * sbt.size(), ok);
    a.tab.base[1] = m.put<JNiels>(vcr.data(), sizeof(JNiels) * vcr.size(), ok);
    uint8_t* d_block = m.put<uint8_t>(block, b.bytes, ok);
    if (!ok) return -2;
    b.point(a, d_block);
    launch_error().clear();
    const uint32_t nb = (n + SB_BLOCK - 1) / SB_BLOCK;
    switch (stage) {
        case 0: rs_enqueue(nullptr, a); break;
        case 1: MASP_LAUNCH(k_rs_key, dim3(nb), dim3(SB_BLOCK), 0, nullptr, a); break;
        case 2: MASP_LAUNCH(k_rs_nonce_hash, dim3(nb), dim3(SB_BLOCK), 0, nullptr, a); break;
        case 3: MASP_LAUNCH(k_rs_nonce_point, dim3(nb), dim3(SB_BLOCK), 0, nullptr, a); break;
        default: MASP_LAUNCH(k_rs_finish, dim3(nb), dim3(SB_BLOCK), 0, nullptr, a); break;
    }
    if (!launch_error().empty() || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(block, d_block, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}

// stage 1..5 of the spend steps on the host over `block` (sbd_spend_block_bytes(n) bytes, in place); stage 0: all five
int sbd_spend_stage_host(int stage, uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds,
                         const uint8_t* leads, const uint8_t* rseeds, const uint8_t* aks, const uint8_t* nsks, const uint8_t* ars,
                         const uint8_t* rcvs, const uint64_t* positions, uint8_t* block) {
    if (stage < 0 || stage > 5) return -1;
    const std::vector<uint32_t> id = words(ids, 32 * (size_t)n), pk = words(pk_ds, 32 * (size_t)n), rs = words(rseeds, 32 * (size_t)n),
                                ak = words(aks, 32 * (size_t)n), nsk = words(nsks, 32 * (size_t)n), ar = words(ars, 32 * (size_t)n),
                                rcv = words(rcvs, 32 * (size_t)n);
    std::vector<uint64_t> val(n + 1), pos(n + 1);
    memcpy(val.data(), values, 8 * (size_t)n);
    memcpy(pos.data(), positions, 8 * (size_t)n);
    SbArgs a;
    a.in.note = {id.data(), val.data(), divs, pk.data(), leads, rs.data(), nullptr, pos.data()};
    a.in.aks = ak.data();
    a.in.nsks = nsk.data();
    a.in.ars = ar.data();
    a.in.rcvs = rcv.data();
    a.ped = (const JNiels*)pedersen_table_bytes().data();
    a.nft = nullifier_table().data();
    a.vcr = output_table().data();
    a.sbt = spend_table().data();
    SbBlock(n).point(a, block);
    for (int s = stage ? stage : 1; s <= (stage ? stage : 5); ++s) sb_stage_host(s, a);
    return 0;
}

int sbd_spend_stage_gpu(int stage, uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds,
                        const uint8_t* leads, const uint8_t* rseeds, const uint8_t* aks, const uint8_t* nsks, const uint8_t* ars,
                        const uint8_t* rcvs, const uint64_t* positions, uint8_t* block) {
    if (n == 0 || stage < 0 || stage > 5) return -1;
    const std::vector<uint8_t>& ped = pedersen_table_bytes();
    const std::vector<JNiels>&nft = nullifier_table(), &vcr = output_table(), &sbt = spend_table();
    const SbBlock b(n);
    DevMem m;
    bool ok = true;
    SbArgs a;
    a.in.note.ids = m.put<uint32_t>(ids, 32 * (size_t)n, ok);
    a.in.note.values = m.put<uint64_t>(values, 8 * (size_t)n, ok);
    a.in.note.diversifiers = m.put<uint8_t>(divs, 11 * (size_t)n, ok);
    a.in.note.pk_ds = m.put<uint32_t>(pk_ds, 32 * (size_t)n, ok);
    a.in.note.leads = m.put<uint8_t>(leads, n, ok);
    a.in.note.rseeds = m.put<uint32_t>(rseeds, 32 * (size_t)n, ok);
    a.in.note.nks = nullptr;
    a.in.note.positions = m.put<uint64_t>(positions, 8 * (size_t)n, ok);
    a.in.aks = m.put<uint32_t>(aks, 32 * (size_t)n, ok);
    a.in.nsks = m.put<uint32_t>(nsks, 32 * (size_t)n, ok);
    a.in.ars = m.put<uint32_t>(ars, 32 * (size_t)n, ok);
    a.in.rcvs = m.put<uint32_t>(rcvs, 32 * (size_t)n, ok);
    a.ped = m.put<JNiels>(ped.data(), ped.size(), ok);
    a.nft = m.put<JNiels>(nft.data(), sizeof(JNiels) * nft.size(), ok);
    a.vcr = m.put<JNiels>(vcr.data(), sizeof(JNiels) * vcr.size(), ok);
    a.sbt = m.put<JNiels>(sbt.data(), sizeof(JNiels) * sbt.size(), ok);
    uint8_t* d_block = m.put<uint8_t>(block, b.bytes, ok);
    if (!ok) return -2;
    b.point(a, d_block);
    launch_error().clear();
    const uint32_t nb = (n + SB_BLOCK - 1) / SB_BLOCK, nb8 = (n * SB_LANES + SB_BLOCK - 1) / SB_BLOCK;
    switch (stage) {
        case 0: sb_enqueue(nullptr, a); break;
        case 1: MASP_LAUNCH(k_sb_parse, dim3(nb, 3), dim3(SB_BLOCK), 0, nullptr, a); break;
        case 2: MASP_LAUNCH(k_sb_keys, dim3(nb, 3), dim3(SB_BLOCK), 0, nullptr, a); break;
        case 3: MASP_LAUNCH(k_sb_commit, dim3(nb8), dim3(SB_BLOCK), 0, nullptr, a); break;
        case 4: MASP_LAUNCH(k_sb_cv, dim3(nb), dim3(SB_BLOCK), 0, nullptr, a); break;
        default: MASP_LAUNCH(k_sb_finish, dim3(nb8), dim3(SB_BLOCK), 0, nullptr, a); break;
    }
    if (!launch_error().empty() || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(block, d_block, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}

}  // extern "C"
