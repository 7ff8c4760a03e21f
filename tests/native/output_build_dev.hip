// Test-only shim over the output descriptions' device code: masp_amd/csrc/device/output_build.hpp on the host (the header is __host__
// __device__), stage by stage over one block of memory that holds everything the kernels hand each other, and the product's own kernels
// (masp_amd/csrc/k_output_build.hip, its kernel half) on the GPU over the same block, one kernel alone or all of them, without a context.
// The tables are the product's (output_table.h, nullifier_table.h, pedersen_table.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#define MASP_OB_KERNELS_ONLY
#include "../../masp_amd/csrc/k_output_build.hip"
#include "../../masp_amd/csrc/output_table.h"

using namespace masp;

namespace {

// the twelve arrays as they come, copied where the device code reads words
struct Inputs {
    std::vector<uint32_t> ids, pk_ds, rseeds, esks, rcvs, ovks, randoms;
    std::vector<uint64_t> values;
    const uint8_t *divs, *leads, *flags;
    bool have_esks, have_randoms;
    static void put(std::vector<uint32_t>& v, const uint8_t* src, size_t bytes) {
        v.assign(bytes / 4 + 1, 0);
        if (src) memcpy(v.data(), src, bytes);
    }
    Inputs(size_t n, const uint8_t* ids_, const uint64_t* values_, const uint8_t* divs_, const uint8_t* pk_ds_, const uint8_t* leads_,
           const uint8_t* rseeds_, const uint8_t* esks_, const uint8_t* rcvs_, const uint8_t* ovks_, const uint8_t* flags_, const uint8_t* randoms_)
        : values(n + 1), divs(divs_), leads(leads_), flags(flags_), have_esks(esks_ != nullptr), have_randoms(randoms_ != nullptr) {
        put(ids, ids_, 32 * n);
        put(pk_ds, pk_ds_, 32 * n);
        put(rseeds, rseeds_, 32 * n);
        put(esks, esks_, 32 * n);
        put(rcvs, rcvs_, 32 * n);
        put(ovks, ovks_, 32 * n);
        put(randoms, randoms_, 96 * n);
        memcpy(values.data(), values_, 8 * n);
    }
    ObIn in() const {
        return {ids.data(), values.data(), divs,  pk_ds.data(), leads, rseeds.data(), have_esks ? esks.data() : nullptr, rcvs.data(), ovks.data(),
                flags,      have_randoms ? randoms.data() : nullptr};
    }
};

// The block: state | status | cv | cmu | epk | memo columns | ciphertext columns | enc rows | cout rows, for n outputs (n_pad = n rounded up
// to the workgroup).  Every part starts on a multiple of 16 bytes.
struct Block {
    size_t n, n_pad, state, status, cv, cmu, epk, memo, cols, enc, cout, bytes;
    explicit Block(size_t n_) : n(n_), n_pad((n_ + OB_BLOCK - 1) / OB_BLOCK * OB_BLOCK) {
        size_t o = 0;
        auto part = [&](size_t b) {
            const size_t at = o;
            o += (b + 15) / 16 * 16;
            return at;
        };
        state = part(sizeof(ObState) * n_pad);
        status = part(n_pad);
        cv = part(32 * n_pad);
        cmu = part(32 * n_pad);
        epk = part(32 * n_pad);
        memo = part(512 * n_pad);
        cols = part(16 * (size_t)OB_COLS * n_pad);
        enc = part(612 * n_pad);
        cout = part(80 * n_pad);
        bytes = o;
    }
    void point(ObArgs& a, uint8_t* base) const {
        a.state = (ObState*)(base + state);
        a.status = base + status;
        a.cvs = (uint32_t*)(base + cv);
        a.cmus = (uint32_t*)(base + cmu);
        a.epks = (uint32_t*)(base + epk);
        a.memo_cols = (uint4*)(base + memo);
        a.cols = (uint4*)(base + cols);
        a.encs = (uint32_t*)(base + enc);
        a.couts = (uint32_t*)(base + cout);
        a.n = (uint32_t)n;
        a.n_pad = (uint32_t)n_pad;
    }
};

// k_ob_commit's sum on the host: the eight lanes' shares folded in nf_fold's order, as lane 0 ends with them
JExt commit_sum(const ObState& st, const JNiels* ped, const JNiels* ncr) {
    JExt p[OB_LANES];
    for (int l = 0; l < OB_LANES; ++l) p[l] = nf_commit_partial(st.nf, ped, ncr, l, OB_LANES);
    for (int m = 1; m < OB_LANES; m <<= 1)
        for (int l = 0; l < OB_LANES; l += 2 * m) p[l] = jj_add(p[l], p[l + m]);
    return p[0];
}

// what kernel `stage` (1 parse, 2 memo, 3 commit, 4 cv, 5 ladder, 6 seal, 7 rows) does, over the block
void stage_host(int stage, const ObArgs& a, const uint4* memo_rows) {
    const JNiels* ped = (const JNiels*)pedersen_table_bytes().data();
    const JNiels* ncr = nullifier_table().data();
    const JNiels* vcr = output_table().data();
    for (uint32_t i = 0; i < a.n; ++i) {
        ObState& st = a.state[i];
        if (stage == 1) {
            for (int y = 0; y < 4; ++y) ob_parse(st, a.in, i, y);
        } else if (stage == 2) {
            if (memo_rows)
                for (uint32_t c = 0; c < OB_MEMO_COLS; ++c) a.memo_cols[(size_t)c * a.n_pad + i] = memo_rows[(size_t)i * OB_MEMO_COLS + c];
        } else if (stage == 3) {
            a.status[i] = ob_status(st);
            if (a.status[i] != OB_OK) continue;
            uint32_t cmu[8];
            nf_commit_finish(st.nf, commit_sum(st, ped, ncr), cmu);
            memcpy(a.cmus + 8 * (size_t)i, cmu, 32);
        } else if (a.status[i] != OB_OK) {
            continue;
        } else if (stage == 4) {
            uint32_t cv[8];
            ob_value_commitment(cv, st, vcr, a.in.rcvs + 8 * (size_t)i);
            memcpy(a.cvs + 8 * (size_t)i, cv, 32);
        } else if (stage == 5) {
            ob_ladder(st, a.epks + 8 * (size_t)i, 0);
            ob_ladder(st, a.epks + 8 * (size_t)i, 1);
        } else if (stage == 6) {
            ob_seal(st, a.in, i, a.cvs + 8 * (size_t)i, a.cmus + 8 * (size_t)i, a.epks + 8 * (size_t)i, memo_rows ? a.memo_cols + i : nullptr, a.n_pad,
                    a.cols + i, a.n_pad);
        } else if (stage == 7) {
            const uint32_t* cols = (const uint32_t*)a.cols;
            for (uint32_t w = 0; w < OB_ENC_WORDS; ++w) a.encs[(size_t)i * OB_ENC_WORDS + w] = cols[4 * ((size_t)(w >> 2) * a.n_pad + i) + (w & 3u)];
            for (uint32_t v = 0; v < OB_OUT_WORDS; ++v)
                a.couts[(size_t)i * OB_OUT_WORDS + v] = cols[4 * ((size_t)(OB_ENC_COLS + (v >> 2)) * a.n_pad + i) + (v & 3u)];
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

size_t obd_block_bytes(uint32_t n) { return Block(n).bytes; }

// where a block's parts start: state, status, cv, cmu, epk, memo columns, ciphertext columns, enc rows, cout rows, and sizeof(ObState), n_pad
void obd_block_layout(uint32_t n, uint64_t out[11]) {
    const Block b(n);
    const uint64_t v[11] = {b.state, b.status, b.cv, b.cmu, b.epk, b.memo, b.cols, b.enc, b.cout, sizeof(ObState), b.n_pad};
    memcpy(out, v, sizeof v);
}

// [k] G_vcr from the fixed-base table (63 windows: k below 2^252) -> the point's encoding
int obd_table_mul_host(const uint8_t k32[32], uint8_t out32[32]) {
    uint32_t k[8], w[8];
    memcpy(k, k32, 32);
    jj_encode(w, nf_table_sum(jj_identity(), output_table().data(), OB_VCR_WINDOWS, k, 0, 1));
    memcpy(out32, w, 32);
    return 0;
}

// the seal step alone, from K_enc on: pt596 the note plaintext (its memo read as columns; use_memo = 0: the empty memo is made up instead and
// pt596's memo is not read), then out_ciphertext from ovk, cv, cmu, epk, pk_d, esk (have_ovk) or from random96
int obd_seal_host(const uint8_t key32[32], const uint8_t pt596[596], int use_memo, int have_ovk, const uint8_t ovk[32], const uint8_t cv[32],
                  const uint8_t cmu[32], const uint8_t epk[32], const uint8_t pk_d[32], const uint8_t esk[32], const uint8_t* random96,
                  uint8_t enc612[612], uint8_t cout80[80]) {
    uint32_t key[8], hdr[21], w[6][8], rnd[24] = {0};
    uint4 memo[OB_MEMO_COLS], cols[OB_COLS];
    memcpy(key, key32, 32);
    memcpy(hdr, pt596, 84);
    memcpy(memo, pt596 + 84, 512);
    const uint8_t* src[6] = {ovk, cv, cmu, epk, pk_d, esk};
    for (int i = 0; i < 6; ++i) memcpy(w[i], src[i], 32);
    if (random96) memcpy(rnd, random96, 96);
    if (!have_ovk && !random96) return -1;
    ob_seal_enc(key, hdr, use_memo ? memo : nullptr, 1, cols, 1);
    ob_seal_out(have_ovk != 0, w[0], w[1], w[2], w[3], w[4], w[5], rnd, cols + OB_ENC_COLS, 1);
    memcpy(enc612, cols, 612);
    memcpy(cout80, cols + OB_ENC_COLS, 80);
    return 0;
}

// stage 1..7 of device/output_build.hpp's steps on the host over `block` (obd_block_bytes(n) bytes, in place); stage 0: all seven
int obd_stage_host(int stage, uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds, const uint8_t* leads,
                   const uint8_t* rseeds, const uint8_t* esks, const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* flags,
                   const uint8_t* randoms, uint8_t* block) {
    if (stage < 0 || stage > 7) return -1;
    const Inputs I(n, ids, values, divs, pk_ds, leads, rseeds, esks, rcvs, ovks, flags, randoms);
    std::vector<uint4> memo_rows(memos ? (size_t)n * OB_MEMO_COLS : 0);
    if (memos) memcpy((void*)memo_rows.data(), memos, 512 * (size_t)n);
    ObArgs a;
    a.in = I.in();
    Block(n).point(a, block);
    for (int s = stage ? stage : 1; s <= (stage ? stage : 7); ++s) stage_host(s, a, memos ? memo_rows.data() : nullptr);
    return 0;
}

// the product's kernel `stage` alone (1..7), or all seven in the product's order (0), over `block` on the GPU: uploaded, run on the null
// stream, downloaded in place.  n >= 1.
int obd_stage_gpu(int stage, uint32_t n, const uint8_t* ids, const uint64_t* values, const uint8_t* divs, const uint8_t* pk_ds, const uint8_t* leads,
                  const uint8_t* rseeds, const uint8_t* esks, const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* flags,
                  const uint8_t* randoms, uint8_t* block) {
    if (n == 0 || stage < 0 || stage > 7) return -1;
    const std::vector<uint8_t>& ped = pedersen_table_bytes();
    const std::vector<JNiels>& ncr = nullifier_table();
    const std::vector<JNiels>& vcr = output_table();
    const Block b(n);
    DevMem m;
    bool ok = true;
    ObArgs a;
    a.in.ids = m.put<uint32_t>(ids, 32 * (size_t)n, ok);
    a.in.values = m.put<uint64_t>(values, 8 * (size_t)n, ok);
    a.in.diversifiers = m.put<uint8_t>(divs, 11 * (size_t)n, ok);
    a.in.pk_ds = m.put<uint32_t>(pk_ds, 32 * (size_t)n, ok);
    a.in.leads = m.put<uint8_t>(leads, n, ok);
    a.in.rseeds = m.put<uint32_t>(rseeds, 32 * (size_t)n, ok);
    a.in.esks = esks ? m.put<uint32_t>(esks, 32 * (size_t)n, ok) : nullptr;
    a.in.rcvs = m.put<uint32_t>(rcvs, 32 * (size_t)n, ok);
    a.in.ovks = m.put<uint32_t>(ovks, 32 * (size_t)n, ok);
    a.in.ovk_flags = flags ? m.put<uint8_t>(flags, n, ok) : nullptr;
    a.in.out_randoms = randoms ? m.put<uint32_t>(randoms, 96 * (size_t)n, ok) : nullptr;
    a.memo_rows = memos ? m.put<uint4>(memos, 512 * (size_t)n, ok) : nullptr;
    a.ped = m.put<JNiels>(ped.data(), ped.size(), ok);
    a.ncr = m.put<JNiels>(ncr.data(), sizeof(JNiels) * ncr.size(), ok);
    a.vcr = m.put<JNiels>(vcr.data(), sizeof(JNiels) * vcr.size(), ok);
    uint8_t* d_block = m.put<uint8_t>(block, b.bytes, ok);
    if (!ok) return -2;
    b.point(a, d_block);
    launch_error().clear();
    const uint32_t nb = (n + OB_BLOCK - 1) / OB_BLOCK;
    switch (stage) {
        case 0: ob_enqueue(nullptr, a); break;
        case 1: MASP_LAUNCH(k_ob_parse, dim3(nb, 4), dim3(OB_BLOCK), 0, nullptr, a); break;
        case 2:
            if (a.memo_rows) MASP_LAUNCH(k_ob_memo, dim3(nb, OB_MEMO_COLS), dim3(OB_BLOCK), 0, nullptr, a);
            break;
        case 3: MASP_LAUNCH(k_ob_commit, dim3((n * OB_LANES + OB_BLOCK - 1) / OB_BLOCK), dim3(OB_BLOCK), 0, nullptr, a); break;
        case 4: MASP_LAUNCH(k_ob_cv, dim3(nb), dim3(OB_BLOCK), 0, nullptr, a); break;
        case 5: MASP_LAUNCH(k_ob_ladder, dim3(nb, 2), dim3(OB_BLOCK), 0, nullptr, a); break;
        case 6: MASP_LAUNCH(k_ob_seal, dim3(nb), dim3(OB_BLOCK), 0, nullptr, a); break;
        default: MASP_LAUNCH(k_ob_rows, dim3((uint32_t)(((uint64_t)n * (OB_ENC_WORDS + OB_OUT_WORDS) + 255) / 256)), dim3(256), 0, nullptr, a); break;
    }
    if (!launch_error().empty() || hipDeviceSynchronize() != hipSuccess) return -3;
    if (hipMemcpy(block, d_block, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}

}  // extern "C"
