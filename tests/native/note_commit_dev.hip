// Test-only shim over the device headers of the compact note scan (masp_amd/csrc/device/blake2s.hpp, group_hash.hpp, pedersen.hpp): each
// function on the host (the headers are __host__ __device__) and, with the _gpu suffix, the same code in a kernel, one item per lane.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/device/compact_note.hpp"
#include "../../masp_amd/csrc/host/jubjub.h"

using namespace masp;

namespace {

constexpr uint32_t STRIDE = 160;   // bytes per slot: 32 head | 128 message

__host__ __device__ uint32_t ld32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
__host__ __device__ void st32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// op 0: BLAKE2s-256 (personal = slot[0..8), message slot[32 .. 32 + len), len <= 128) -> 32 bytes
// op 1: the group hash "MASP__gd" of the diversifier slot[32..43) -> the cleared point's encoding, out[32] = 1 if it exists
// op 2: the asset generator of the identifier slot[32..64) -> the point's encoding, out[32] = 1 if it exists, out[33] = 1 if the digest
//       the function hands out equals that encoding
// op 3: cmu of (asset identifier 32 | value 8 | diversifier 11, a pad byte | pk_d 32 | rcm 32) at slot[32..148), built as k_nsc_parse and
//       k_nsc_commit build it -> 32 bytes, out[32] = 1 if the identifier and the diversifier have their points
// op 4: the 512-bit integer slot[32..96) mod r_J -> 32 bytes
// op 5: PRF^expand(rseed = slot[32..64), [slot[0]]) mod r_J -> 32 bytes
// op 6: stage 2 of the compact scan for one candidate, the four steps the kernels run (device/compact_note.hpp): lead byte slot[0], key
//       slot[32..64), ivk slot[64..96), epk slot[96..128), cmu slot[128..160), the 84 ciphertext bytes at `extra` -> out[0] = the number of
//       steps that passed (4: a note; lead byte 1 has no fourth step and counts it as passed), out[1..33) pk_d when it got that far
__host__ __device__ void run_one(int op, const uint8_t* slot, uint32_t len, const JNiels* table, const uint8_t* extra, uint8_t* out) {
    const uint8_t* msg = slot + 32;
    if (op == 6) {
        uint32_t key[8], ivk[8], epk[8], cmu[8], row[NSC_ENC_WORDS];
        for (int i = 0; i < 8; ++i) {
            key[i] = ld32(slot + 32 + 4 * i);
            ivk[i] = ld32(slot + 64 + 4 * i);
            epk[i] = ld32(slot + 96 + 4 * i);
            cmu[i] = ld32(slot + 128 + 4 * i);
        }
        for (uint32_t i = 0; i < NSC_ENC_WORDS; ++i) row[i] = ld32(extra + 4 * i);
        const int lead = slot[0];
        NscState st;
        if (!nsc_parse(st, key, row, lead)) return;
        out[0] = 1;
        if (!nsc_pkd(st, ivk)) return;
        out[0] = 2;
        for (int i = 0; i < 8; ++i) st32(out + 1 + 4 * i, st.msg[18 + i]);
        if (!nsc_commit(st, table, cmu, lead)) return;
        out[0] = 3;
        if (lead == 2 && !nsc_esk(st, epk)) return;
        out[0] = 4;
    } else if (op == 0) {
        uint32_t m[32], h[8];
        for (int i = 0; i < 32; ++i) {
            m[i] = 0;
            for (int b = 3; b >= 0; --b) m[i] = (m[i] << 8) | ((uint32_t)(4 * i + b) < len ? msg[4 * i + b] : 0);
        }
        blake2s_256(h, m, len, ld32(slot), ld32(slot + 4));
        for (int i = 0; i < 8; ++i) st32(out + 4 * i, h[i]);
    } else if (op == 1) {
        const uint32_t d[3] = {ld32(msg), ld32(msg + 4), ld32(msg + 8)};
        JExt p;
        if (!jj_group_hash_gd(p, d)) return;
        uint32_t w[8];
        jj_encode(w, p);
        for (int i = 0; i < 8; ++i) st32(out + 4 * i, w[i]);
        out[32] = 1;
    } else if (op == 2) {
        uint32_t id[8], dg[8], w[8];
        for (int i = 0; i < 8; ++i) id[i] = ld32(msg + 4 * i);
        JExt p;
        if (!jj_asset_generator(p, dg, id)) return;
        jj_encode(w, p);
        bool same = true;
        for (int i = 0; i < 8; ++i) {
            st32(out + 4 * i, w[i]);
            same = same && w[i] == dg[i];
        }
        out[32] = 1;
        out[33] = same;
    } else if (op == 3) {
        uint32_t id[8], m[PED_NC_MSG_WORDS], rcm[8], cmu[8];
        for (int i = 0; i < 8; ++i) id[i] = ld32(msg + 4 * i);
        JExt p;
        if (!jj_asset_generator(p, m, id)) return;
        m[8] = ld32(msg + 32);
        m[9] = ld32(msg + 36);
        const uint32_t d[3] = {ld32(msg + 40), ld32(msg + 44), ld32(msg + 48)};
        if (!jj_group_hash_gd(p, d)) return;
        jj_encode(m + 10, p);
        for (int i = 0; i < 8; ++i) m[18 + i] = ld32(msg + 52 + 4 * i);
        for (int i = 0; i < 8; ++i) rcm[i] = ld32(msg + 84 + 4 * i);
        const JExt g_ncr = *(const JExt*)(table + PED_NC_TABLE);
        note_commit_u(cmu, table, g_ncr, m, rcm);
        for (int i = 0; i < 8; ++i) st32(out + 4 * i, cmu[i]);
        out[32] = 1;
    } else if (op == 4) {
        uint32_t in[16], r[8];
        for (int i = 0; i < 16; ++i) in[i] = ld32(msg + 4 * i);
        rj_from_bytes_wide(r, in);
        for (int i = 0; i < 8; ++i) st32(out + 4 * i, r[i]);
    } else {
        uint32_t rs[8], r[8];
        for (int i = 0; i < 8; ++i) rs[i] = ld32(msg + 4 * i);
        rseed_scalar(r, rs, slot[0]);
        for (int i = 0; i < 8; ++i) st32(out + 4 * i, r[i]);
    }
}

__global__ void k_run(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, const JNiels* table, const uint8_t* extra, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) run_one(op, slots + (size_t)STRIDE * i, lens[i], table, extra + 84 * (size_t)i, out + 64 * (size_t)i);
}

Fr fr_of_host(const masp_host::Fr& x) {
    uint64_t c[4];
    x.to_canonical(c);
    Fr r;
    for (int i = 0; i < 4; ++i) {
        r.v[2 * i] = (uint32_t)c[i];
        r.v[2 * i + 1] = (uint32_t)(c[i] >> 32);
    }
    return fe_to_mont(r);
}

// the table as the product builds it (k_note_scan_compact.hip): the Niels points [segment][window][k], then G_ncr
const std::vector<uint8_t>& table_bytes() {
    static const std::vector<uint8_t> t = [] {
        std::vector<uint8_t> b(sizeof(JNiels) * PED_NC_TABLE + sizeof(JExt));
        const masp_host::PedersenWindows& W = masp_host::pedersen_windows();
        JNiels* n = (JNiels*)b.data();
        for (uint32_t s = 0; s < PED_NC_SEGMENTS; ++s)
            for (uint32_t w = 0; w < PED_WINDOWS; ++w)
                for (uint32_t k = 0; k < 4; ++k) {
                    const masp_host::JPoint::Niels& e = W.e[s][w][k];
                    n[(s * PED_WINDOWS + w) * 4 + k] = {fr_of_host(e.vmu), fr_of_host(e.vpu), fr_of_host(e.t2d)};
                }
        const masp_host::JAffine g = masp_host::generators().note_commitment_randomness.to_affine();
        const Fr u = fr_of_host(g.u), v = fr_of_host(g.v);
        const JExt ge = {u, v, fe_one<FrCfg>(), fe_mul(u, v)};
        memcpy(b.data() + sizeof(JNiels) * PED_NC_TABLE, &ge, sizeof(JExt));
        return b;
    }();
    return t;
}

}  // namespace

extern "C" {

// n slots of 160 bytes, lens[n] (<= 128), extra n x 84 (read by op 6 only), out n x 64 (zeroed here)
int ncm_run_host(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, const uint8_t* extra, uint8_t* out) {
    if (op < 0 || op > 6) return -1;
    memset(out, 0, 64 * (size_t)n);
    const JNiels* table = (const JNiels*)table_bytes().data();
    for (uint32_t i = 0; i < n; ++i) {
        if (lens[i] > 128) return -1;
        run_one(op, slots + (size_t)STRIDE * i, lens[i], table, extra + 84 * (size_t)i, out + 64 * (size_t)i);
    }
    return 0;
}

int ncm_run_gpu(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, const uint8_t* extra, uint8_t* out) {
    if (op < 0 || op > 6 || n == 0) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (lens[i] > 128) return -1;
    const std::vector<uint8_t>& tb = table_bytes();
    uint8_t *d_slots = nullptr, *d_out = nullptr, *d_table = nullptr, *d_extra = nullptr;
    uint32_t* d_lens = nullptr;
    int rc = -2;
    if (hipMalloc(&d_slots, (size_t)STRIDE * n) == hipSuccess && hipMalloc(&d_lens, 4 * (size_t)n) == hipSuccess &&
        hipMalloc(&d_out, 64 * (size_t)n) == hipSuccess && hipMalloc(&d_table, tb.size()) == hipSuccess &&
        hipMalloc(&d_extra, 84 * (size_t)n) == hipSuccess && hipMemcpy(d_extra, extra, 84 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_slots, slots, (size_t)STRIDE * n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_lens, lens, 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_table, tb.data(), tb.size(), hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_out, 0, 64 * (size_t)n) == hipSuccess) {
        hipLaunchKernelGGL(k_run, dim3((n + 63) / 64), dim3(64), 0, 0, op, d_slots, d_lens, n, (const JNiels*)d_table, d_extra, d_out);
        if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(out, d_out, 64 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    (void)hipFree(d_slots);
    (void)hipFree(d_lens);
    (void)hipFree(d_out);
    (void)hipFree(d_table);
    (void)hipFree(d_extra);
    return rc;
}

}  // extern "C"
