// Test-only shim over masp_amd/csrc/device/merkle.hpp: its functions on the host (the header is __host__ __device__), with the table
// the product builds (masp_amd/csrc/pedersen_table.h builds the same from the same host windows).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../masp_amd/csrc/device/merkle.hpp"
#include "../../masp_amd/csrc/host/jubjub.h"

using namespace masp;

namespace {

uint32_t ld32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

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

// the head of the Niels table that a Merkle hash reads, [segment][window][k] in chunk order
const std::vector<JNiels>& table() {
    static const std::vector<JNiels> t = [] {
        std::vector<JNiels> n(MT_TABLE);
        const masp_host::PedersenWindows& W = masp_host::pedersen_windows();
        for (uint32_t c = 0; c < MT_CHUNKS; ++c)
            for (uint32_t k = 0; k < 4; ++k) {
                const masp_host::JPoint::Niels& e = W.e[c / PED_WINDOWS][c % PED_WINDOWS][k];
                n[4 * c + k] = {fr_of_host(e.vmu), fr_of_host(e.vpu), fr_of_host(e.t2d)};
            }
        return n;
    }();
    return t;
}

}  // namespace

extern "C" {

// n items of (level u32 | lhs 32 | rhs 32) at 68-byte pitch -> n x 32 bytes
int mkl_combine_host(const uint8_t* items, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* it = items + 68 * (size_t)i;
        uint32_t l[8], r[8], o[8];
        for (int k = 0; k < 8; ++k) {
            l[k] = ld32(it + 4 + 4 * k);
            r[k] = ld32(it + 36 + 4 * k);
        }
        merkle_combine(o, table().data(), ld32(it), l, r);
        memcpy(out + 32 * (size_t)i, o, 32);
    }
    return 0;
}

// n x 32 bytes -> n flags
int mkl_is_canonical_host(const uint8_t* nodes, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t w[8];
        for (int k = 0; k < 8; ++k) w[k] = ld32(nodes + 32 * (size_t)i + 4 * k);
        out[i] = fr_is_canonical(w) ? 1 : 0;
    }
    return 0;
}

// start and unpadded width of row i of the node vector over n nodes
void mkl_row_host(uint64_t n, uint32_t i, uint64_t* start, uint64_t* width) { mt_row(n, i, *start, *width); }

}  // extern "C"
