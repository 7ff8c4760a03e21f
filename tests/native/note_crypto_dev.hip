// Test-only shim over the device headers of the note scan (masp_amd/csrc/device/blake2b.hpp, chacha20.hpp, poly1305.hpp): each function
// on the host (the headers are __host__ __device__) and, with the _gpu suffix, the same code in a kernel, one message per lane.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../masp_amd/csrc/device/blake2b.hpp"
#include "../../masp_amd/csrc/device/chacha20.hpp"
#include "../../masp_amd/csrc/device/poly1305.hpp"

using namespace masp;

namespace {

constexpr uint32_t STRIDE = 160;   // bytes per message slot: 32 key | 128 message (Poly1305, BLAKE2b) or 32 key | 4 counter | 12 nonce (ChaCha20)

__host__ __device__ uint32_t ld32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
__host__ __device__ void st32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// op 0: BLAKE2b (personal = slot[0..16), outlen = slot[16], message slot[32 .. 32 + len)) -> 64 bytes
// op 1: ChaCha20 block (key slot[0..32), counter slot[32..36), nonce slot[36..48)) -> 64 bytes
// op 2: Poly1305 (key slot[0..32), message slot[32 .. 32 + len), len <= 128) -> 16 bytes
__host__ __device__ void run_one(int op, const uint8_t* slot, uint32_t len, uint8_t* out) {
    if (op == 0) {
        uint64_t m[16], h[8];
        for (int i = 0; i < 16; ++i) {
            m[i] = 0;
            for (int b = 7; b >= 0; --b) m[i] = (m[i] << 8) | ((uint32_t)(8 * i + b) < len ? slot[32 + 8 * i + b] : 0);
        }
        const uint64_t p0 = ld32(slot) | ((uint64_t)ld32(slot + 4) << 32), p1 = ld32(slot + 8) | ((uint64_t)ld32(slot + 12) << 32);
        blake2b_one_block(h, m, len, slot[16], p0, p1);
        for (int i = 0; i < 8; ++i) {
            st32(out + 8 * i, (uint32_t)h[i]);
            st32(out + 8 * i + 4, (uint32_t)(h[i] >> 32));
        }
    } else if (op == 1) {
        uint32_t key[8], nonce[3], o[16];
        for (int i = 0; i < 8; ++i) key[i] = ld32(slot + 4 * i);
        for (int i = 0; i < 3; ++i) nonce[i] = ld32(slot + 36 + 4 * i);
        chacha20_block(o, key, ld32(slot + 32), nonce);
        for (int i = 0; i < 16; ++i) st32(out + 4 * i, o[i]);
    } else {
        uint32_t key[8], tag[4];
        for (int i = 0; i < 8; ++i) key[i] = ld32(slot + 4 * i);
        Poly1305State st;
        poly1305_init(st, key);
        for (uint32_t off = 0; off < len; off += 16) {
            uint8_t blk[16];
            const bool full = len - off >= 16;
            for (uint32_t i = 0; i < 16; ++i) blk[i] = off + i < len ? slot[32 + off + i] : (off + i == len ? 1 : 0);
            poly1305_block(st, ld32(blk), ld32(blk + 4), ld32(blk + 8), ld32(blk + 12), full);
        }
        poly1305_finish(st, key + 4, tag);
        for (int i = 0; i < 4; ++i) st32(out + 4 * i, tag[i]);
    }
}

__global__ void k_run(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) run_one(op, slots + (size_t)STRIDE * i, lens[i], out + 64 * (size_t)i);
}

}  // namespace

extern "C" {

// n message slots of 160 bytes, lens[n] (<= 128), out n x 64
int nc_run_host(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        if (lens[i] > 128) return -1;
        run_one(op, slots + (size_t)STRIDE * i, lens[i], out + 64 * (size_t)i);
    }
    return 0;
}

int nc_run_gpu(int op, const uint8_t* slots, const uint32_t* lens, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i)
        if (lens[i] > 128) return -1;
    uint8_t *d_slots = nullptr, *d_out = nullptr;
    uint32_t* d_lens = nullptr;
    int rc = -2;
    if (hipMalloc(&d_slots, (size_t)STRIDE * n) == hipSuccess && hipMalloc(&d_lens, 4 * (size_t)n) == hipSuccess &&
        hipMalloc(&d_out, 64 * (size_t)n) == hipSuccess && hipMemcpy(d_slots, slots, (size_t)STRIDE * n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_lens, lens, 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_out, 0, 64 * (size_t)n) == hipSuccess) {
        hipLaunchKernelGGL(k_run, dim3((n + 63) / 64), dim3(64), 0, 0, op, d_slots, d_lens, n, d_out);
        if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(out, d_out, 64 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    (void)hipFree(d_slots);
    (void)hipFree(d_lens);
    (void)hipFree(d_out);
    return rc;
}

}  // extern "C"
