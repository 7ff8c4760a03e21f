// Test-only shim over the device header of the output recovery scan (masp_amd/csrc/device/out_recovery.hpp): its pair function on the
// host (the header is __host__ __device__) and, with the _gpu suffix, the same code in a kernel, one pair per lane.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../masp_amd/csrc/device/out_recovery.hpp"

using namespace masp;

namespace {

constexpr uint32_t ROW = 176;   // cv 32 | cmu 32 | epk 32 | out_ciphertext 80: the eleven columns in their order
constexpr uint32_t OUT = 36;    // ock 32 | 1 if the tag verifies, else 0, as a word

__host__ __device__ uint32_t ld32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
__host__ __device__ void st32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

__host__ __device__ void run_one(const uint8_t* ovk, const uint8_t* row, uint8_t* out) {
    uint32_t k[8], ock[8];
    uint4 col[OR_COLS];
    for (int i = 0; i < 8; ++i) k[i] = ld32(ovk + 4 * i);
    for (uint32_t c = 0; c < OR_COLS; ++c)
        col[c] = make_uint4(ld32(row + 16 * c), ld32(row + 16 * c + 4), ld32(row + 16 * c + 8), ld32(row + 16 * c + 12));
    const bool ok = or_pair(ock, k, col, 1);
    for (int i = 0; i < 8; ++i) st32(out + 4 * i, ock[i]);
    st32(out + 32, ok ? 1u : 0u);
}

__global__ void k_run(const uint8_t* ovks, const uint8_t* rows, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) run_one(ovks + 32 * (size_t)i, rows + (size_t)ROW * i, out + (size_t)OUT * i);
}

}  // namespace

extern "C" {

// n pairs: ovks n x 32, rows n x 176, out n x 36
int or_run_host(const uint8_t* ovks, const uint8_t* rows, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) run_one(ovks + 32 * (size_t)i, rows + (size_t)ROW * i, out + (size_t)OUT * i);
    return 0;
}

int or_run_gpu(const uint8_t* ovks, const uint8_t* rows, uint32_t n, uint8_t* out) {
    if (n == 0) return 0;
    uint8_t *d_ovks = nullptr, *d_rows = nullptr, *d_out = nullptr;
    int rc = -2;
    if (hipMalloc(&d_ovks, 32 * (size_t)n) == hipSuccess && hipMalloc(&d_rows, (size_t)ROW * n) == hipSuccess &&
        hipMalloc(&d_out, (size_t)OUT * n) == hipSuccess && hipMemcpy(d_ovks, ovks, 32 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_rows, rows, (size_t)ROW * n, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_out, 0, (size_t)OUT * n) == hipSuccess) {
        hipLaunchKernelGGL(k_run, dim3((n + 63) / 64), dim3(64), 0, 0, d_ovks, d_rows, n, d_out);
        if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(out, d_out, (size_t)OUT * n, hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    (void)hipFree(d_ovks);
    (void)hipFree(d_rows);
    (void)hipFree(d_out);
    return rc;
}

}  // extern "C"
