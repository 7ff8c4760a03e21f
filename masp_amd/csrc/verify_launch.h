// Launch schedule of the batch verifier's last device stage, shared by masp_hip_verify_batch (k_verify.hip) and the test-side unit
// tests/native/verify_dev.hip, so that the stage tests run the schedule that ships.  Only enqueues on `s`.
#pragma once
#include <algorithm>

#include "device/pairing.hpp"
#include "util.h"

namespace masp {

// vals[0] <- the product of the n Fp12 values at vals (12 Fp each, n >= 1; the others are overwritten with partial products):
// min(n, 64) waves multiply a strided share each, then one wave multiplies their results.  lds: n_slots x 48 bytes of dynamic LDS.
inline void launch_fp12_product(hipStream_t s, const PairingProgramDev& mul12, uint32_t n_slots, uint32_t lds, Fp* vals, uint32_t n) {
    const uint32_t g = std::min<uint32_t>(n, 64);
    MASP_LAUNCH(k_fp12_product, dim3(g), dim3(64), lds, s, mul12, n_slots, vals, n, g);
    if (g > 1) MASP_LAUNCH(k_fp12_product, dim3(1), dim3(64), lds, s, mul12, n_slots, vals, g, 1u);
}

}  // namespace masp
