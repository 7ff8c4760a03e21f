// The fixed-base table of the value commitments in the output descriptions (k_output_build.hip, device/output_build.hpp): the Niels
// points k 16^w G_vcr for k = 1..15 over 63 windows, in the device's Montgomery limbs and in the form of nullifier_table.h's: 945 points,
// 89 KiB.  Built once per process on the host from masp_host::generators(), uploaded once per context into a buffer of its own (under
// WalletState::mu); the tables of pedersen_table.h and nullifier_table.h stay what they are.
#pragma once
#include "device/output_build.hpp"
#include "nullifier_table.h"

namespace masp {

inline const std::vector<JNiels>& output_table() {
    static const std::vector<JNiels> t = [] {
        std::vector<JNiels> n(OB_VCR_TABLE);
        masp_host::JPoint base = masp_host::generators().value_commitment_randomness;
        for (uint32_t w = 0; w < OB_VCR_WINDOWS; ++w) {
            masp_host::JPoint p = base;
            for (uint32_t k = 0; k < 15; ++k) {
                const masp_host::JPoint::Niels e = masp_host::JPoint::Niels::from(p.to_affine());
                n[15 * w + k] = {fr_of_host(e.vmu), fr_of_host(e.vpu), fr_of_host(e.t2d)};
                p = p.add(base);
            }
            base = base.dbl().dbl().dbl().dbl();
        }
        return n;
    }();
    return t;
}

// enqueues the table's upload on `s` if the context does not hold it yet, as nullifier_table_ensure does
inline int output_table_ensure(WalletState& w, hipStream_t s) {
    const std::vector<JNiels>& t = output_table();
    return w.ob_table.ensure((const uint8_t*)t.data(), sizeof(JNiels) * t.size(), s);
}

}  // namespace masp
