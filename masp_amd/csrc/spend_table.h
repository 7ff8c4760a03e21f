// The fixed-base tables of the spend descriptions and the RedJubjub signatures (k_spend_build.hip, device/spend_build.hpp): the Niels
// points k 16^w G for k = 1..15 over 63 windows of G_spend (spending_key_generator) and, behind them, of G_pgk
// (proof_generation_key_generator), in the device's Montgomery limbs and in the form of output_table.h's: 1 890 points, 177 KiB.  Built
// once per process on the host from masp_host::generators(), uploaded once per context into a buffer of its own (under WalletState::mu);
// binding signatures stand on G_vcr, whose windows output_table.h uploads.
#pragma once
#include "device/spend_build.hpp"
#include "output_table.h"

namespace masp {

inline const std::vector<JNiels>& spend_table() {
    static const std::vector<JNiels> t = [] {
        std::vector<JNiels> n(SB_TABLE);
        auto fill = [&](JNiels* out, masp_host::JPoint base) {
            for (uint32_t w = 0; w < SB_WINDOWS; ++w) {
                masp_host::JPoint p = base;
                for (uint32_t k = 0; k < 15; ++k) {
                    const masp_host::JPoint::Niels e = masp_host::JPoint::Niels::from(p.to_affine());
                    out[15 * w + k] = {fr_of_host(e.vmu), fr_of_host(e.vpu), fr_of_host(e.t2d)};
                    p = p.add(base);
                }
                base = base.dbl().dbl().dbl().dbl();
            }
        };
        fill(n.data(), masp_host::generators().spending_key);
        fill(n.data() + SB_BASE_TABLE, masp_host::generators().proof_generation_key);
        return n;
    }();
    return t;
}

// enqueues the table's upload on `s` if the context does not hold it yet, as output_table_ensure does
inline int spend_table_ensure(WalletState& w, hipStream_t s) {
    const std::vector<JNiels>& t = spend_table();
    return w.sb_table.ensure((const uint8_t*)t.data(), sizeof(JNiels) * t.size(), s);
}

}  // namespace masp
