// The fixed-base tables of the note nullifiers (k_nullifier.hip, device/nullifier.hpp): the Niels points k 16^w G for k = 1..15 of
// G_ncr (63 windows) and, behind them, of G_nf (16 windows), in the device's Montgomery limbs: 1 185 points, 111 KiB.  Built once per
// process on the host from masp_host::generators(), uploaded once per context into a buffer of its own (under WalletState::mu): the Pedersen table
// of pedersen_table.h, which the compact scan and the trees read, stays what it is.
#pragma once
#include "device/nullifier.hpp"
#include "pedersen_table.h"

namespace masp {

inline const std::vector<JNiels>& nullifier_table() {
    static const std::vector<JNiels> t = [] {
        std::vector<JNiels> n(NF_TABLE);
        auto fill = [&](JNiels* out, masp_host::JPoint base, uint32_t windows) {
            for (uint32_t w = 0; w < windows; ++w) {
                masp_host::JPoint p = base;
                for (uint32_t k = 0; k < 15; ++k) {
                    const masp_host::JPoint::Niels e = masp_host::JPoint::Niels::from(p.to_affine());
                    out[15 * w + k] = {fr_of_host(e.vmu), fr_of_host(e.vpu), fr_of_host(e.t2d)};
                    p = p.add(base);
                }
                base = base.dbl().dbl().dbl().dbl();
            }
        };
        fill(n.data(), masp_host::generators().note_commitment_randomness, NF_NCR_WINDOWS);
        fill(n.data() + NF_NCR_TABLE, masp_host::generators().nullifier_position, NF_POS_WINDOWS);
        return n;
    }();
    return t;
}

// enqueues the table's upload on `s` if the context does not hold it yet, as pedersen_table_ensure does
inline int nullifier_table_ensure(WalletState& w, hipStream_t s) {
    const std::vector<JNiels>& t = nullifier_table();
    return w.nf_table.ensure((const uint8_t*)t.data(), sizeof(JNiels) * t.size(), s);
}

}  // namespace masp
