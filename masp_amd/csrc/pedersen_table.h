// The Pedersen Niels table of a device context, shared by the compact note scan (k_note_scan_compact.hip: the NoteCommitment hash over all five
// segments) and the commitment tree (k_merkle.hip: the Merkle hash over the head of the first three): built once per process on the host from
// masp_host::pedersen_windows(), uploaded once per context by whichever of them runs first (under WalletState::mu).
#pragma once
#include "device/pedersen.hpp"
#include "host/jubjub.h"
#include "internal.h"

namespace masp {

inline Fr fr_of_host(const masp_host::Fr& x) {
    uint64_t c[4];
    x.to_canonical(c);
    Fr r;
    for (int i = 0; i < 4; ++i) {
        r.v[2 * i] = (uint32_t)c[i];
        r.v[2 * i + 1] = (uint32_t)(c[i] >> 32);
    }
    return fe_to_mont(r);
}

// the Niels points (k + 1) 16^w G_s, [segment][window][k], and G_ncr behind them, in the device's limbs
inline const std::vector<uint8_t>& pedersen_table_bytes() {
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

// enqueues the table's upload on `s` if the context does not hold it yet; the caller synchronises `s` before anything reads the table, and
// WalletCall::done releases it if the call fails before that is known
inline int pedersen_table_ensure(WalletState& w, hipStream_t s) {
    const std::vector<uint8_t>& t = pedersen_table_bytes();
    return w.nsc_table.ensure(t.data(), t.size(), s);
}

}  // namespace masp
