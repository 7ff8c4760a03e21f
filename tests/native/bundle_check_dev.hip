// Test-only shim over the bundle pre-check's device code: masp_amd/csrc/device/bundle_check.hpp on the host (the header is __host__
// __device__), item by item, and a whole call as masp_hip_sapling_check_bundles runs it: the lanes of its kernels one after the other over
// the same arrays, with the proofs' statuses handed in (`Proof::read` is device-only; the tests take it from the host library).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/masp_hip.h"
#include "../../masp_amd/csrc/device/bundle_check.hpp"

using namespace masp;

namespace {

std::vector<uint32_t> words(const uint8_t* p, size_t bytes) {
    std::vector<uint32_t> w(bytes / 4 + 1);
    if (bytes) memcpy(w.data(), p, bytes);
    return w;
}

}  // namespace

extern "C" {

// one encoding -> BC_PT_*; uv64: canonical u | v (zeros if it does not decode)
int bcd_point(const uint8_t enc32[32], uint8_t uv64[64]) {
    uint32_t w[8], u[8], v[8];
    memcpy(w, enc32, 32);
    const int st = bc_point(u, v, w);
    memcpy(uv64, u, 32);
    memcpy(uv64 + 32, v, 32);
    return st;
}

// one value-balance entry -> 0, BC_BUNDLE_VALUE_RANGE or BC_BUNDLE_ASSET; out32: the encoding of the term that bvk adds
int bcd_balance_term(const uint8_t id32[32], const uint8_t value16[16], uint8_t out32[32]) {
    uint32_t id[8], val[4], w[8];
    memcpy(id, id32, 32);
    memcpy(val, value16, 16);
    JExt t;
    const int st = bc_balance_term(t, id, val);
    jj_encode(w, t);
    memcpy(out32, w, 32);
    return st;
}

void bcd_multipack(const uint8_t nf32[32], uint8_t out64[64]) {
    uint32_t nf[8], lo[8], hi[8];
    memcpy(nf, nf32, 32);
    bc_multipack(lo, hi, nf);
    memcpy(out64, lo, 32);
    memcpy(out64 + 32, hi, 32);
}

// A whole call on the host.  proof_refused: a byte per description (spends, then converts, then outputs), nonzero where `Proof::read`
// refuses its proof.  -> 0, or 1 where the entry point answers MASP_HIP_E_INVALID_ARG for the counts.
int bcd_check_bundles_host(const masp_hip_bundle_check* args, const uint8_t* proof_refused) {
    const masp_hip_bundle_check& h = *args;
    const size_t S = h.n_spends, C = h.n_converts, O = h.n_outputs, B = h.n_balance, N = h.n_bundles, P = 2 * S + C + 2 * O, D = S + C + O;
    if (N == 0) return 0;
    std::vector<uint32_t> offsets(4 * (N + 1));
    uint64_t run[4] = {0, 0, 0, 0};
    for (size_t b = 0; b <= N; ++b)
        for (int k = 0; k < 4; ++k) {
            offsets[4 * b + k] = (uint32_t)run[k];
            if (b < N) run[k] += h.counts[4 * b + k];
        }
    if (run[0] != S || run[1] != C || run[2] != O || run[3] != B) return 1;
    std::vector<uint8_t> enc8(32 * P + 1);
    if (S) memcpy(&enc8[0], h.spend_cv, 32 * S);
    if (S) memcpy(&enc8[32 * S], h.spend_rk, 32 * S);
    if (C) memcpy(&enc8[64 * S], h.convert_cv, 32 * C);
    if (O) memcpy(&enc8[64 * S + 32 * C], h.output_cv, 32 * O);
    if (O) memcpy(&enc8[64 * S + 32 * C + 32 * O], h.output_epk, 32 * O);
    const std::vector<uint32_t> enc = words(enc8.data(), 32 * P), sa = words(h.spend_anchor, 32 * S), nf = words(h.spend_nullifier, 32 * S),
                                ca = words(h.convert_anchor, 32 * C), cmu = words(h.output_cmu, 32 * O), asset = words(h.balance_asset, 32 * B),
                                value = words(h.balance_value, 16 * B);
    std::vector<uint8_t> proof_status(3 * D + 1, 0), pt_status(P + 1), term_status(B + 1), status(D + 1), bundle_status(N);
    for (size_t d = 0; d < D; ++d) proof_status[3 * d] = proof_refused[d] ? 1 : 0;
    std::vector<uint32_t> pt_uv(16 * P + 1), si(56 * S + 1), ci(24 * C + 1), oi(40 * O + 1), bvk(8 * N);
    std::vector<JExt> term(B + 1);
    BcArgs a;
    a.enc = enc.data();
    a.spend_anchor = sa.data();
    a.spend_nf = nf.data();
    a.convert_anchor = ca.data();
    a.output_cmu = cmu.data();
    a.asset = asset.data();
    a.value = value.data();
    a.offsets = offsets.data();
    a.proof_status = proof_status.data();
    a.pt_status = pt_status.data();
    a.pt_uv = pt_uv.data();
    a.term = term.data();
    a.term_status = term_status.data();
    a.status = status.data();
    a.spend_inputs = si.data();
    a.convert_inputs = ci.data();
    a.output_inputs = oi.data();
    a.bvk = bvk.data();
    a.bundle_status = bundle_status.data();
    a.n_spends = (uint32_t)S;
    a.n_converts = (uint32_t)C;
    a.n_outputs = (uint32_t)O;
    a.n_balance = (uint32_t)B;
    a.n_bundles = (uint32_t)N;
    for (uint32_t i = 0; i < P; ++i) bc_point_lane(a, i);
    for (uint32_t i = 0; i < B; ++i) bc_term_lane(a, i);
    for (uint32_t i = 0; i < D; ++i) bc_row_lane(a, i);
    for (uint32_t i = 0; i < N; ++i) bc_bvk_lane(a, i);
    if (S) memcpy(h.spend_status, &status[0], S);
    if (C) memcpy(h.convert_status, &status[S], C);
    if (O) memcpy(h.output_status, &status[S + C], O);
    if (S) memcpy(h.spend_inputs, si.data(), 224 * S);
    if (C) memcpy(h.convert_inputs, ci.data(), 96 * C);
    if (O) memcpy(h.output_inputs, oi.data(), 160 * O);
    memcpy(h.bvk, bvk.data(), 32 * N);
    memcpy(h.bundle_status, bundle_status.data(), N);
    return 0;
}

}  // extern "C"
