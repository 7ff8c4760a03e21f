// Launch schedule of the batch verifier's last device stage, shared by masp_hip_verify_batch (k_verify.hip) and the test-side unit
// tests/native/verify_dev.hip, so that the stage tests run the schedule that ships.  Only enqueues on `s`.
// Below it: the host tables of masp_hip_verify_each (the final exponentiation's programs and schedule, the key's points in device
// form), shared with tests/native/verify_each_dev.hip for the same reason.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "device/pairing.hpp"
#include "host/groth16_vk.h"
#include "host/pairing_prog.h"
#include "util.h"

namespace masp {

// Interpreter programs (host/pairing_prog.h) as the kernels read them: the ops of all of them in one array, and every program's step_start
// as absolute indices into it.  dev(i, ...) is program i over the uploaded copies of the two arrays; n_slots is what the largest one needs.
struct ProgramTable {
    std::vector<uint32_t> ops, steps;
    std::vector<size_t> st_off;
    std::vector<uint32_t> n_steps;
    uint32_t n_slots = 0;
    PairingProgramDev dev(int i, const uint32_t* d_ops, const uint32_t* d_steps) const { return {d_ops, d_steps + st_off[i], n_steps[i]}; }
};
inline ProgramTable concat_programs(std::initializer_list<const masp_host::prog::Program*> programs) {
    ProgramTable t;
    for (const masp_host::prog::Program* p : programs) {
        const uint32_t op_off = (uint32_t)t.ops.size();
        t.st_off.push_back(t.steps.size());
        for (uint32_t s : p->step_start) t.steps.push_back(s + op_off);
        t.ops.insert(t.ops.end(), p->ops.begin(), p->ops.end());
        t.n_steps.push_back((uint32_t)p->step_start.size() - 1);
        t.n_slots = std::max(t.n_slots, p->n_slots);
    }
    return t;
}
// the batch verifier's three: dbl, add (k_miller_pairs) and mul12 (k_fp12_product)
inline ProgramTable pairing_program_table() {
    const masp_host::prog::PairingPrograms& pp = masp_host::prog::pairing_programs();
    return concat_programs({&pp.dbl, &pp.add, &pp.mul12});
}

// vals[0] <- the product of the n Fp12 values at vals (12 Fp each, n >= 1; the others are overwritten with partial products):
// min(n, 64) waves multiply a strided share each, then one wave multiplies their results.  lds: n_slots x 48 bytes of dynamic LDS.
inline void launch_fp12_product(hipStream_t s, const PairingProgramDev& mul12, uint32_t n_slots, uint32_t lds, Fp* vals, uint32_t n) {
    const uint32_t g = std::min<uint32_t>(n, 64);
    MASP_LAUNCH(k_fp12_product, dim3(g), dim3(64), lds, s, mul12, n_slots, vals, n, g);
    if (g > 1) MASP_LAUNCH(k_fp12_product, dim3(1), dim3(64), lds, s, mul12, n_slots, vals, g, 1u);
}

// ---- masp_hip_verify_each ---------------------------------------------------------------------------------------------------
// host points -> device form.  Both sides keep Montgomery residues to the radix 2^384, so a coordinate is the same 48 bytes.
inline G1Affine dev_g1(const masp_host::bls::G1A& p) {
    G1Affine r;
    if (p.inf) return {fe_zero<FpCfg>(), fe_zero<FpCfg>()};
    memcpy(&r.x, &p.x, 48);
    memcpy(&r.y, &p.y, 48);
    return r;
}
inline G2Affine dev_g2(const masp_host::bls::G2A& p) {
    G2Affine r;
    if (p.inf) return {Fp2Ops::zero(), Fp2Ops::zero()};
    memcpy(&r.x.c0, &p.x.a, 48);
    memcpy(&r.x.c1, &p.x.b, 48);
    memcpy(&r.y.c0, &p.y.a, 48);
    memcpy(&r.y.c1, &p.y.b, 48);
    return r;
}
// the Jacobian points of a table in affine form with ONE inversion (the product of all Z, unwound)
inline void batch_affine(const std::vector<masp_host::bls::G1J>& in, G1Affine* out) {
    namespace hb = masp_host::bls;
    std::vector<hb::Fp> pre(in.size());
    hb::Fp run = hb::Fp::one();
    for (size_t i = 0; i < in.size(); ++i) {
        pre[i] = run;
        if (!in[i].Z.is_zero()) run = run * in[i].Z;
    }
    hb::Fp inv = run.inv();
    for (size_t i = in.size(); i-- > 0;) {
        if (in[i].Z.is_zero()) {
            out[i] = dev_g1({hb::Fp::zero(), hb::Fp::zero(), true});
            continue;
        }
        const hb::Fp zi = inv * pre[i], zi2 = zi.sq();
        inv = inv * in[i].Z;
        out[i] = dev_g1({in[i].X * zi2, in[i].Y * zi2 * zi, false});
    }
}

// IC_0, then per public input j the 64 x 15 multiples d 16^w IC_j (PreparedVk::ic_tab) in affine form: k_verify_acc's `ic0` and `tab`
inline std::vector<G1Affine> ic_table(const masp_host::PreparedVk& vk) {
    const size_t n_public = vk.ic.size() - 1;
    std::vector<G1Affine> ic(1 + 960 * n_public);
    ic[0] = dev_g1(vk.ic[0]);
    for (size_t j = 0; j < n_public; ++j) batch_affine(vk.ic_tab[j + 1], &ic[1 + 960 * j]);
    return ic;
}
// the six programs of the final exponentiation concatenated (mul, sq, frob, frob2, inv1, inv2), its schedule and the 15 Frobenius
// constants, as k_final_exp reads them
struct FinalExpTables : ProgramTable {
    std::vector<uint32_t> sched;
    Fp consts[15];
};
inline FinalExpTables final_exp_tables() {
    namespace mp = masp_host::prog;
    const mp::FinalExpPrograms& fp = mp::final_exp_programs();
    FinalExpTables t;
    static_cast<ProgramTable&>(t) = concat_programs({fp.all(0), fp.all(1), fp.all(2), fp.all(3), fp.all(4), fp.all(5)});
    t.sched = mp::final_exp_schedule();
    masp_host::bls::Fp c[15];
    mp::final_exp_constants(c);
    static_assert(sizeof(masp_host::bls::Fp) == sizeof(Fp), "one residue is 48 bytes on both sides");
    memcpy(t.consts, c, sizeof(c));
    return t;
}

}  // namespace masp
