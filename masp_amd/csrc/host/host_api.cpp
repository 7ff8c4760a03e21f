// libmasp_host: C ABI over the host-side witness generator (circuits.h).  This is the part of
// `SaplingProvingContext::{spend_proof, output_proof, convert_proof}` that precedes `create_random_proof`
// (/root/reference/masp_proofs/src/sapling/prover.rs:51-113, :163-198, :214-248): native key / commitment /
// nullifier derivation, then synthesis of the circuit into (input_assignment, aux_assignment).
// It also exports the static R1CS of each circuit (what bellperson's KeypairAssembly collects) and the
// native primitives, so that tests can pin them against the reference's vectors.
#include <atomic>
#include <memory>
#include <thread>

#include "../../../include/masp_host.h"   // the declarations of everything defined here: a mismatch does not compile
#include "circuits.h"
#include "groth16_vk.h"
#include "note_encryption.h"
#include "pairing_prog.h"
#include "pairing.h"

using namespace masp_host;



namespace {
struct CircuitHandle {
    std::unique_ptr<CS> cs;
};
Var remap(Var v, uint32_t n_inputs) { return (v & AUX) ? n_inputs + (v & ~AUX) : v; }

// aux_montgomery: the aux assignment leaves as Montgomery residues (four little-endian u64 limbs: blst_fr's memory, what
// masp_hip_job::aux_form = MASP_HIP_AUX_MONTGOMERY announces) — no conversion of ~30 000 non-boolean elements per Spend
void write_assignment(const CS& cs, uint8_t* inputs, uint8_t* aux, bool aux_montgomery = false) {
    for (size_t i = 0; i < cs.num_inputs(); ++i) cs.inputs()[i].to_bytes(inputs + 32 * i);
    if (aux_montgomery) {
        static_assert(sizeof(Fr) == 32, "Fr is four 64-bit Montgomery limbs");
        if (!cs.aux_in_place()) memcpy(aux, cs.aux(), 32 * cs.num_aux());   // (in place: the constraint system wrote into `aux` itself)
        return;
    }
    // 70 % of a MASP witness is 0 or 1 (booleans): no Montgomery conversion needed for those
    const Fr one = Fr::one();
    for (size_t j = 0; j < cs.num_aux(); ++j) {
        const Fr& v = cs.aux()[j];
        uint8_t* o = aux + 32 * j;
        if (v.is_zero()) {
            memset(o, 0, 32);
        } else if (v == one) {
            memset(o, 0, 32);
            o[0] = 1;
        } else {
            v.to_bytes(o);
        }
    }
}
// jubjub::Fr is a canonical value by construction in the reference; here scalars arrive as raw bytes.  The circuits witness
// only their low 252 bits while the native cv / rk / cm use all 256, so an unreduced scalar would give a silently
// invalid proof: reject anything >= the Jubjub subgroup order (0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7).
bool jubjub_scalar_canonical(const uint8_t s[32]) {
    static const uint8_t ORDER_LE[32] = {0xb7, 0x2c, 0xf7, 0xd6, 0x5e, 0x0e, 0x97, 0xd0, 0x82, 0x10, 0xc8, 0xcc, 0x93, 0x20, 0x68, 0xa6,
                                         0x00, 0x3b, 0x34, 0x01, 0x01, 0x3b, 0x67, 0x06, 0xa9, 0xaf, 0x33, 0x65, 0xea, 0xb4, 0x7d, 0x0e};
    for (int i = 31; i >= 0; --i) {
        if (s[i] < ORDER_LE[i]) return true;
        if (s[i] > ORDER_LE[i]) return false;
    }
    return false;  // equal to the order
}
// auxiliary variables of circuit `kind` (0 spend, 1 output, 2 convert): the size of the caller's aux buffer
size_t aux_count(int kind) {
    static const size_t n[3] = {[] {
                                    CS cs(false, false);
                                    SpendW w{};
                                    w.vc.asset_generator = w.ak = w.g_d = w.pk_d = JPoint::identity();
                                    synthesize_spend(cs, w);
                                    return cs.num_aux();
                                }(),
                                [] {
                                    CS cs(false, false);
                                    OutputW w{};
                                    w.vc.asset_generator = w.g_d = w.pk_d = JPoint::identity();
                                    synthesize_output(cs, w);
                                    return cs.num_aux();
                                }(),
                                [] {
                                    CS cs(false, false);
                                    ConvertW w{};
                                    w.vc.asset_generator = JPoint::identity();
                                    synthesize_convert(cs, w);
                                    return cs.num_aux();
                                }()};
    return n[kind];
}
// the constraint system of one witness: straight into the caller's aux buffer when that is to hold Montgomery residues (check & 2)
// and nothing is recorded
CS* new_witness_cs(int kind, int check, uint8_t* aux) {
    if ((check & 2) && !(check & 1) && ((uintptr_t)aux % alignof(Fr)) == 0) return new CS(false, true, reinterpret_cast<Fr*>(aux), aux_count(kind));
    return new CS((check & 1) != 0, true);
}
bool load_path(MerklePathW& p, const uint8_t* siblings, uint64_t position) {
    for (int i = 0; i < TREE_DEPTH; ++i) {
        Fr s;
        if (!Fr::from_bytes(s, siblings + 32 * i)) return false;
        p.auth_path.push_back({s, (bool)((position >> i) & 1)});
    }
    return true;
}
}  // namespace

#ifdef MASP_HOST_TIMING
#include <chrono>
#define TIMING_T0 auto _t = std::chrono::steady_clock::now(); static double _acc[8]; static const char* _nm[8]; static int _calls; int _k = 0;
#define TIMING_MARK(NAME) { auto _n = std::chrono::steady_clock::now(); int _i = 0; for (; _i < 8 && _nm[_i] && strcmp(_nm[_i], NAME); ++_i); _nm[_i] = NAME; _acc[_i] += std::chrono::duration<double, std::milli>(_n - _t).count(); _t = _n; }
#else
#define TIMING_T0
#define TIMING_MARK(NAME)
#endif

extern "C" {


// ---- static circuits: kind 0 spend, 1 output, 2 convert --------------------------------------------
void* masp_host_circuit_setup(int kind) {
    if (!Fr::one_constant_ok()) return nullptr;
    try {
        std::unique_ptr<CircuitHandle> h(new CircuitHandle);
        h->cs.reset(new CS(true, false));
        if (kind == 0) {
            SpendW w{};
            w.vc.asset_generator = JPoint::identity();
            w.ak = w.g_d = w.pk_d = JPoint::identity();
            synthesize_spend(*h->cs, w);
        } else if (kind == 1) {
            OutputW w{};
            w.vc.asset_generator = JPoint::identity();
            w.g_d = w.pk_d = JPoint::identity();
            synthesize_output(*h->cs, w);
        } else if (kind == 2) {
            ConvertW w{};
            w.vc.asset_generator = JPoint::identity();
            synthesize_convert(*h->cs, w);
        } else {
            return nullptr;
        }
        return h.release();
    } catch (...) {
        return nullptr;
    }
}
void masp_host_circuit_free(void* h) { delete (CircuitHandle*)h; }
// out: n_inputs, n_aux, n_constraints, nnz(A), nnz(B), nnz(C)
void masp_host_circuit_counts(void* hh, uint32_t* out) {
    CS& cs = *((CircuitHandle*)hh)->cs;
    out[0] = cs.num_inputs();
    out[1] = cs.num_aux();
    out[2] = cs.num_constraints();
    for (int i = 0; i < 3; ++i) out[3 + i] = cs.matrix(i).col.size();
}
// columns: input i -> i, aux j -> n_inputs + j (the masp_hip_r1cs convention); coef 32 B LE canonical
void masp_host_circuit_matrix(void* hh, int mi, uint32_t* rowptr, uint32_t* col, uint8_t* coef) {
    CS& cs = *((CircuitHandle*)hh)->cs;
    const CS::Matrix& M = cs.matrix(mi);
    memcpy(rowptr, M.rowptr.data(), 4 * M.rowptr.size());
    for (size_t t = 0; t < M.col.size(); ++t) {
        col[t] = remap(M.col[t], (uint32_t)cs.num_inputs());
        M.coef[t].to_bytes(coef + 32 * t);
    }
}
void masp_host_circuit_hash(void* hh, char* out65) {
    std::string s = ((CircuitHandle*)hh)->cs->hash();
    memcpy(out65, s.c_str(), 65);
}

// ---- witness generation -----------------------------------------------------------------------------
// check & 1: additionally record the constraints and fail with MASP_HOST_E_UNSATISFIED if any is violated.
// check & 2: write the aux assignment as Montgomery residues (see write_assignment) instead of canonical bytes.
// rcm is the note commitment randomness `note.rcm()` (sapling.rs:856-863) as 32 bytes LE.
int masp_host_spend_assignment(const uint8_t ak[32], const uint8_t nsk[32], const uint8_t diversifier[11], const uint8_t rcm[32],
                               const uint8_t ar[32], const uint8_t asset_identifier[32], uint64_t value, const uint8_t anchor[32],
                               const uint8_t* path_siblings /*32 x 32*/, uint64_t position, const uint8_t rcv[32], int check,
                               uint8_t* inputs /*8 x 32*/, uint8_t* aux /*100497 x 32*/, uint8_t cv_out[32], uint8_t rk_out[32],
                               uint8_t nf_out[32]) {
    try {
        SpendW w;
        if (!jubjub_scalar_canonical(nsk) || !jubjub_scalar_canonical(rcm) || !jubjub_scalar_canonical(ar) || !jubjub_scalar_canonical(rcv))
            return MASP_HOST_E_INVALID;
        if (!asset_generator(w.vc.asset_generator, asset_identifier)) return MASP_HOST_E_INVALID;
        w.vc.value = value;
        memcpy(w.vc.randomness, rcv, 32);
        if (!JPoint::from_bytes(w.ak, ak)) return MASP_HOST_E_INVALID;
        memcpy(w.nsk, nsk, 32);
        memcpy(w.rcm, rcm, 32);
        memcpy(w.ar, ar, 32);
        if (!Fr::from_bytes(w.anchor, anchor) || !load_path(w.path, path_siblings, position)) return MASP_HOST_E_INVALID;
        // viewing key, payment address (prover.rs:78-84)
        JPoint nk = generators().proof_generation_key.mul(nsk);
        uint8_t ivk[32];
        crh_ivk(ivk, w.ak, nk);
        if (!group_hash(w.g_d, diversifier, 11, "MASP__gd")) return MASP_HOST_E_DIVERSIFIER;
        w.pk_d = w.g_d.mul(ivk);
        // outputs the caller needs next to the proof (prover.rs:87-98,151-156)
        JPoint cv = value_commitment(w.vc.asset_generator, value, rcv);
        JPoint rk = w.ak.add(generators().spending_key.mul(ar));
        JPoint cm = note_commitment(w.vc.asset_generator, value, w.g_d, w.pk_d, rcm);
        cv.to_bytes(cv_out);
        rk.to_bytes(rk_out);
        nullifier(nf_out, cm, position, nk);
        std::unique_ptr<CS> cs_owner(new_witness_cs(0, check, aux));
        CS& cs = *cs_owner;
        synthesize_spend(cs, w);
        if ((check & 1) && cs.first_unsatisfied() >= 0) return MASP_HOST_E_UNSATISFIED;
        write_assignment(cs, inputs, aux, (check & 2) != 0);
        return MASP_HOST_OK;
    } catch (const SynthesisError&) {
        return MASP_HOST_E_SYNTHESIS;
    }
}
int masp_host_output_assignment(const uint8_t esk[32], const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t rcm[32],
                                const uint8_t asset_identifier[32], uint64_t value, const uint8_t rcv[32], int check,
                                uint8_t* inputs /*6 x 32*/, uint8_t* aux /*30896 x 32*/, uint8_t cv_out[32]) {
    try {
        OutputW w;
        if (!jubjub_scalar_canonical(esk) || !jubjub_scalar_canonical(rcm) || !jubjub_scalar_canonical(rcv)) return MASP_HOST_E_INVALID;
        if (!asset_generator(w.vc.asset_generator, asset_identifier)) return MASP_HOST_E_INVALID;
        w.vc.value = value;
        memcpy(w.vc.randomness, rcv, 32);
        memcpy(w.asset_identifier, asset_identifier, 32);
        if (!group_hash(w.g_d, diversifier, 11, "MASP__gd")) return MASP_HOST_E_DIVERSIFIER;
        if (!JPoint::from_bytes(w.pk_d, pk_d)) return MASP_HOST_E_INVALID;
        memcpy(w.rcm, rcm, 32);
        memcpy(w.esk, esk, 32);
        value_commitment(w.vc.asset_generator, value, rcv).to_bytes(cv_out);
        std::unique_ptr<CS> cs_owner(new_witness_cs(1, check, aux));
        CS& cs = *cs_owner;
        synthesize_output(cs, w);
        if ((check & 1) && cs.first_unsatisfied() >= 0) return MASP_HOST_E_UNSATISFIED;
        write_assignment(cs, inputs, aux, (check & 2) != 0);
        return MASP_HOST_OK;
    } catch (const SynthesisError&) {
        return MASP_HOST_E_SYNTHESIS;
    }
}
// generator: the AllowedConversion's asset generator point (masp_primitives/src/convert.rs:23-29), 32 bytes
int masp_host_convert_assignment(const uint8_t generator[32], uint64_t value, const uint8_t anchor[32], const uint8_t* path_siblings,
                                 uint64_t position, const uint8_t rcv[32], int check, uint8_t* inputs /*4 x 32*/,
                                 uint8_t* aux /*47322 x 32*/, uint8_t cv_out[32]) {
    try {
        ConvertW w;
        if (!jubjub_scalar_canonical(rcv)) return MASP_HOST_E_INVALID;
        if (!JPoint::from_bytes(w.vc.asset_generator, generator)) return MASP_HOST_E_INVALID;
        w.vc.value = value;
        memcpy(w.vc.randomness, rcv, 32);
        if (!Fr::from_bytes(w.anchor, anchor) || !load_path(w.path, path_siblings, position)) return MASP_HOST_E_INVALID;
        value_commitment(w.vc.asset_generator, value, rcv).to_bytes(cv_out);
        std::unique_ptr<CS> cs_owner(new_witness_cs(2, check, aux));
        CS& cs = *cs_owner;
        synthesize_convert(cs, w);
        if ((check & 1) && cs.first_unsatisfied() >= 0) return MASP_HOST_E_UNSATISFIED;
        write_assignment(cs, inputs, aux, (check & 2) != 0);
        return MASP_HOST_OK;
    } catch (const SynthesisError&) {
        return MASP_HOST_E_SYNTHESIS;
    }
}

// n field elements as Montgomery residues (four little-endian u64 limbs: what `check & 2` makes the synthesizers write) ->
// 32-byte little-endian canonical values.  For callers that need both forms of an assignment (a checker next to the prover).
void masp_host_fr_from_montgomery(const uint8_t* in, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        Fr v;
        memcpy(v.l, in + 32 * i, 32);
        v.to_bytes(out + 32 * i);
    }
}

// ---- several witnesses per call: the Merkle blocks in lockstep (circuits.h merkle_block_batch) -------------------------
// One job = the arguments of masp_host_spend_assignment / masp_host_convert_assignment plus its return code.  `check` as there
// (check & 1 records and verifies the constraints: that goes witness by witness through the generic gadgets).  Returns the number
// of jobs whose rc is not MASP_HOST_OK.  A caller gives each of its threads a group of ~16 jobs.
// (masp_host_spend_job / masp_host_convert_job: include/masp_host.h)
int masp_host_spend_assignments(size_t n, masp_host_spend_job* jobs, int check) {
    if (check & 1) {
        int bad = 0;
        for (size_t j = 0; j < n; ++j) {
            masp_host_spend_job& J = jobs[j];
            J.rc = masp_host_spend_assignment(J.ak, J.nsk, J.diversifier, J.rcm, J.ar, J.asset_identifier, J.value, J.anchor, J.path_siblings, J.position,
                                              J.rcv, check, J.inputs, J.aux, J.cv_out, J.rk_out, J.nf_out);
            bad += J.rc != MASP_HOST_OK;
        }
        return bad;
    }
    std::vector<SpendW> w(n);
    std::vector<std::unique_ptr<CS>> cs(n);
    std::vector<SpendState> st(n);
    std::vector<size_t> live;
    TIMING_T0
    for (size_t j = 0; j < n; ++j) {
        masp_host_spend_job& J = jobs[j];
        J.rc = MASP_HOST_OK;
        try {
            SpendW& W = w[j];
            if (!jubjub_scalar_canonical(J.nsk) || !jubjub_scalar_canonical(J.rcm) || !jubjub_scalar_canonical(J.ar) || !jubjub_scalar_canonical(J.rcv) ||
                !asset_generator(W.vc.asset_generator, J.asset_identifier) || !JPoint::from_bytes(W.ak, J.ak)) {
                J.rc = MASP_HOST_E_INVALID;
                continue;
            }
            W.vc.value = J.value;
            memcpy(W.vc.randomness, J.rcv, 32);
            memcpy(W.nsk, J.nsk, 32);
            memcpy(W.rcm, J.rcm, 32);
            memcpy(W.ar, J.ar, 32);
            if (!Fr::from_bytes(W.anchor, J.anchor) || !load_path(W.path, J.path_siblings, J.position)) {
                J.rc = MASP_HOST_E_INVALID;
                continue;
            }
            JPoint nk = generators().proof_generation_key.mul(J.nsk);
            uint8_t ivk[32];
            crh_ivk(ivk, W.ak, nk);
            if (!group_hash(W.g_d, J.diversifier, 11, "MASP__gd")) {
                J.rc = MASP_HOST_E_DIVERSIFIER;
                continue;
            }
            W.pk_d = W.g_d.mul(ivk);
            JPoint cv = value_commitment(W.vc.asset_generator, J.value, J.rcv);
            JPoint rk = W.ak.add(generators().spending_key.mul(J.ar));
            JPoint cm = note_commitment(W.vc.asset_generator, J.value, W.g_d, W.pk_d, J.rcm);
            cv.to_bytes(J.cv_out);
            rk.to_bytes(J.rk_out);
            nullifier(J.nf_out, cm, J.position, nk);
            cs[j].reset(new_witness_cs(0, check, J.aux));
            synthesize_spend_pre(*cs[j], W, st[j]);
            live.push_back(j);
        } catch (const SynthesisError&) {
            J.rc = MASP_HOST_E_SYNTHESIS;
        }
    }
    TIMING_MARK("pre")
    // the Merkle blocks of all live witnesses side by side
    {
        std::vector<CS*> c;
        std::vector<AllocatedNum> cur;
        std::vector<const MerklePathW*> paths;
        std::vector<std::vector<Boolean>*> pos;
        std::vector<size_t> mark;
        for (size_t j : live) {
            c.push_back(cs[j].get());
            cur.push_back(st[j].cur);
            paths.push_back(&w[j].path);
            pos.push_back(&st[j].position_bits);
            mark.push_back(cs[j]->num_aux());
        }
        bool fast = false;
        try {
            fast = !live.empty() && merkle_block_batch(live.size(), c.data(), cur.data(), paths.data(), pos.data());
        } catch (const std::exception&) {
            fast = false;
        }
        for (size_t i = 0; i < live.size(); ++i) {
            const size_t j = live[i];
            if (fast) {
                st[j].cur = cur[i];
                continue;
            }
            try {  // a vanished denominator somewhere in the batch: every witness through the gadgets, which report it as the reference does
                cs[j]->truncate_aux(mark[i]);
                st[j].position_bits.clear();
                st[j].cur = merkle_ascend(*cs[j], st[j].cur, w[j].path, &st[j].position_bits);
            } catch (const SynthesisError&) {
                jobs[j].rc = MASP_HOST_E_SYNTHESIS;
            }
        }
    }
    TIMING_MARK("merkle")
    int bad = 0;
    for (size_t j = 0; j < n; ++j) {
        masp_host_spend_job& J = jobs[j];
        if (J.rc == MASP_HOST_OK) {
            try {
                synthesize_spend_post(*cs[j], w[j], st[j]);
                TIMING_MARK("post")
                write_assignment(*cs[j], J.inputs, J.aux, (check & 2) != 0);
                TIMING_MARK("write")
            } catch (const SynthesisError&) {
                J.rc = MASP_HOST_E_SYNTHESIS;
            }
        }
        bad += J.rc != MASP_HOST_OK;
    }
#ifdef MASP_HOST_TIMING
    if (++_calls % 4 == 0) { for (int i = 0; i < 8 && _nm[i]; ++i) fprintf(stderr, "%s %.3f ms/inst  ", _nm[i], _acc[i] / (_calls * n)); fprintf(stderr, "\n"); }
#endif
    return bad;
}
int masp_host_convert_assignments(size_t n, masp_host_convert_job* jobs, int check) {
    if (check & 1) {
        int bad = 0;
        for (size_t j = 0; j < n; ++j) {
            masp_host_convert_job& J = jobs[j];
            J.rc = masp_host_convert_assignment(J.generator, J.value, J.anchor, J.path_siblings, J.position, J.rcv, check, J.inputs, J.aux, J.cv_out);
            bad += J.rc != MASP_HOST_OK;
        }
        return bad;
    }
    std::vector<ConvertW> w(n);
    std::vector<std::unique_ptr<CS>> cs(n);
    std::vector<ConvertState> st(n);
    std::vector<size_t> live;
    for (size_t j = 0; j < n; ++j) {
        masp_host_convert_job& J = jobs[j];
        J.rc = MASP_HOST_OK;
        try {
            ConvertW& W = w[j];
            if (!jubjub_scalar_canonical(J.rcv) || !JPoint::from_bytes(W.vc.asset_generator, J.generator)) {
                J.rc = MASP_HOST_E_INVALID;
                continue;
            }
            W.vc.value = J.value;
            memcpy(W.vc.randomness, J.rcv, 32);
            if (!Fr::from_bytes(W.anchor, J.anchor) || !load_path(W.path, J.path_siblings, J.position)) {
                J.rc = MASP_HOST_E_INVALID;
                continue;
            }
            value_commitment(W.vc.asset_generator, J.value, J.rcv).to_bytes(J.cv_out);
            cs[j].reset(new_witness_cs(2, check, J.aux));
            synthesize_convert_pre(*cs[j], W, st[j]);
            live.push_back(j);
        } catch (const SynthesisError&) {
            J.rc = MASP_HOST_E_SYNTHESIS;
        }
    }
    {
        std::vector<CS*> c;
        std::vector<AllocatedNum> cur;
        std::vector<const MerklePathW*> paths;
        std::vector<std::vector<Boolean>*> pos;
        std::vector<size_t> mark;
        for (size_t j : live) {
            c.push_back(cs[j].get());
            cur.push_back(st[j].cur);
            paths.push_back(&w[j].path);
            pos.push_back(nullptr);
            mark.push_back(cs[j]->num_aux());
        }
        bool fast = false;
        try {
            fast = !live.empty() && merkle_block_batch(live.size(), c.data(), cur.data(), paths.data(), pos.data());
        } catch (const std::exception&) {
            fast = false;
        }
        for (size_t i = 0; i < live.size(); ++i) {
            const size_t j = live[i];
            if (fast) {
                st[j].cur = cur[i];
                continue;
            }
            try {
                cs[j]->truncate_aux(mark[i]);
                st[j].cur = merkle_ascend(*cs[j], st[j].cur, w[j].path, nullptr);
            } catch (const SynthesisError&) {
                jobs[j].rc = MASP_HOST_E_SYNTHESIS;
            }
        }
    }
    int bad = 0;
    for (size_t j = 0; j < n; ++j) {
        masp_host_convert_job& J = jobs[j];
        if (J.rc == MASP_HOST_OK) {
            try {
                synthesize_convert_post(*cs[j], w[j], st[j]);
                write_assignment(*cs[j], J.inputs, J.aux, (check & 2) != 0);
            } catch (const SynthesisError&) {
                J.rc = MASP_HOST_E_SYNTHESIS;
            }
        }
        bad += J.rc != MASP_HOST_OK;
    }
    return bad;
}

// ---- Groth16 self-verification (sapling/prover.rs:148,266) ---------------------------------------------
// params: the Parameters bytes (only the verifying-key prefix is read).  Returns a handle or NULL.
void* masp_host_vk_prepare(const uint8_t* params, size_t len) {
    std::unique_ptr<PreparedVk> vk(new PreparedVk);
    if (!prepare_vk(*vk, params, len)) return nullptr;
    return vk.release();
}
void masp_host_vk_free(void* h) { delete (PreparedVk*)h; }
// public_inputs: n_public x 32 B LE, excluding ONE.  1 = valid, 0 = invalid, < 0 = malformed
int masp_host_vk_verify(const void* h, const uint8_t proof[192], const uint8_t* public_inputs, uint32_t n_public) {
    const PreparedVk& vk = *(const PreparedVk*)h;
    if ((size_t)n_public + 1 != vk.ic.size()) return -1;
    bls::G1A a, c;
    bls::G2A b;
    if (!bls::g1_compressed(a, proof) || !bls::g2_compressed(b, proof + 48) || !bls::g1_compressed(c, proof + 144)) return -2;
    if (a.inf || b.inf || c.inf) return -2;  // bellman's Proof::read refuses the identity in any of the three ("point at infinity")
    bls::G1J acc = bls::G1J::from(vk.ic[0]);
    for (uint32_t i = 0; i < n_public; ++i) {
        Fr chk;
        if (!Fr::from_bytes(chk, public_inputs + 32 * i)) return -3;
        acc = acc.add(vk.ic_mul(i + 1, public_inputs + 32 * i));
    }
    // e(A, B) == e(alpha, beta) e(acc, gamma) e(C, delta)   <=>   ML(A,B) ML(-acc,gamma) ML(-C,delta) / ML(alpha,beta) -> 1
    // (conj = inverse once final-exponentiated)
    bls::G1A nacc = acc.affine(), nc = c;
    nacc.y = nacc.y.neg();
    nc.y = nc.y.neg();
    std::vector<bls::MillerPair> pairs;
    if (!a.inf && !b.inf) pairs.emplace_back(a, b);
    if (!nacc.inf) pairs.emplace_back(nacc, vk.gamma);
    if (!nc.inf) pairs.emplace_back(nc, vk.delta);
    bls::Fp12 f = bls::multi_miller(pairs) * vk.alpha_beta.conj();
    return bls::final_exp(f) == bls::Fp12::one() ? 1 : 0;
}
// bellman `Proof::read` alone, as BatchValidator::check_bundle calls it before queueing a proof
// (masp_proofs/src/sapling/verifier/batch.rs:85,125,154): 1 = the three points are canonical, on the curve, in the
// prime-order subgroups and none is the identity; 0 = refused
int masp_host_proof_read(const uint8_t proof[192]) {
    bls::G1A a, c;
    bls::G2A b;
    if (!bls::g1_compressed(a, proof) || !bls::g2_compressed(b, proof + 48) || !bls::g1_compressed(c, proof + 144)) return 0;
    return a.inf || b.inf || c.inf ? 0 : 1;
}
// Batched form (bellman `verify_proofs_batch`, reached from /root/reference/masp_proofs/src/sapling/verifier/batch.rs:24-31):
// with random z_i,  prod_i e(z_i A_i, B_i) == e(alpha,beta)^(sum z_i) e(sum_i z_i acc_i, gamma) e(sum_i z_i C_i, delta).
// proofs: n x 192 B; public_inputs: n x n_public x 32 B; z: n x 16 B of caller-supplied randomness (128-bit coefficients).
// 1 = all valid, 0 = at least one invalid (the caller re-checks one by one to find it), < 0 = malformed.
int masp_host_vk_verify_batch(const void* h, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint32_t n_public,
                              const uint8_t* z) {
    const PreparedVk& vk = *(const PreparedVk*)h;
    if ((size_t)n_public + 1 != vk.ic.size()) return -1;
    if (n == 0) return 1;
    std::vector<bls::MillerPair> pairs;
    pairs.reserve(n);
    bls::G1J csum = bls::G1J::inf();
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* pr = proofs + 192 * i;
        bls::G1A a, c;
        bls::G2A b;
        if (!bls::g1_compressed(a, pr) || !bls::g2_compressed(b, pr + 48) || !bls::g1_compressed(c, pr + 144)) return -2;
        if (a.inf || b.inf || c.inf) return -2;  // (as above: Proof::read refuses the identity)
        uint8_t zi[32] = {0};
        memcpy(zi, z + 16 * i, 16);
        zi[0] |= 1;  // never zero
        bls::G1A za = bls::G1J::from(a).mul_le(zi, 128).affine();
        csum = csum.add(bls::G1J::from(c).mul_le(zi, 128));
        if (!za.inf && !b.inf) pairs.emplace_back(za, b);
    }
    return batch_verify_finish(vk, n, public_inputs, n_public, z, bls::multi_miller(pairs), csum.affine());
}

// The Miller loop of the GPU batch verifier exists as levelled straight-line programs (host/pairing_prog.h).  This runs
// them on the host interpreter for one pair (P: 96 B uncompressed G1, Q: 192 B uncompressed G2) and compares the result,
// coefficient for coefficient, with this library's own Miller loop (pairing.h) and with the templated tower instantiated
// over the concrete field.  0 = equal.  stats (may be NULL): ops / steps / steps with products / products / slots of
// the doubling program, then the same five of the addition program, then of the Fp12 product.
int masp_host_pairing_program_selftest(const uint8_t* p96, const uint8_t* q192, uint32_t* stats) {
    bls::G1A P;
    bls::G2A Q;
    if (!bls::g1_uncompressed(P, p96) || !bls::g2_uncompressed(Q, q192) || P.inf || Q.inf) return -1;
    const prog::PairingPrograms& pp = prog::pairing_programs();
    if (stats) {
        const prog::Program* ps[3] = {&pp.dbl, &pp.add, &pp.mul12};
        for (int i = 0; i < 3; ++i) {
            stats[5 * i] = (uint32_t)ps[i]->ops.size();
            stats[5 * i + 1] = (uint32_t)ps[i]->step_start.size() - 1;
            stats[5 * i + 2] = ps[i]->n_mul_steps;
            stats[5 * i + 3] = ps[i]->n_mul;
            stats[5 * i + 4] = ps[i]->n_slots;
        }
    }
    const bls::Fp12 want = bls::miller(P, Q);
    if (!(prog::miller_by_program(P, Q) == want)) return 1;
    // the templated formulas over the concrete field, step by step
    prog::Fp12T<bls::Fp> f = {{{bls::Fp::one(), bls::Fp::zero()}, {bls::Fp::zero(), bls::Fp::zero()}, {bls::Fp::zero(), bls::Fp::zero()}},
                              {{bls::Fp::zero(), bls::Fp::zero()}, {bls::Fp::zero(), bls::Fp::zero()}, {bls::Fp::zero(), bls::Fp::zero()}}};
    prog::MillerT<bls::Fp> m;
    m.xp = P.x; m.yp = P.y;
    m.xq = {Q.x.a, Q.x.b}; m.yq = {Q.y.a, Q.y.b};
    m.X = m.xq; m.Y = m.yq; m.Z = {bls::Fp::one(), bls::Fp::zero()};
    const uint64_t xabs = 0xd201000000010000ull;
    for (int b = 62; b >= 0; --b) {
        f = f.sq();
        m.dbl_step(f);
        if ((xabs >> b) & 1) m.add_step(f);
    }
    bls::Fp12 g = {{{f.a.a.a, f.a.a.b}, {f.a.b.a, f.a.b.b}, {f.a.c.a, f.a.c.b}}, {{f.b.a.a, f.b.a.b}, {f.b.b.a, f.b.b.b}, {f.b.c.a, f.b.c.b}}};
    if (!(g.conj() == want)) return 2;
    // Fp12 product program
    std::vector<bls::Fp> sl(pp.n_slots, bls::Fp::zero());
    const bls::Fp12 y = want.sq();
    auto flat = [](const bls::Fp12& x, bls::Fp* o) {
        const bls::Fp v[12] = {x.a.a.a, x.a.a.b, x.a.b.a, x.a.b.b, x.a.c.a, x.a.c.b, x.b.a.a, x.b.a.b, x.b.b.a, x.b.b.b, x.b.c.a, x.b.c.b};
        for (int i = 0; i < 12; ++i) o[i] = v[i];
    };
    bls::Fp pf[12];
    flat(want, &sl[prog::SLOT_F]);
    flat(y, &sl[prog::SLOT_Y]);
    prog::run_program(pp.mul12, sl.data());
    flat(want * y, pf);
    for (int i = 0; i < 12; ++i)
        if (!(sl[prog::SLOT_F + i] == pf[i])) return 3;
    return 0;
}

// The final exponentiation of the GPU per-proof verifier exists as programs too (host/pairing_prog.h: product, squaring, the two
// Frobenius maps, the two halves of the inversion) under one driver that the device kernel shares.  This runs them on the host
// interpreter in the kernel's order on f (in576: 12 Fp, 48 bytes big-endian each, in the flat order of bls::Fp12) and compares the
// result, coefficient for coefficient, with bls::final_exp.  0 = equal, out576 = f^(3 (p^12 - 1) / r);  2 = f has norm zero (only
// f = 0 has), the branch before the inversion was taken and the verdict of such a value is "invalid" (out576 = zeros);  1 = the two
// differ;  3 = the zero-norm branch was taken for a value that has an inverse;  -1 = a coefficient >= p.
// stats (may be NULL, 32 words): ops / steps / steps with products / products / slots of mul, sq, frob, frob2, inv1, inv2, then
// the slots of the whole set (saved values and constants included) and the bytes of LDS they take on the device.
int masp_host_final_exp_program_selftest(const uint8_t* in576, uint8_t* out576, uint32_t* stats) {
    const prog::FinalExpPrograms& fp = prog::final_exp_programs();
    if (stats) {
        for (int i = 0; i < 6; ++i) {
            const prog::Program* q = fp.all(i);
            stats[5 * i] = (uint32_t)q->ops.size();
            stats[5 * i + 1] = (uint32_t)q->step_start.size() - 1;
            stats[5 * i + 2] = q->n_mul_steps;
            stats[5 * i + 3] = q->n_mul;
            stats[5 * i + 4] = q->n_slots;
        }
        stats[30] = fp.n_slots;
        stats[31] = fp.n_slots * 48;
    }
    bls::Fp12 f, got;
    bls::Fp* c = &f.a.a.a;
    bool zero = true;
    for (int i = 0; i < 12; ++i) {
        if (!bls::Fp::from_be(c[i], in576 + 48 * i)) return -1;
        zero = zero && c[i].is_zero();
    }
    memset(out576, 0, 576);
    if (!prog::final_exp_by_program(f, got)) return zero ? 2 : 3;
    if (!(got == bls::final_exp(f))) return 1;
    const bls::Fp* g = &got.a.a.a;
    for (int i = 0; i < 12; ++i) {
        uint64_t v[6];
        g[i].canon(v);
        for (int k = 0; k < 48; ++k) out576[48 * i + k] = (uint8_t)(v[5 - k / 8] >> (8 * (7 - k % 8)));
    }
    return 0;
}

// ---- native primitives (pinned by the reference's vectors in tests/) ---------------------------------
// which: 0 proof_generation_key 1 note_commitment_randomness 2 nullifier_position 3 value_commitment_randomness
//        4 spending_key 5..10 pedersen[0..5]; out: u | v as 2 x 32 B LE
void masp_host_generator(int which, uint8_t out64[64]) {
    const Generators& g = generators();
    const JPoint* p[11] = {&g.proof_generation_key, &g.note_commitment_randomness, &g.nullifier_position, &g.value_commitment_randomness,
                           &g.spending_key, &g.pedersen[0], &g.pedersen[1], &g.pedersen[2], &g.pedersen[3], &g.pedersen[4], &g.pedersen[5]};
    JAffine a = p[which]->to_affine();
    a.u.to_bytes(out64);
    a.v.to_bytes(out64 + 32);
}
// personalization: -1 NoteCommitment, otherwise MerkleTree(depth); bits: one byte per bit; out: u | v
void masp_host_pedersen_hash(int personalization, const uint8_t* bits, size_t nbits, uint8_t out64[64]) {
    std::vector<bool> b(nbits);
    for (size_t i = 0; i < nbits; ++i) b[i] = bits[i] != 0;
    Personalization p{personalization < 0, personalization < 0 ? 0u : (unsigned)personalization};
    JAffine a = pedersen_hash(p, b).to_affine();
    a.u.to_bytes(out64);
    a.v.to_bytes(out64 + 32);
}
int masp_host_asset_identifier(const uint8_t* name, size_t len, uint8_t out32[32]) { return asset_identifier(out32, name, len) ? 0 : 1; }
int masp_host_asset_generator(const uint8_t id[32], uint8_t out32[32]) {
    JPoint p;
    if (!asset_generator(p, id)) return 1;
    p.to_bytes(out32);
    return 0;
}
int masp_host_value_commitment(const uint8_t id[32], uint64_t value, const uint8_t rcv[32], uint8_t out32[32], uint8_t uv64[64]) {
    JPoint g;
    if (!asset_generator(g, id)) return 1;
    JPoint cv = value_commitment(g, value, rcv);
    cv.to_bytes(out32);
    if (uv64) {
        JAffine a = cv.to_affine();
        a.u.to_bytes(uv64);
        a.v.to_bytes(uv64 + 32);
    }
    return 0;
}
// note commitment u-coordinate (cmu) from (asset id, value, diversifier, pk_d, rcm)
int masp_host_note_cmu(const uint8_t id[32], uint64_t value, const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t rcm[32],
                       uint8_t cmu32[32]) {
    JPoint g, gd, pk;
    if (!asset_generator(g, id) || !group_hash(gd, diversifier, 11, "MASP__gd") || !JPoint::from_bytes(pk, pk_d)) return 1;
    note_commitment(g, value, gd, pk, rcm).to_affine().u.to_bytes(cmu32);
    return 0;
}
// Note::cmu and Note::nf(&nk, position) (masp_primitives/src/sapling.rs) for n notes, dealt to `threads` host threads sixteen at a time;
// what masp_hip_sapling_note_nullifiers computes, and its other side in the tests.  status: the first check that fails (1 asset
// identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 nk), the note's outputs then zeros.  pk_d and nk are decoded as
// masp_host_note_cmu decodes pk_d: canonical and on the curve, no subgroup test.
int masp_host_sapling_note_nullifiers(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                      const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* nks,
                                      const uint64_t* positions, uint8_t* status, uint8_t* cmus_out, uint8_t* nfs_out, int threads) {
    if (n > ((size_t)1 << 22)) return MASP_HOST_E_INVALID;
    if (n == 0) return MASP_HOST_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !nks || !positions || !status || !nfs_out)
        return MASP_HOST_E_INVALID;
    (void)pedersen_windows();   // the lazily built tables, before the threads race for them
    (void)generators();
    auto one = [&](size_t i) {
        uint8_t* nf = nfs_out + 32 * i;
        memset(nf, 0, 32);
        if (cmus_out) memset(cmus_out + 32 * i, 0, 32);
        JPoint g, gd, pk, nk;
        uint8_t rcm[32];
        const uint8_t lead = lead_bytes[i], *r = rseeds + 32 * i;
        if (!asset_generator(g, asset_identifiers + 32 * i)) return 1;
        if (!group_hash(gd, diversifiers + 11 * i, 11, "MASP__gd")) return 2;
        if (!JPoint::from_bytes(pk, pk_ds + 32 * i)) return 3;
        if (lead == 1) {
            if (!rj_is_canonical(r)) return 4;   // jubjub::Fr::from_repr(rcm)
            memcpy(rcm, r, 32);
        } else if (lead == 2) {
            rseed_scalar(rcm, r, 4);
        } else {
            return 4;
        }
        if (!JPoint::from_bytes(nk, nks + 32 * i)) return 5;
        const JPoint cm = note_commitment(g, values[i], gd, pk, rcm);
        if (cmus_out) cm.to_affine().u.to_bytes(cmus_out + 32 * i);
        nullifier(nf, cm, positions[i], nk);   // (decoding accepts canonical encodings only: nk's bytes are the ones that came)
        return 0;
    };
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i0 = next.fetch_add(16);
            if (i0 >= n) return;
            for (size_t i = i0; i < std::min(n, i0 + 16); ++i) status[i] = (uint8_t)one(i);
        }
    };
    std::vector<std::thread> pool;
    if (n >= 64)   // (a few notes are not worth the threads' start)
        for (int k = 1; k < nt; ++k) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return MASP_HOST_OK;
}
int masp_host_merkle_hash(unsigned depth, const uint8_t lhs[32], const uint8_t rhs[32], uint8_t out32[32]) {
    Fr l, r;
    if (!Fr::from_bytes(l, lhs) || !Fr::from_bytes(r, rhs)) return 1;
    merkle_hash(depth, l, r).to_bytes(out32);
    return 0;
}
void masp_host_merkle_empty_roots(uint8_t out[33 * 32]) {
    const auto& e = merkle_empty_roots();
    for (int h = 0; h <= 32; ++h) memcpy(out + 32 * h, e[h].data(), 32);
}
// FrozenCommitmentTree::complete (masp_primitives/src/merkle_tree.rs:177-205) over a row of n nodes at height0, root() and path() (:207-251),
// a row's parents dealt to `threads` host threads; what masp_hip_merkle_tree_complete computes, and its other side in the tests
int masp_host_merkle_tree_complete(unsigned height0, size_t n, const uint8_t* row, uint8_t* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                                   uint8_t root32[32], size_t n_paths, const uint64_t* positions, uint8_t* paths_out, int64_t* bad_index,
                                   int threads) {
    if (bad_index) *bad_index = -1;
    if (height0 > 32 || !root32 || (n && !row) || n > ((size_t)1 << 22) || n > ((uint64_t)1 << (32 - height0)) || (n_paths && !positions) ||
        (n_paths && height0 < 32 && !paths_out))
        return MASP_HOST_E_INVALID;
    for (size_t p = 0; p < n_paths; ++p)
        if (positions[p] >= n) return MASP_HOST_E_INVALID;
    const unsigned depth = 32 - height0;
    size_t total = 0;
    if (n) {
        size_t width = n;
        for (unsigned i = 0; i < depth; ++i) {
            width += width & 1;
            total += width;
            width /= 2;
        }
        total += width;   // the node of level 32
    }
    if (n_nodes) *n_nodes = total;
    if (nodes_out && nodes_capacity < total) return MASP_HOST_E_CAPACITY;
    for (size_t i = 0; i < n; ++i) {
        Fr x;
        if (!Fr::from_bytes(x, row + 32 * i)) {
            if (bad_index) *bad_index = (int64_t)i;
            return MASP_HOST_E_INVALID;
        }
    }
    const auto& empty = merkle_empty_roots();
    if (n == 0) {
        memcpy(root32, empty[32].data(), 32);
        return MASP_HOST_OK;
    }
    (void)pedersen_windows();   // the lazily built table, before the threads race for it
    std::vector<uint8_t> own;
    uint8_t* t = nodes_out;
    if (!t) {
        own.resize(32 * total);
        t = own.data();
    }
    memcpy(t, row, 32 * n);
    const int nt = std::max(1, std::min<int>(threads, 256));
    size_t start = 0, width = n;
    for (unsigned i = 0; i < depth; ++i) {
        const unsigned level = height0 + i;
        if (width & 1) memcpy(t + 32 * (start + width++), empty[level].data(), 32);
        const size_t parents = width / 2;
        const uint8_t* src = t + 32 * start;
        uint8_t* dst = t + 32 * (start + width);
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (;;) {
                const size_t j0 = next.fetch_add(16);
                if (j0 >= parents) return;
                for (size_t j = j0; j < std::min(parents, j0 + 16); ++j) merkle_hash_bytes(level, src + 64 * j, src + 64 * j + 32).to_bytes(dst + 32 * j);
            }
        };
        std::vector<std::thread> pool;
        if (parents >= 64)   // (a narrow row is not worth the threads' start)
            for (int k = 1; k < nt; ++k) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        start += width;
        width = parents;
    }
    memcpy(root32, t + 32 * (total - 1), 32);
    for (size_t p = 0; p < n_paths; ++p) {
        size_t pos = positions[p], s = 0, w = n;
        for (unsigned i = 0; i < depth; ++i) {
            w += w & 1;
            memcpy(paths_out + 32 * (p * depth + i), t + 32 * (s + (pos ^ 1)), 32);   // (the sibling of a last, even node is the row's padding)
            s += w;
            w /= 2;
            pos /= 2;
        }
    }
    return MASP_HOST_OK;
}
// A block of n leaves at `start` of the depth-32 tree: level by level the complete nodes whose last leaf lies in the block, the first
// parent's left child out of the old frontier where the level starts at an odd index; what masp_hip_merkle_tree_append computes
int masp_host_merkle_tree_append(uint64_t start, const uint8_t frontier[32 * 32], size_t n, const uint8_t* row, uint8_t* nodes_out,
                                 size_t nodes_capacity, size_t* n_nodes, int64_t* bad_index, int threads) {
    if (bad_index) *bad_index = -1;
    const uint64_t full = (uint64_t)1 << 32, end = start + n;
    if (start > full || n > ((size_t)1 << 22) || end > full || (n && !row) || (n && start && !frontier)) return MASP_HOST_E_INVALID;
    size_t total = 0;
    for (unsigned h = 1; h <= 32; ++h) total += (size_t)((end >> h) - (start >> h));
    if (n_nodes) *n_nodes = total;
    if (!nodes_out) return MASP_HOST_OK;   // the count alone
    if (nodes_capacity < total) return MASP_HOST_E_CAPACITY;
    if (n == 0) return MASP_HOST_OK;
    Fr x;
    for (unsigned h = 0; h < 32; ++h)
        if (((start >> h) & 1) && !Fr::from_bytes(x, frontier + 32 * h)) {
            if (bad_index) *bad_index = -2 - (int64_t)h;
            return MASP_HOST_E_INVALID;
        }
    for (size_t i = 0; i < n; ++i)
        if (!Fr::from_bytes(x, row + 32 * i)) {
            if (bad_index) *bad_index = (int64_t)i;
            return MASP_HOST_E_INVALID;
        }
    (void)pedersen_windows();   // the lazily built table, before the threads race for it
    const int nt = std::max(1, std::min<int>(threads, 256));
    const uint8_t* src = row;
    uint8_t* dst = nodes_out;   // (every refusal is behind us)
    for (unsigned level = 0; level < 32; ++level) {
        const uint64_t c0 = start >> level, c1 = end >> level;
        const size_t parents = (size_t)((c1 >> 1) - (c0 >> 1)), odd = (size_t)(c0 & 1);
        if (!parents) break;   // (and none above)
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (;;) {
                const size_t t0 = next.fetch_add(16);
                if (t0 >= parents) return;
                for (size_t t = t0; t < std::min(parents, t0 + 16); ++t) {
                    const uint8_t* r = src + 32 * (2 * t + 1 - odd);
                    const uint8_t* l = (odd && t == 0) ? frontier + 32 * level : r - 32;
                    merkle_hash_bytes(level, l, r).to_bytes(dst + 32 * t);
                }
            }
        };
        std::vector<std::thread> pool;
        if (parents >= 64)   // (a narrow level is not worth the threads' start)
            for (int k = 1; k < nt; ++k) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        src = dst;
        dst += 32 * parents;
    }
    return MASP_HOST_OK;
}
// [k]P for P given as 32 bytes; (point decode / scalar multiplication / encode round trip)
int masp_host_jubjub_mul(const uint8_t p32[32], const uint8_t k32[32], uint8_t out32[32]) {
    JPoint p;
    if (!JPoint::from_bytes(p, p32)) return 1;
    p.mul(k32).to_bytes(out32);
    return 0;
}
// affine coordinates (u | v, 2 x 32 B LE) of an encoded point
int masp_host_point_uv(const uint8_t p32[32], uint8_t out64[64]) {
    JPoint p;
    if (!JPoint::from_bytes(p, p32)) return 1;
    JAffine a = p.to_affine();
    a.u.to_bytes(out64);
    a.v.to_bytes(out64 + 32);
    return 0;
}
// p + q, or p - q when subtract != 0 (value-commitment bookkeeping of the proving context)
int masp_host_jubjub_add(const uint8_t p32[32], const uint8_t q32[32], int subtract, uint8_t out32[32]) {
    JPoint p, q;
    if (!JPoint::from_bytes(p, p32) || !JPoint::from_bytes(q, q32)) return 1;
    p.add(subtract ? q.neg() : q).to_bytes(out32);
    return 0;
}
// acc + sum_i (+/-) points[i]  (n compressed points; subtract[i] != 0: that point is subtracted; subtract may be NULL): the value
// commitments of a chunk of descriptions in one call (SaplingProvingContext::cv_sum, sapling/prover.rs:154,205,272)
int masp_host_jubjub_sum(const uint8_t acc32[32], const uint8_t* points, size_t n, const uint8_t* subtract, uint8_t out32[32]) {
    JPoint acc;
    if (!JPoint::from_bytes(acc, acc32)) return 1;
    for (size_t i = 0; i < n; ++i) {
        JPoint q;
        if (!JPoint::from_bytes(q, points + 32 * i)) return 1;
        acc = acc.add(subtract && subtract[i] ? q.neg() : q);
    }
    acc.to_bytes(out32);
    return 0;
}
// leaf of the commitment tree for a spendable note: derives nk, ivk, g_d, pk_d exactly as spend_proof does and
// returns cmu (what the wallet already knows as the note commitment); also pk_d for callers that want the address
int masp_host_spend_leaf(const uint8_t ak[32], const uint8_t nsk[32], const uint8_t diversifier[11], const uint8_t rcm[32],
                         const uint8_t id[32], uint64_t value, uint8_t cmu32[32], uint8_t pk_d32[32]) {
    JPoint akp, g, gd;
    if (!JPoint::from_bytes(akp, ak) || !asset_generator(g, id)) return MASP_HOST_E_INVALID;
    if (!group_hash(gd, diversifier, 11, "MASP__gd")) return MASP_HOST_E_DIVERSIFIER;
    JPoint nk = generators().proof_generation_key.mul(nsk);
    uint8_t ivk[32];
    crh_ivk(ivk, akp, nk);
    JPoint pk = gd.mul(ivk);
    note_commitment(g, value, gd, pk, rcm).to_affine().u.to_bytes(cmu32);
    if (pk_d32) pk.to_bytes(pk_d32);
    return MASP_HOST_OK;
}
// AllowedConversion::from(I128Sum) (masp_primitives/src/convert.rs:86-118): generator = sum_i sign(v_i) * [|v_i| as u64] G_i with
// G_i the asset generator of identifier i, cofactor NOT cleared.  values: n x 16 bytes, little-endian two's-complement
// i128.  `abs as u64` keeps the low 64 bits, as the reference's cast does; i128::MIN has no absolute value (the reference
// panics "invalid conversion"): MASP_HOST_E_INVALID.
int masp_host_allowed_conversion(size_t n, const uint8_t* identifiers /* n x 32 */, const uint8_t* values /* n x 16 */, uint8_t generator_out[32]) {
    JPoint acc = JPoint::identity();
    for (size_t i = 0; i < n; ++i) {
        JPoint g;
        if (!asset_generator(g, identifiers + 32 * i)) return MASP_HOST_E_INVALID;
        const uint8_t* v = values + 16 * i;
        uint64_t lo = 0, hi = 0;
        for (int b = 0; b < 8; ++b) {
            lo |= (uint64_t)v[b] << (8 * b);
            hi |= (uint64_t)v[8 + b] << (8 * b);
        }
        const bool negative = (hi >> 63) != 0;
        if (negative) {
            if (hi == (1ull << 63) && lo == 0) return MASP_HOST_E_INVALID;  // i128::MIN
            lo = ~lo + 1;                                                     // low 64 bits of -value
        }
        uint8_t k[32] = {0};
        for (int b = 0; b < 8; ++b) k[b] = (uint8_t)(lo >> (8 * b));
        JPoint t = g.mul(k);
        acc = acc.add(negative ? t.neg() : t);
    }
    acc.to_bytes(generator_out);
    return MASP_HOST_OK;
}
// leaf of the convert tree: u of PedersenHash(NoteCommitment, repr(generator))  (convert.rs:39-64)
int masp_host_convert_cmu(const uint8_t generator[32], uint8_t out32[32]) {
    JPoint g;
    if (!JPoint::from_bytes(g, generator)) return 1;
    uint8_t b[32];
    g.to_bytes(b);
    pedersen_hash({true, 0}, bytes_to_bits_le(b, 32)).to_affine().u.to_bytes(out32);
    return 0;
}
// The two calls above for n_conv conversions whose terms lie in CSR form, dealt to `threads` host threads sixteen at a time; what
// masp_hip_sapling_allowed_conversions computes, and its other side in the tests.  The terms are summed as given (nothing merged, no zero
// dropped).  status: 1 a term's identifier has no generator, else 2 a term's value is i128::MIN; the conversion's outputs then zeros.
int masp_host_allowed_conversions(size_t n_conv, const uint64_t* term_offsets, size_t n_terms, const uint8_t* identifiers,
                                  const uint8_t* values, uint8_t* status, uint8_t* generators_out, uint8_t* cmus_out, int threads) {
    if (n_conv > ((size_t)1 << 22) || n_terms > ((size_t)1 << 24)) return MASP_HOST_E_INVALID;
    if (n_conv == 0) return MASP_HOST_OK;
    if (!term_offsets || !status || !cmus_out || (n_terms && (!identifiers || !values))) return MASP_HOST_E_INVALID;
    if (term_offsets[0] != 0 || term_offsets[n_conv] != n_terms) return MASP_HOST_E_INVALID;
    for (size_t c = 0; c < n_conv; ++c)
        if (term_offsets[c] > term_offsets[c + 1]) return MASP_HOST_E_INVALID;
    (void)pedersen_windows();   // the lazily built table, before the threads race for it
    auto one = [&](size_t c) {
        uint8_t* cmu = cmus_out + 32 * c;
        memset(cmu, 0, 32);
        if (generators_out) memset(generators_out + 32 * c, 0, 32);
        JPoint acc = JPoint::identity();
        int st = 0;
        for (uint64_t i = term_offsets[c]; i < term_offsets[c + 1]; ++i) {
            JPoint g;
            if (!asset_generator(g, identifiers + 32 * i)) {
                st = 1;
                continue;
            }
            const uint8_t* v = values + 16 * i;
            uint64_t lo = 0, hi = 0;
            for (int b = 0; b < 8; ++b) {
                lo |= (uint64_t)v[b] << (8 * b);
                hi |= (uint64_t)v[8 + b] << (8 * b);
            }
            const bool negative = (hi >> 63) != 0;
            if (negative) {
                if (hi == (1ull << 63) && lo == 0) {   // i128::MIN
                    if (!st) st = 2;
                    continue;
                }
                lo = ~lo + 1;   // low 64 bits of -value
            }
            if (st) continue;   // (the other terms only decide between 1 and 2)
            uint8_t k[32] = {0};
            for (int b = 0; b < 8; ++b) k[b] = (uint8_t)(lo >> (8 * b));
            const JPoint t = g.mul(k);
            acc = acc.add(negative ? t.neg() : t);
        }
        if (st) return st;
        uint8_t gb[32];
        acc.to_bytes(gb);
        if (generators_out) memcpy(generators_out + 32 * c, gb, 32);
        pedersen_hash({true, 0}, bytes_to_bits_le(gb, 32)).to_affine().u.to_bytes(cmu);
        return 0;
    };
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t c0 = next.fetch_add(16);
            if (c0 >= n_conv) return;
            for (size_t c = c0; c < std::min(n_conv, c0 + 16); ++c) status[c] = (uint8_t)one(c);
        }
    };
    std::vector<std::thread> pool;
    if (n_conv >= 64)   // (a few conversions are not worth the threads' start)
        for (int k = 1; k < nt; ++k) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return MASP_HOST_OK;
}
// ---- Sapling note encryption and trial decryption (note_encryption.h) --------------------------------
int masp_host_sapling_ka_agree(const uint8_t sk[32], const uint8_t p32[32], uint8_t out32[32]) {
    JPoint p;
    if (!JPoint::from_bytes(p, p32)) return MASP_HOST_E_INVALID;
    ka_agree(sk, p).to_bytes(out32);
    return MASP_HOST_OK;
}
// Diversifier::g_d: the group hash of a diversifier (personal "MASP__gd"), the base of its payment addresses
int masp_host_diversifier_base(const uint8_t diversifier[11], uint8_t out32[32]) {
    JPoint gd;
    if (!group_hash(gd, diversifier, 11, "MASP__gd")) return MASP_HOST_E_DIVERSIFIER;
    gd.to_bytes(out32);
    return MASP_HOST_OK;
}
void masp_host_kdf_sapling(const uint8_t secret[32], const uint8_t epk[32], uint8_t key32[32]) { kdf_sapling(key32, secret, epk); }
void masp_host_prf_expand(const uint8_t* sk, size_t sklen, const uint8_t* t, size_t tlen, uint8_t out64[64]) { prf_expand(out64, sk, sklen, t, tlen); }
void masp_host_sapling_rseed_scalar(const uint8_t rseed[32], int domain, uint8_t out32[32]) { rseed_scalar(out32, rseed, (uint8_t)domain); }
void masp_host_chacha20poly1305_encrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* plaintext, size_t n, uint8_t* ciphertext,
                                        uint8_t tag[16]) {
    aead_encrypt(ciphertext, tag, key, nonce, plaintext, n);
}
int masp_host_chacha20poly1305_decrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* ciphertext, size_t n, const uint8_t tag[16],
                                       uint8_t* plaintext) {
    return aead_decrypt(plaintext, key, nonce, ciphertext, n, tag) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
int masp_host_sapling_note_encrypt(const uint8_t esk[32], const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t plaintext[596],
                                   uint8_t epk_out[32], uint8_t enc_out[612]) {
    if (!rj_is_canonical(esk)) return MASP_HOST_E_INVALID;
    JPoint gd;
    if (!group_hash(gd, diversifier, 11, "MASP__gd")) return MASP_HOST_E_DIVERSIFIER;
    return note_encrypt(esk, diversifier, pk_d, plaintext, epk_out, enc_out) ? MASP_HOST_OK : MASP_HOST_E_INVALID;
}
int masp_host_sapling_try_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc[612], int lead_byte,
                                          uint8_t plaintext_out[596], uint8_t pk_d_out[32]) {
    if (!rj_is_canonical(ivk)) return MASP_HOST_E_INVALID;
    return try_note_decryption(ivk, epk, cmu, enc, lead_byte, plaintext_out, pk_d_out) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
int masp_host_sapling_finish_note_decryption(const uint8_t key[32], const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32],
                                             const uint8_t enc[612], int lead_byte, uint8_t plaintext_out[596], uint8_t pk_d_out[32]) {
    if (!rj_is_canonical(ivk)) return MASP_HOST_E_INVALID;
    return finish_note_decryption(key, ivk, epk, cmu, enc, lead_byte, plaintext_out, pk_d_out) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
// batch::try_note_decryption on `threads` host threads: per output the first ivk of the list that decrypts it
int masp_host_sapling_try_note_decryption_batch(size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks, const uint8_t* cmus,
                                                const uint8_t* encs, int lead_byte, int threads, int32_t* hit_ivk, uint8_t* plaintexts,
                                                uint8_t* pk_ds) {
    for (size_t k = 0; k < n_ivk; ++k)
        if (!rj_is_canonical(ivks + 32 * k)) return MASP_HOST_E_INVALID;
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t o = next.fetch_add(1);
            if (o >= n_out) return;
            hit_ivk[o] = -1;
            JPoint e;
            if (!JPoint::from_bytes(e, epks + 32 * o)) continue;
            for (size_t k = 0; k < n_ivk; ++k) {
                uint8_t secret[32], key[32];
                ka_agree(ivks + 32 * k, e).to_bytes(secret);
                kdf_sapling(key, secret, epks + 32 * o);
                if (finish_note_decryption(key, ivks + 32 * k, epks + 32 * o, cmus + 32 * o, encs + ENC_CIPHERTEXT_SIZE * o, lead_byte,
                                           plaintexts + NOTE_PLAINTEXT_SIZE * o, pk_ds + 32 * o)) {
                    hit_ivk[o] = (int32_t)k;
                    break;
                }
            }
        }
    };
    (void)generators();          // the lazily built tables, before the threads race for them
    (void)pedersen_windows();
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return MASP_HOST_OK;
}
int masp_host_sapling_try_compact_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc84[84],
                                                  int lead_byte, uint8_t plaintext84_out[84], uint8_t pk_d_out[32]) {
    if (!rj_is_canonical(ivk)) return MASP_HOST_E_INVALID;
    return try_compact_note_decryption(ivk, epk, cmu, enc84, lead_byte, plaintext84_out, pk_d_out) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
// batch::try_compact_note_decryption on `threads` host threads: per output the first ivk of the list for which the whole check succeeds;
// n_candidates (may be null): the pairs whose epk decodes and whose decrypted byte 0 is lead_byte
int masp_host_sapling_try_compact_note_decryption_batch(size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks, const uint8_t* cmus,
                                                        const uint8_t* encs84, int lead_byte, int threads, int32_t* hit_ivk, uint8_t* plaintexts84,
                                                        uint8_t* pk_ds, uint64_t* n_candidates) {
    for (size_t k = 0; k < n_ivk; ++k)
        if (!rj_is_canonical(ivks + 32 * k)) return MASP_HOST_E_INVALID;
    std::atomic<size_t> next{0};
    std::atomic<uint64_t> candidates{0};
    auto work = [&] {
        uint64_t mine = 0;
        for (;;) {
            const size_t o = next.fetch_add(1);
            if (o >= n_out) break;
            hit_ivk[o] = -1;
            JPoint e;
            if (!JPoint::from_bytes(e, epks + 32 * o)) continue;
            for (size_t k = 0; k < n_ivk; ++k) {   // (every ivk: the count is over all pairs, the result the first success)
                uint8_t secret[32], key[32], pt[COMPACT_NOTE_SIZE], pk[32];
                ka_agree(ivks + 32 * k, e).to_bytes(secret);
                kdf_sapling(key, secret, epks + 32 * o);
                bool cand = false;
                const bool ok = finish_compact_note_decryption(key, ivks + 32 * k, epks + 32 * o, cmus + 32 * o, encs84 + COMPACT_NOTE_SIZE * o,
                                                               lead_byte, pt, pk, &cand);
                mine += cand;
                if (ok && hit_ivk[o] < 0) {
                    hit_ivk[o] = (int32_t)k;
                    memcpy(plaintexts84 + COMPACT_NOTE_SIZE * o, pt, COMPACT_NOTE_SIZE);
                    memcpy(pk_ds + 32 * o, pk, 32);
                }
            }
        }
        candidates += mine;
    };
    (void)generators();          // the lazily built tables, before the threads race for them
    (void)pedersen_windows();
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (n_candidates) *n_candidates = candidates.load();
    return MASP_HOST_OK;
}
// ---- the sender's side: out_ciphertext and recovery with an ovk (note_encryption.h) --------------------------------
void masp_host_prf_ock(const uint8_t ovk[32], const uint8_t cv[32], const uint8_t cmu[32], const uint8_t epk[32], uint8_t ock_out[32]) {
    prf_ock(ock_out, ovk, cv, cmu, epk);
}
void masp_host_sapling_encrypt_outgoing(const uint8_t ock[32], const uint8_t pk_d[32], const uint8_t esk[32], uint8_t c_out[80]) {
    encrypt_outgoing(c_out, ock, pk_d, esk);
}
int masp_host_sapling_try_output_recovery_with_ock(const uint8_t ock[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc[612],
                                                   const uint8_t c_out[80], int lead_byte, uint8_t plaintext_out[596], uint8_t pk_d_out[32]) {
    return try_output_recovery_with_ock(ock, epk, cmu, enc, c_out, lead_byte, plaintext_out, pk_d_out) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
int masp_host_sapling_try_output_recovery(const uint8_t ovk[32], const uint8_t cv[32], const uint8_t epk[32], const uint8_t cmu[32],
                                          const uint8_t enc[612], const uint8_t c_out[80], int lead_byte, uint8_t plaintext_out[596],
                                          uint8_t pk_d_out[32]) {
    return try_output_recovery(ovk, cv, epk, cmu, enc, c_out, lead_byte, plaintext_out, pk_d_out) ? MASP_HOST_OK : MASP_HOST_E_NO_NOTE;
}
// try_sapling_output_recovery over outputs x ovks on `threads` host threads: per output the first ovk of the list that recovers it
int masp_host_sapling_try_output_recovery_batch(size_t n_ovk, const uint8_t* ovks, size_t n_out, const uint8_t* cvs, const uint8_t* epks,
                                                const uint8_t* cmus, const uint8_t* encs, const uint8_t* c_outs, int lead_byte, int threads,
                                                int32_t* hit_ovk, uint8_t* plaintexts, uint8_t* pk_ds) {
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t o = next.fetch_add(1);
            if (o >= n_out) return;
            hit_ovk[o] = -1;
            for (size_t k = 0; k < n_ovk; ++k)
                if (try_output_recovery(ovks + 32 * k, cvs + 32 * o, epks + 32 * o, cmus + 32 * o, encs + ENC_CIPHERTEXT_SIZE * o,
                                        c_outs + OUT_CIPHERTEXT_SIZE * o, lead_byte, plaintexts + NOTE_PLAINTEXT_SIZE * o, pk_ds + 32 * o)) {
                    hit_ovk[o] = (int32_t)k;
                    break;
                }
        }
    };
    (void)generators();          // the lazily built tables, before the threads race for them
    (void)pedersen_windows();
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return MASP_HOST_OK;
}
// SaplingOutputInfo::build without the proof for n outputs, dealt to `threads` host threads sixteen at a time; what
// masp_hip_sapling_build_outputs computes, and its other side in the tests.  Composed from what the one-output calls are made of:
// value_commitment, note_commitment, note_encrypt, prf_ock, encrypt_outgoing.
int masp_host_sapling_build_outputs(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                    const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* esks,
                                    const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* ovk_flags,
                                    const uint8_t* out_randoms, uint8_t* status, uint8_t* cvs_out, uint8_t* cmus_out, uint8_t* epks_out,
                                    uint8_t* encs_out, uint8_t* couts_out, int threads) {
    if (n > ((size_t)1 << 20)) return MASP_HOST_E_INVALID;
    if (n == 0) return MASP_HOST_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !rcvs || !ovks || !status || !cvs_out || !cmus_out ||
        !epks_out || !encs_out || !couts_out)
        return MASP_HOST_E_INVALID;
    if (!esks && memchr(lead_bytes, 1, n)) return MASP_HOST_E_INVALID;                          // a lead byte 1 needs its esk
    if (!out_randoms && ovk_flags && memchr(ovk_flags, 0, n)) return MASP_HOST_E_INVALID;       // an absent ovk needs its 96 bytes
    (void)pedersen_windows();   // the lazily built tables, before the threads race for them
    (void)generators();
    auto one = [&](size_t i) {
        uint8_t *cv = cvs_out + 32 * i, *cmu = cmus_out + 32 * i, *epk = epks_out + 32 * i, *enc = encs_out + ENC_CIPHERTEXT_SIZE * i,
                *cout = couts_out + OUT_CIPHERTEXT_SIZE * i;
        auto refuse = [&](int s) {
            memset(cv, 0, 32);
            memset(cmu, 0, 32);
            memset(epk, 0, 32);
            memset(enc, 0, ENC_CIPHERTEXT_SIZE);
            memset(cout, 0, OUT_CIPHERTEXT_SIZE);
            return s;
        };
        JPoint g, gd, pk;
        uint8_t rcm[32], esk[32], pt[NOTE_PLAINTEXT_SIZE];
        const uint8_t lead = lead_bytes[i], *id = asset_identifiers + 32 * i, *d = diversifiers + 11 * i, *pkd = pk_ds + 32 * i, *r = rseeds + 32 * i;
        if (!asset_generator(g, id)) return refuse(1);
        if (!group_hash(gd, d, 11, "MASP__gd")) return refuse(2);
        if (!JPoint::from_bytes(pk, pkd)) return refuse(3);
        if (lead == 1) {
            if (!rj_is_canonical(r)) return refuse(4);   // jubjub::Fr::from_repr(rcm)
            if (!rj_is_canonical(esks + 32 * i)) return refuse(5);
            memcpy(rcm, r, 32);
            memcpy(esk, esks + 32 * i, 32);
        } else if (lead == 2) {
            rseed_scalar(rcm, r, 4);   // Note::rcm
            rseed_scalar(esk, r, 5);   // Note::derive_esk
        } else {
            return refuse(4);
        }
        if (!rj_is_canonical(rcvs + 32 * i)) return refuse(6);
        value_commitment(g, values[i], rcvs + 32 * i).to_bytes(cv);
        note_commitment(g, values[i], gd, pk, rcm).to_affine().u.to_bytes(cmu);
        pt[0] = lead;
        memcpy(pt + 1, d, 11);
        for (int k = 0; k < 8; ++k) pt[12 + k] = (uint8_t)(values[i] >> (8 * k));
        memcpy(pt + 20, id, 32);
        memcpy(pt + 52, r, 32);
        if (memos) {
            memcpy(pt + 84, memos + 512 * i, 512);
        } else {
            memset(pt + 84, 0, 512);
            pt[84] = 0xf6;   // the empty memo
        }
        (void)note_encrypt(esk, d, pkd, pt, epk, enc);   // (g_d and pk_d were decoded above)
        if (!ovk_flags || ovk_flags[i]) {
            uint8_t ock[32];
            prf_ock(ock, ovks + 32 * i, cv, cmu, epk);
            encrypt_outgoing(cout, ock, pkd, esk);
        } else {
            const uint8_t* rnd = out_randoms + 96 * i;
            encrypt_outgoing(cout, rnd, rnd + 32, rnd + 64);
        }
        return 0;
    };
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i0 = next.fetch_add(16);
            if (i0 >= n) return;
            for (size_t i = i0; i < std::min(n, i0 + 16); ++i) status[i] = (uint8_t)one(i);
        }
    };
    std::vector<std::thread> pool;
    if (n >= 64)   // (a few outputs are not worth the threads' start)
        for (int k = 1; k < nt; ++k) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return MASP_HOST_OK;
}
}  // extern "C"

// ---- spend descriptions and RedJubjub signatures in batches --------------------------------------------
namespace {
// a + b mod r_J, both below r_J, 32 little-endian bytes each
void rj_add(uint8_t out[32], const uint8_t a[32], const uint8_t b[32]) {
    uint64_t x[4], y[4], d[4];
    memcpy(x, a, 32);
    memcpy(y, b, 32);
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) {
        c += (unsigned __int128)x[i] + y[i];
        x[i] = (uint64_t)c;
        c >>= 64;
    }   // (below 2 r_J < 2^253: no carry out)
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 t = (unsigned __int128)x[i] - RJ[i] - (uint64_t)borrow;
        d[i] = (uint64_t)t;
        borrow = (t >> 64) & 1;
    }
    memcpy(out, borrow ? x : d, 32);
}
// a b mod r_J: the 512-bit product through rj_from_bytes_wide
void rj_mul(uint8_t out[32], const uint8_t a[32], const uint8_t b[32]) {
    uint64_t x[4], y[4], p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    memcpy(x, a, 32);
    memcpy(y, b, 32);
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) {
            c += (unsigned __int128)x[i] * y[j] + p[i + j];
            p[i + j] = (uint64_t)c;
            c >>= 64;
        }
        p[i + 4] = (uint64_t)c;
    }
    uint8_t wide[64];
    memcpy(wide, p, 64);
    rj_from_bytes_wide(out, wide);
}
// H*(a | b | c) mod r_J (masp_primitives/src/sapling/util.rs: hash_to_scalar, personal "MASP__RedJubjubH")
void h_star(uint8_t out[32], const uint8_t* a, size_t alen, const uint8_t* b, const uint8_t* c) {
    uint8_t wide[64];
    Blake2b h((const uint8_t*)"MASP__RedJubjubH", 64);
    h.update(a, alen);
    h.update(b, 32);
    h.update(c, 32);
    h.finalize(wide);
    rj_from_bytes_wide(out, wide);
}
// one(i) -> status[i] for i < n, dealt to `threads` host threads sixteen at a time
template <class F>
void deal(size_t n, int threads, uint8_t* status, F one) {
    const int nt = std::max(1, std::min<int>(threads, 256));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i0 = next.fetch_add(16);
            if (i0 >= n) return;
            for (size_t i = i0; i < std::min(n, i0 + 16); ++i) status[i] = (uint8_t)one(i);
        }
    };
    std::vector<std::thread> pool;
    if (n >= 64)   // (a few items are not worth the threads' start)
        for (int k = 1; k < nt; ++k) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}
}  // namespace

extern "C" {
// spend_sig_internal (masp_primitives/src/sapling.rs:167-195: PrivateKey::randomize, PublicKey::from_private, PrivateKey::sign of
// sapling/redjubjub.rs:121-160) over either basepoint for n items; what masp_hip_redjubjub_sign_batch computes, and its other side in the
// tests.  rsk = 0 is signed with, as the reference does.
int masp_host_redjubjub_sign_batch(size_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes, const uint8_t* kinds,
                                   const uint8_t* randoms, uint8_t* status, uint8_t* vks_out, uint8_t* sigs_out, int threads) {
    if (n > ((size_t)1 << 20)) return MASP_HOST_E_INVALID;
    if (n == 0) return MASP_HOST_OK;
    if (!sks || !sighashes || !kinds || !randoms || !status || !sigs_out) return MASP_HOST_E_INVALID;
    for (size_t i = 0; i < n; ++i)
        if (kinds[i] > 1) return MASP_HOST_E_INVALID;
    (void)generators();   // the lazily built tables, before the threads race for them
    deal(n, threads, status, [&](size_t i) {
        uint8_t* sig = sigs_out + 64 * i;
        memset(sig, 0, 64);
        if (vks_out) memset(vks_out + 32 * i, 0, 32);
        const uint8_t *sk = sks + 32 * i, *m = sighashes + 32 * i;
        if (!rj_is_canonical(sk)) return 1;   // PrivateKey::read
        uint8_t rsk[32], vk[32], r[32], c[32], cr[32];
        memcpy(rsk, sk, 32);
        if (alphas) {
            if (!rj_is_canonical(alphas + 32 * i)) return 2;
            rj_add(rsk, sk, alphas + 32 * i);
        }
        const JPoint& g = kinds[i] ? generators().value_commitment_randomness : generators().spending_key;
        g.mul(rsk).to_bytes(vk);
        h_star(r, randoms + 80 * i, 80, vk, m);
        g.mul(r).to_bytes(sig);
        h_star(c, sig, 32, vk, m);
        rj_mul(cr, c, rsk);
        rj_add(sig + 32, r, cr);
        if (vks_out) memcpy(vks_out + 32 * i, vk, 32);
        return 0;
    });
    return MASP_HOST_OK;
}
// What the builder puts around a Spend proof for n spends; what masp_hip_sapling_build_spends computes, and its other side in the tests.
// Composed from what the one-item calls are made of: value_commitment, note_commitment, nullifier.
int masp_host_sapling_build_spends(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                   const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* aks,
                                   const uint8_t* nsks, const uint8_t* ars, const uint8_t* rcvs, const uint64_t* positions, uint8_t* status,
                                   uint8_t* cvs_out, uint8_t* rks_out, uint8_t* nfs_out, uint8_t* cmus_out, uint8_t* nks_out, int threads) {
    if (n > ((size_t)1 << 20)) return MASP_HOST_E_INVALID;
    if (n == 0) return MASP_HOST_OK;
    if (!asset_identifiers || !values || !diversifiers || !pk_ds || !lead_bytes || !rseeds || !aks || !nsks || !ars || !rcvs || !positions ||
        !status || !cvs_out || !rks_out || !nfs_out)
        return MASP_HOST_E_INVALID;
    (void)pedersen_windows();   // the lazily built tables, before the threads race for them
    (void)generators();
    deal(n, threads, status, [&](size_t i) {
        memset(cvs_out + 32 * i, 0, 32);
        memset(rks_out + 32 * i, 0, 32);
        memset(nfs_out + 32 * i, 0, 32);
        if (cmus_out) memset(cmus_out + 32 * i, 0, 32);
        if (nks_out) memset(nks_out + 32 * i, 0, 32);
        JPoint g, gd, pk, ak;
        uint8_t rcm[32], nkb[32];
        const uint8_t lead = lead_bytes[i], *r = rseeds + 32 * i;
        if (!asset_generator(g, asset_identifiers + 32 * i)) return 1;
        if (!group_hash(gd, diversifiers + 11 * i, 11, "MASP__gd")) return 2;
        if (!JPoint::from_bytes(pk, pk_ds + 32 * i)) return 3;
        if (lead == 1) {
            if (!rj_is_canonical(r)) return 4;   // jubjub::Fr::from_repr(rcm)
            memcpy(rcm, r, 32);
        } else if (lead == 2) {
            rseed_scalar(rcm, r, 4);
        } else {
            return 4;
        }
        if (!JPoint::from_bytes(ak, aks + 32 * i)) return 5;
        if (ak.mul_by_cofactor().is_identity()) return 6;   // the Spend circuit: ak is not of small order
        if (!rj_is_canonical(nsks + 32 * i)) return 7;
        if (!rj_is_canonical(ars + 32 * i)) return 8;
        if (!rj_is_canonical(rcvs + 32 * i)) return 9;
        const JPoint nk = generators().proof_generation_key.mul(nsks + 32 * i);
        nk.to_bytes(nkb);
        ak.add(generators().spending_key.mul(ars + 32 * i)).to_bytes(rks_out + 32 * i);
        value_commitment(g, values[i], rcvs + 32 * i).to_bytes(cvs_out + 32 * i);
        const JPoint cm = note_commitment(g, values[i], gd, pk, rcm);
        if (cmus_out) cm.to_affine().u.to_bytes(cmus_out + 32 * i);
        nullifier(nfs_out + 32 * i, cm, positions[i], nk);
        if (nks_out) memcpy(nks_out + 32 * i, nkb, 32);
        return 0;
    });
    return MASP_HOST_OK;
}
}  // extern "C"
