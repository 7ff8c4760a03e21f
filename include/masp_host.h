/* masp_host.h — C ABI of libmasp_host.so: the host side of the proving path that PRECEDES the Groth16 prover.
 *
 * What `SaplingProvingContext::{spend_proof, output_proof, convert_proof}` do before they call `create_random_proof`
 * (/root/reference/masp_proofs/src/sapling/prover.rs:51-113, :163-198, :214-248): native key / commitment / nullifier derivation
 * and `Circuit::synthesize` (/root/reference/masp_proofs/src/circuit/sapling.rs:139-596, circuit/convert.rs:29-128) into
 * (input_assignment, aux_assignment) — plus the static R1CS of each circuit (what bellperson's KeypairAssembly collects), the
 * self-verification of sapling/prover.rs:148,266 (`verify_proof` with the PreparedVerifyingKey of lib.rs:391-393) and the native
 * primitives the reference's vectors pin (tests/golden/).  A Rust caller keeps its own synthesis and needs none
 * of this; a C / C++ caller feeds masp_hip_prove_batch (include/masp_hip.h) from here.  No GPU code: plain C++ behind C linkage.
 *
 * Conventions as in masp_hip.h: integer return codes, caller-owned buffers, no exceptions across the boundary.  Field elements are
 * 32-byte little-endian canonical values unless a parameter says Montgomery; Jubjub points are their 32-byte `to_bytes()` encoding.
 * Thread-safe: every function may be called from any number of threads (handles are immutable once built).
 * The definitions in masp_amd/csrc/host/host_api.cpp include this header, so the compiler checks every signature;
 * tests/test_capi_symbols.py checks the header against `nm -D`. */
#ifndef MASP_HOST_H
#define MASP_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MASP_HOST_OK 0
#define MASP_HOST_E_INVALID 1       /* an argument is not a canonical scalar / a point on the curve / a field element */
#define MASP_HOST_E_DIVERSIFIER 2   /* the diversifier has no group hash: the reference's Err(()) at sapling/prover.rs:84 */
#define MASP_HOST_E_SYNTHESIS 3     /* bellperson's SynthesisError */
#define MASP_HOST_E_UNSATISFIED 4   /* check & 1: a constraint does not hold */
#define MASP_HOST_E_NO_NOTE 5       /* trial decryption: the output is not a note of this key (the reference's None) */
#define MASP_HOST_E_CAPACITY 6      /* an output buffer of the caller is too small: the call says how much it needs */

/* `kind` everywhere: 0 Spend, 1 Output, 2 Convert (= MASP_HIP_SPEND / _OUTPUT / _CONVERT) */

/* ---- the static R1CS of a circuit (-> masp_hip_r1cs) ---- */
void* masp_host_circuit_setup(int kind);                 /* handle, or NULL */
void masp_host_circuit_free(void* h);
/* out[6]: n_inputs, n_aux, n_constraints, nnz(A), nnz(B), nnz(C) */
void masp_host_circuit_counts(void* h, uint32_t* out);
/* matrix mi (0 A, 1 B, 2 C) as CSR: rowptr[n_constraints + 1], col[nnz] (input i -> i, aux j -> n_inputs + j), coef[nnz][32] */
void masp_host_circuit_matrix(void* h, int mi, uint32_t* rowptr, uint32_t* col, uint8_t* coef);
/* bellperson's TestConstraintSystem::hash() of the circuit as 64 hex digits + NUL (pinned: circuit/sapling.rs:733,1026, convert.rs:221) */
void masp_host_circuit_hash(void* h, char* out65);

/* ---- witness generation.  check & 1: also record the constraints and fail with MASP_HOST_E_UNSATISFIED if one is violated;
 * check & 2: write the aux assignment as Montgomery residues (four little-endian u64 limbs: masp_hip_job::aux_form =
 * MASP_HIP_AUX_MONTGOMERY), straight into `aux` when it is 8-byte aligned.  rcm = note.rcm() as 32 bytes. ---- */
int masp_host_spend_assignment(const uint8_t ak[32], const uint8_t nsk[32], const uint8_t diversifier[11], const uint8_t rcm[32],
                               const uint8_t ar[32], const uint8_t asset_identifier[32], uint64_t value, const uint8_t anchor[32],
                               const uint8_t* path_siblings /* 32 x 32, leaf level first */, uint64_t position, const uint8_t rcv[32], int check,
                               uint8_t* inputs /* 8 x 32 */, uint8_t* aux /* 100497 x 32 */, uint8_t cv_out[32], uint8_t rk_out[32],
                               uint8_t nf_out[32]);
int masp_host_output_assignment(const uint8_t esk[32], const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t rcm[32],
                                const uint8_t asset_identifier[32], uint64_t value, const uint8_t rcv[32], int check,
                                uint8_t* inputs /* 6 x 32 */, uint8_t* aux /* 30896 x 32 */, uint8_t cv_out[32]);
/* generator: the AllowedConversion's asset generator (masp_primitives/src/convert.rs:23-29) */
int masp_host_convert_assignment(const uint8_t generator[32], uint64_t value, const uint8_t anchor[32], const uint8_t* path_siblings,
                                 uint64_t position, const uint8_t rcv[32], int check, uint8_t* inputs /* 4 x 32 */,
                                 uint8_t* aux /* 47322 x 32 */, uint8_t cv_out[32]);
/* n Montgomery residues (as `check & 2` writes them) -> canonical bytes */
void masp_host_fr_from_montgomery(const uint8_t* in, uint8_t* out, size_t n);

/* Several witnesses per call: their Merkle blocks are synthesised in lockstep (one shared inversion per window across the group:
 * ~2x the witnesses per second and thread).  A job = the arguments of the single-witness call + its return code; the call returns
 * the number of jobs whose rc is not MASP_HOST_OK.  A caller gives each of its threads a group of ~16 jobs. */
typedef struct masp_host_spend_job {
    const uint8_t *ak, *nsk, *diversifier, *rcm, *ar, *asset_identifier;
    uint64_t value;
    const uint8_t *anchor, *path_siblings;
    uint64_t position;
    const uint8_t* rcv;
    uint8_t *inputs, *aux, *cv_out, *rk_out, *nf_out;
    int rc;
} masp_host_spend_job;
typedef struct masp_host_convert_job {
    const uint8_t* generator;
    uint64_t value;
    const uint8_t *anchor, *path_siblings;
    uint64_t position;
    const uint8_t* rcv;
    uint8_t *inputs, *aux, *cv_out;
    int rc;
} masp_host_convert_job;
int masp_host_spend_assignments(size_t n, masp_host_spend_job* jobs, int check);
int masp_host_convert_assignments(size_t n, masp_host_convert_job* jobs, int check);

/* ---- Groth16 verification on the host (sapling/prover.rs:148,266; batched: sapling/verifier/batch.rs:24-31) ---- */
void* masp_host_vk_prepare(const uint8_t* params, size_t len);   /* Parameters bytes: only the verifying-key prefix is read */
void masp_host_vk_free(void* h);
/* public_inputs: n_public x 32, excluding ONE.  1 valid, 0 invalid, < 0 malformed */
int masp_host_vk_verify(const void* h, const uint8_t proof[192], const uint8_t* public_inputs, uint32_t n_public);
/* `Proof::read` alone (sapling/verifier/batch.rs:85,125,154): 1 if the proof's three points decode as it requires (canonical, on the
 * curve, in the prime-order subgroups, not the identity), else 0 */
int masp_host_proof_read(const uint8_t proof[192]);
/* n proofs, one random linear combination with the caller's z (n x 16 bytes).  1 all valid, 0 at least one is not, < 0 malformed */
int masp_host_vk_verify_batch(const void* h, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint32_t n_public,
                              const uint8_t* z);
/* the GPU verifier's Miller-loop programs on a host interpreter against this library's own Miller loop, for one pair (P 96 B, Q 192 B
 * uncompressed); 0 = equal.  stats (may be NULL): 15 words, see host_api.cpp */
int masp_host_pairing_program_selftest(const uint8_t* p96, const uint8_t* q192, uint32_t* stats);
/* The final exponentiation's programs (product, squaring, Frobenius, Frobenius^2, the two halves of the inversion) run on the host
 * interpreter in the device kernel's order on f (in576: 12 Fp, 48 bytes big-endian each) and compared with the library's own final
 * exponentiation.  0 = equal, out576 = f^(3 (p^12 - 1) / r); 2 = f has norm zero, the branch in front of the inversion was taken:
 * the verdict is "invalid" (out576 = zeros); 1 / 3 = the programs are wrong; -1 = a coefficient >= p.  stats (may be NULL, 32 words):
 * ops / steps / steps with products / products / slots of each of the six, then the slots of the set and their bytes of LDS. */
int masp_host_final_exp_program_selftest(const uint8_t* in576, uint8_t* out576, uint32_t* stats);

/* ---- native primitives (pinned by the reference's vectors: tests/golden/) ---- */
/* which: 0 proof_generation_key, 1 note_commitment_randomness, 2 nullifier_position, 3 value_commitment_randomness, 4 spending_key,
 * 5..10 pedersen[0..5]; out: u | v */
void masp_host_generator(int which, uint8_t out64[64]);
/* personalization: -1 NoteCommitment, else MerkleTree(depth); bits: one byte per bit; out: u | v */
void masp_host_pedersen_hash(int personalization, const uint8_t* bits, size_t nbits, uint8_t out64[64]);
int masp_host_asset_identifier(const uint8_t* name, size_t len, uint8_t out32[32]);
int masp_host_asset_generator(const uint8_t id[32], uint8_t out32[32]);
int masp_host_value_commitment(const uint8_t id[32], uint64_t value, const uint8_t rcv[32], uint8_t out32[32], uint8_t uv64[64]);
int masp_host_note_cmu(const uint8_t id[32], uint64_t value, const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t rcm[32],
                       uint8_t cmu32[32]);
/* Note::cmu and Note::nf(&nk, position) (masp_primitives/src/sapling.rs) for n <= 2^22 notes on `threads` host threads: the arguments and
 * results of masp_hip_sapling_note_nullifiers (include/masp_hip.h) without the context.  asset_identifiers, pk_ds, rseeds (rcm for lead
 * byte 1, rseed for lead byte 2), nks, cmus_out (may be NULL), nfs_out: n x 32; diversifiers: n x 11; lead_bytes, status: n.
 * status[i]: 0, or the first check that fails: 1 the asset identifier has no generator, 2 the diversifier has no g_d, 3 pk_d does not decode,
 * 4 the lead byte is neither 1 nor 2 or rcm >= r_J, 5 nk does not decode; the note's outputs are then zeros and nothing else changes.
 * pk_d and nk are decoded as masp_host_note_cmu decodes pk_d (canonical, on the curve) and hashed as the given bytes; the reference's
 * types make both points of the prime-order subgroup, which is NOT tested here.  MASP_HOST_E_INVALID: a NULL array with n > 0, n > 2^22. */
int masp_host_sapling_note_nullifiers(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                      const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* nks,
                                      const uint64_t* positions, uint8_t* status, uint8_t* cmus_out, uint8_t* nfs_out, int threads);
/* Output descriptions without their proofs (SaplingOutputInfo::build of masp_primitives/src/transaction/components/sapling/builder.rs) for
 * n <= 2^20 outputs on `threads` host threads: the arguments and results of masp_hip_sapling_build_outputs (include/masp_hip.h) without the
 * context, composed from masp_host_value_commitment, masp_host_note_cmu, masp_host_sapling_note_encrypt, masp_host_prf_ock and
 * masp_host_sapling_encrypt_outgoing.  No randomness is drawn.  memos, ovk_flags, out_randoms (no flag is 0) and esks (no lead byte is 1)
 * may be NULL, as there.  status[i]: 0, or the first check that fails: 1 the asset identifier has no generator, 2 the diversifier has no g_d,
 * 3 pk_d does not decode, 4 the lead byte is neither 1 nor 2 or rcm >= r_J, 5 lead byte 1 with esk >= r_J, 6 rcv >= r_J; the output's five
 * outputs are then zeros and nothing else changes.  A zero esk is not refused; pk_d's subgroup membership is not tested.
 * MASP_HOST_E_INVALID: any other NULL array with n > 0, n > 2^20; nothing is written. */
int masp_host_sapling_build_outputs(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                    const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* esks,
                                    const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* ovk_flags,
                                    const uint8_t* out_randoms, uint8_t* status, uint8_t* cvs_out, uint8_t* cmus_out, uint8_t* epks_out,
                                    uint8_t* encs_out, uint8_t* couts_out, int threads);
/* RedJubjub signatures (spend_sig_internal of masp_primitives/src/sapling.rs over sapling/redjubjub.rs:121-160) for n <= 2^20 items on
 * `threads` host threads: the arguments and results of masp_hip_redjubjub_sign_batch (include/masp_hip.h) without the context.  No
 * randomness is drawn: randoms holds the reference's 80 bytes T per item.  alphas and vks_out may be NULL.  kinds: 0 spend authorisation,
 * 1 binding; anything else MASP_HOST_E_INVALID before any work.  status[i]: 0, 1 sk >= r_J, 2 alpha >= r_J; the item's outputs are then
 * zeros and nothing else changes.  rsk = 0 is not refused.  MASP_HOST_E_INVALID: any other NULL array with n > 0, n > 2^20. */
int masp_host_redjubjub_sign_batch(size_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes, const uint8_t* kinds,
                                   const uint8_t* randoms, uint8_t* status, uint8_t* vks_out, uint8_t* sigs_out, int threads);
/* Spend descriptions without their proofs (the builder of masp_primitives/src/transaction/components/sapling/builder.rs) for n <= 2^20
 * spends on `threads` host threads: the arguments and results of masp_hip_sapling_build_spends (include/masp_hip.h) without the context.
 * cmus_out and nks_out may be NULL.  status[i]: 0, or the first check that fails: 1 to 4 as in masp_host_sapling_note_nullifiers, 5 ak
 * does not decode, 6 [8] ak is the identity, 7 nsk >= r_J, 8 ar >= r_J, 9 rcv >= r_J; the spend's outputs are then zeros and nothing else
 * changes.  Beyond check 6 the subgroup membership of ak is not tested, nor is pk_d's.  MASP_HOST_E_INVALID: any other NULL array with
 * n > 0, n > 2^20; nothing is written. */
int masp_host_sapling_build_spends(size_t n, const uint8_t* asset_identifiers, const uint64_t* values, const uint8_t* diversifiers,
                                   const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds, const uint8_t* aks,
                                   const uint8_t* nsks, const uint8_t* ars, const uint8_t* rcvs, const uint64_t* positions, uint8_t* status,
                                   uint8_t* cvs_out, uint8_t* rks_out, uint8_t* nfs_out, uint8_t* cmus_out, uint8_t* nks_out, int threads);
int masp_host_merkle_hash(unsigned depth, const uint8_t lhs[32], const uint8_t rhs[32], uint8_t out32[32]);
/* empty_root(0..32) of the commitment tree, 33 x 32 bytes: the uncommitted leaf 1 and the roots of the empty subtrees above it */
void masp_host_merkle_empty_roots(uint8_t out[33 * 32]);
/* FrozenCommitmentTree (masp_primitives/src/merkle_tree.rs:105-256) on the host, the arguments and results of masp_hip_merkle_tree_complete
 * (include/masp_hip.h) without the context and with the number of host threads a row's parents are dealt to.  MASP_HOST_E_INVALID: an
 * argument out of range, a position >= n, or a node that is not canonical (*bad_index = the first such, else -1);
 * MASP_HOST_E_CAPACITY: nodes_out given with nodes_capacity < *n_nodes.  Either way no output but *n_nodes / *bad_index is written. */
int masp_host_merkle_tree_complete(unsigned height0, size_t n, const uint8_t* row, uint8_t* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                                   uint8_t root32[32], size_t n_paths, const uint64_t* positions, uint8_t* paths_out, int64_t* bad_index,
                                   int threads);
/* A block of n leaves at position `start` of the depth-32 tree against the old frontier: the arguments and results of
 * masp_hip_merkle_tree_append (include/masp_hip.h) without the context and with the number of host threads a level's parents are dealt to. */
int masp_host_merkle_tree_append(uint64_t start, const uint8_t frontier[32 * 32], size_t n, const uint8_t* row, uint8_t* nodes_out,
                                 size_t nodes_capacity, size_t* n_nodes, int64_t* bad_index, int threads);
int masp_host_jubjub_mul(const uint8_t p32[32], const uint8_t k32[32], uint8_t out32[32]);
int masp_host_point_uv(const uint8_t p32[32], uint8_t out64[64]);
int masp_host_jubjub_add(const uint8_t p32[32], const uint8_t q32[32], int subtract, uint8_t out32[32]);
/* acc + sum_i (+/-) points[i]: the value commitments of a chunk of descriptions (SaplingProvingContext::cv_sum); subtract may be NULL */
int masp_host_jubjub_sum(const uint8_t acc32[32], const uint8_t* points, size_t n, const uint8_t* subtract, uint8_t out32[32]);
/* leaf of the commitment tree for a spendable note (cmu), and pk_d if wanted (may be NULL) */
int masp_host_spend_leaf(const uint8_t ak[32], const uint8_t nsk[32], const uint8_t diversifier[11], const uint8_t rcm[32],
                         const uint8_t id[32], uint64_t value, uint8_t cmu32[32], uint8_t pk_d32[32]);
/* AllowedConversion::from(I128Sum) (masp_primitives/src/convert.rs:86-118): identifiers n x 32, values n x 16 (LE two's-complement i128) */
int masp_host_allowed_conversion(size_t n, const uint8_t* identifiers, const uint8_t* values, uint8_t generator_out[32]);
/* leaf of the convert tree (convert.rs:39-64) */
int masp_host_convert_cmu(const uint8_t generator[32], uint8_t out32[32]);
/* The two calls above for n_conv <= 2^22 conversions on `threads` host threads: the arguments and results of
 * masp_hip_sapling_allowed_conversions (include/masp_hip.h) without the context.  Conversion c owns the terms term_offsets[c] ..
 * term_offsets[c + 1] - 1 (term_offsets[0] = 0, non-decreasing, term_offsets[n_conv] = n_terms <= 2^24) of identifiers (n_terms x 32) and
 * values (n_terms x 16, LE two's-complement i128), summed as given: nothing merged, no zero dropped.  status[c]: 0, or 1 a term's identifier
 * has no generator, else 2 a term's value is i128::MIN; generators_out (n_conv x 32, may be NULL) and cmus_out (n_conv x 32) are then zeros
 * and nothing else changes.  MASP_HOST_E_INVALID: offsets that break the rules, a NULL array that is read or written, a count too large. */
int masp_host_allowed_conversions(size_t n_conv, const uint64_t* term_offsets, size_t n_terms, const uint8_t* identifiers,
                                  const uint8_t* values, uint8_t* status, uint8_t* generators_out, uint8_t* cmus_out, int threads);

/* ---- Sapling note encryption and trial decryption (masp_note_encryption, masp_primitives/src/sapling/note_encryption.rs).
 * A note plaintext is 596 bytes: lead byte (1: rcm follows, 2: a ZIP 212 rseed follows) | diversifier 11 | value u64 LE | asset identifier 32 |
 * rcm or rseed 32 | memo 512; enc_ciphertext is those 596 bytes under ChaCha20-Poly1305 (all-zero nonce, no associated data) and the
 * 16-byte tag.  ivk, esk: canonical scalars below r_J, else MASP_HOST_E_INVALID. ---- */
/* sapling_ka_agree: [8 sk] P as 32 bytes */
int masp_host_sapling_ka_agree(const uint8_t sk[32], const uint8_t p32[32], uint8_t out32[32]);
/* Diversifier::g_d as 32 bytes; MASP_HOST_E_DIVERSIFIER if the diversifier has none (pk_d = [ivk] g_d makes a payment address) */
int masp_host_diversifier_base(const uint8_t diversifier[11], uint8_t out32[32]);
/* kdf_sapling: BLAKE2b-256 personalised "MASP__SaplingKDF" over secret | epk */
void masp_host_kdf_sapling(const uint8_t secret[32], const uint8_t epk[32], uint8_t key32[32]);
/* PRF^expand: BLAKE2b-512 personalised "MASP__ExpandSeed" over sk | t */
void masp_host_prf_expand(const uint8_t* sk, size_t sklen, const uint8_t* t, size_t tlen, uint8_t out64[64]);
/* PRF^expand(rseed, [domain]) reduced mod r_J: domain 4 = rcm, 5 = esk of a ZIP 212 note */
void masp_host_sapling_rseed_scalar(const uint8_t rseed[32], int domain, uint8_t out32[32]);
/* the AEAD alone (RFC 8439, no associated data); decrypt: MASP_HOST_E_NO_NOTE if the tag does not verify */
void masp_host_chacha20poly1305_encrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* plaintext, size_t n, uint8_t* ciphertext,
                                        uint8_t tag[16]);
int masp_host_chacha20poly1305_decrypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* ciphertext, size_t n, const uint8_t tag[16],
                                       uint8_t* plaintext);
/* epk = [esk] g_d, enc_ciphertext under kdf([8 esk] pk_d, epk).  esk is an argument (the reference draws or derives it): deterministic */
int masp_host_sapling_note_encrypt(const uint8_t esk[32], const uint8_t diversifier[11], const uint8_t pk_d[32], const uint8_t plaintext[596],
                                   uint8_t epk_out[32], uint8_t enc_out[612]);
/* try_sapling_note_decryption for one ivk and one output (epk, cmu, enc_ciphertext).  lead_byte: the one the consensus rules expect at the
 * output's height (1 or 2).  MASP_HOST_OK: plaintext_out and pk_d_out = [ivk] g_d are written; MASP_HOST_E_NO_NOTE: every refusal of the
 * reference (epk does not decode, tag, lead byte, asset identifier, rcm, diversifier, pk_d, commitment, the esk check of lead byte 2) */
int masp_host_sapling_try_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc[612], int lead_byte,
                                          uint8_t plaintext_out[596], uint8_t pk_d_out[32]);
/* the same from the symmetric key on (try_note_decryption_inner): the second half of masp_hip_sapling_trial_decrypt's hits */
int masp_host_sapling_finish_note_decryption(const uint8_t key[32], const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32],
                                             const uint8_t enc[612], int lead_byte, uint8_t plaintext_out[596], uint8_t pk_d_out[32]);
/* batch::try_note_decryption on `threads` host threads: hit_ivk[o] = the first ivk index that decrypts output o, or -1; plaintexts
 * (n_out x 596) and pk_ds (n_out x 32) are written for the hits */
int masp_host_sapling_try_note_decryption_batch(size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks, const uint8_t* cmus,
                                                const uint8_t* encs, int lead_byte, int threads, int32_t* hit_ivk, uint8_t* plaintexts,
                                                uint8_t* pk_ds);
/* The compact (ZIP 307) form, try_sapling_compact_note_decryption (masp_note_encryption/src/lib.rs:589-624): a compact output carries
 * epk, cmu and the first 84 bytes of enc_ciphertext (the note plaintext without its memo), so there is no tag: the 84 bytes are decrypted with
 * the keystream from block 1 and everything after decryption is what the full form does (the same refusals, the tag apart).
 * MASP_HOST_OK: plaintext84_out and pk_d_out are written; MASP_HOST_E_NO_NOTE otherwise. */
int masp_host_sapling_try_compact_note_decryption(const uint8_t ivk[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc84[84],
                                                  int lead_byte, uint8_t plaintext84_out[84], uint8_t pk_d_out[32]);
/* batch::try_compact_note_decryption on `threads` host threads, results as in the full batch form (plaintexts84: n_out x 84).  n_candidates
 * (may be NULL): the number of (output, ivk) pairs whose epk decodes and whose decrypted byte 0 equals lead_byte: the pairs that pass the
 * compact form's only cheap filter, what masp_hip_sapling_compact_trial_decrypt's candidate count is compared with */
int masp_host_sapling_try_compact_note_decryption_batch(size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks, const uint8_t* cmus,
                                                        const uint8_t* encs84, int lead_byte, int threads, int32_t* hit_ivk, uint8_t* plaintexts84,
                                                        uint8_t* pk_ds, uint64_t* n_candidates);

/* ---- The sender's side: out_ciphertext and recovery with an outgoing viewing key (masp_note_encryption/src/lib.rs:450-481, :626-718;
 * masp_primitives/src/sapling/note_encryption.rs:90-110, :517-551).  out_ciphertext is the 64 bytes op = pk_d | esk under
 * ChaCha20-Poly1305 (all-zero nonce, no associated data) keyed by the ock, and the 16-byte tag: 80 bytes. ---- */
/* PRF^ock: BLAKE2b-256 personalised "MASP__Derive_ock" over ovk | cv | cmu | epk.  cv: the 32 bytes as they stand in the output description
 * (the reference re-encodes a decoded cv; decoding accepts canonical encodings only, so the bytes are the same) */
void masp_host_prf_ock(const uint8_t ovk[32], const uint8_t cv[32], const uint8_t cmu[32], const uint8_t epk[32], uint8_t ock_out[32]);
/* encrypt_outgoing_plaintext from the ock on: c_out = AEAD(ock, pk_d | esk).  The ovk = none case is the caller's: a random ock and random
 * bytes in the place of pk_d | esk */
void masp_host_sapling_encrypt_outgoing(const uint8_t ock[32], const uint8_t pk_d[32], const uint8_t esk[32], uint8_t c_out[80]);
/* try_sapling_output_recovery_with_ock for one output (epk, cmu, enc_ciphertext, out_ciphertext), in the reference's order: c_out's tag and
 * decryption; pk_d a canonical point of the prime-order subgroup; esk a canonical scalar; [8 esk] pk_d, the KDF, enc's tag and decryption;
 * the lead byte, asset identifier, rcm, g_d, [esk] g_d = epk, pk_d != identity; for lead byte 2 the derived esk = op's; the commitment and the
 * esk check.  MASP_HOST_OK: plaintext_out and pk_d_out are written; MASP_HOST_E_NO_NOTE: every refusal of the reference.  The second half
 * of masp_hip_sapling_output_recovery_scan's hits. */
int masp_host_sapling_try_output_recovery_with_ock(const uint8_t ock[32], const uint8_t epk[32], const uint8_t cmu[32], const uint8_t enc[612],
                                                   const uint8_t c_out[80], int lead_byte, uint8_t plaintext_out[596], uint8_t pk_d_out[32]);
/* try_sapling_output_recovery: PRF^ock, then the function above */
int masp_host_sapling_try_output_recovery(const uint8_t ovk[32], const uint8_t cv[32], const uint8_t epk[32], const uint8_t cmu[32],
                                          const uint8_t enc[612], const uint8_t c_out[80], int lead_byte, uint8_t plaintext_out[596],
                                          uint8_t pk_d_out[32]);
/* the same over n_out outputs x n_ovk ovks on `threads` host threads: hit_ovk[o] = the first ovk index that recovers output o, or -1;
 * plaintexts (n_out x 596) and pk_ds (n_out x 32) are written for the hits */
int masp_host_sapling_try_output_recovery_batch(size_t n_ovk, const uint8_t* ovks, size_t n_out, const uint8_t* cvs, const uint8_t* epks,
                                                const uint8_t* cmus, const uint8_t* encs, const uint8_t* c_outs, int lead_byte, int threads,
                                                int32_t* hit_ovk, uint8_t* plaintexts, uint8_t* pk_ds);

#ifdef __cplusplus
}
#endif
#endif
