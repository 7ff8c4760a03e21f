/* masp_hip.h — C ABI of the MI355X-native Groth16 prover for the MASP Spend / Output / Convert circuits.
 *
 * The reference has no C ABI of its own for this path; these entry points sit exactly
 * where masp_proofs calls into bellperson, i.e. what a Rust FFI layer in a fork of masp_proofs binds:
 *
 *   masp_hip_circuit_load   <- bellman::groth16::Parameters::<Bls12>::read(_, false)
 *                              (/root/reference/masp_proofs/src/lib.rs:336-341) + the circuit's static
 *                              shape that bellperson re-derives on every proof (DensityTracker, A.3 step 2)
 *   masp_hip_prove          <- bellman::groth16::create_random_proof / create_proof
 *                              (/root/reference/masp_proofs/src/sapling/prover.rs:117,202,252) followed by
 *                              Proof::write (/root/reference/masp_proofs/src/prover.rs:190-193,218-221,245-248)
 *   masp_hip_prove_batch    <- the serial per-description loops of SaplingBuilder::build
 *                              (/root/reference/masp_primitives/src/transaction/components/sapling/builder.rs:935-1140)
 *   masp_hip_msm_g1/_g2,
 *   masp_hip_quotient_h     <- bellperson multiexp / EvaluationDomain (un-vendored);
 *                              exposed so each kernel family can be checked and timed on its own.
 *
 * Conventions: C linkage, no exceptions across the boundary, integer return codes (0 = ok), the caller
 * owns every buffer, outputs are written only on success.  A context may be shared between threads:
 * masp_hip_prove / masp_hip_prove_batch are re-entrant (concurrent callers each get batches on their own
 * stream + scratch from the context's pool, so their proofs overlap on the device); circuit loads and the
 * building-block / measurement entry points take the context exclusively.
 * Field elements cross the boundary as 32-byte little-endian
 * canonical integers (`Scalar::to_repr()`), points in the zcash encodings of the bellman wire format.
 */
#ifndef MASP_HIP_H
#define MASP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MASP_HIP_OK 0
#define MASP_HIP_E_INVALID_ARG 1          /* NULL / out-of-range argument */
#define MASP_HIP_E_PARAMS_FORMAT 2        /* undecodable Parameters bytes (the reference panics: lib.rs:337) */
#define MASP_HIP_E_PARAMS_SHAPE 3         /* query lengths disagree with the circuit (SURVEY.md App. C invariants) */
#define MASP_HIP_E_NO_DEVICE 4            /* no gfx950 device / HIP extension unusable — there is NO CPU fallback */
#define MASP_HIP_E_HIP 5                  /* HIP runtime error (see masp_hip_last_error) */
#define MASP_HIP_E_UNEXPECTED_IDENTITY 6  /* delta_g1 / delta_g2 is the identity (bellperson SynthesisError::UnexpectedIdentity); toxic waste that would make h so */
#define MASP_HIP_E_NOT_LOADED 7           /* circuit slot empty */
#define MASP_HIP_E_SCALAR_RANGE 8         /* a scalar >= r was supplied */
#define MASP_HIP_E_POINT_ENCODING 9       /* a Jubjub point encoding does not decode (JPoint::from_bytes, ZIP 216 rules) */
#define MASP_HIP_E_CAPACITY 10            /* an output buffer of the caller is too small: the call says how much it needs */

#define MASP_HIP_MAX_CIRCUITS 8
/* conventional slots for the three MASP circuits */
#define MASP_HIP_SPEND 0
#define MASP_HIP_OUTPUT 1
#define MASP_HIP_CONVERT 2

typedef struct masp_hip_ctx masp_hip_ctx;

/* Static R1CS of one circuit as three CSR matrices over n_constraints rows.  Column v < n_inputs is
 * Input(v) (Input(0) = ONE), otherwise Aux(v - n_inputs).  Terms are merged per variable and non-zero.
 * coef: 32 bytes little-endian canonical per term.  (What `Circuit::synthesize` emits through
 * `ConstraintSystem::enforce`, /root/reference/masp_proofs/src/circuit/sapling.rs:139-596, convert.rs:29-128.) */
typedef struct {
    uint32_t n_inputs, n_aux, n_constraints;
    const uint32_t* a_rowptr; const uint32_t* a_col; const uint8_t* a_coef;
    const uint32_t* b_rowptr; const uint32_t* b_col; const uint8_t* b_coef;
    const uint32_t* c_rowptr; const uint32_t* c_col; const uint8_t* c_coef;
} masp_hip_r1cs;

/* One proving job (masp_hip_prove_batch). a/b/c may be NULL: they are then computed on the GPU from the
 * circuit's static R1CS, so only the assignment crosses PCIe. */
typedef struct {
    uint32_t circuit;          /* slot */
    const uint8_t* inputs;     /* n_inputs x 32 (inputs[0] = ONE) */
    const uint8_t* aux;        /* n_aux x 32 */
    const uint8_t* a;          /* (n_constraints + n_inputs) x 32, or NULL */
    const uint8_t* b;
    const uint8_t* c;
    uint8_t r[32], s[32];      /* Groth16 blinding scalars (the reference draws them from OsRng) */
    uint32_t aux_form;         /* MASP_HIP_AUX_CANONICAL (0): aux[i] = Scalar::to_repr(), 32 bytes little-endian canonical;
                                  MASP_HIP_AUX_MONTGOMERY (1): aux[i] = the Montgomery residue a * 2^256 mod r as four little-endian
                                  u64 limbs — the IN-MEMORY form of blst_fr / bls12_381::Scalar: a binding can hand
                                  over the Vec<Scalar> of its recording constraint system without converting 100 000 elements per
                                  Spend (libmasp_host does: 16 % of its synthesis time).  inputs, a, b, c, r, s stay canonical. */
    uint32_t reserved;         /* must be 0 (MASP_HIP_E_INVALID_ARG otherwise).  ABI note: aux_form and reserved were appended in round 3
                                  (sizeof 112 -> 120 on LP64: 4 + 4 padding + five pointers + 64 bytes of r | s + these two words); the
                                  struct carries no size field, so a binding built against the older header must be rebuilt —
                                  INTEGRATION.md "ABI revisions".  The layout is asserted at the end of this header */
} masp_hip_job;
#define MASP_HIP_AUX_CANONICAL 0
#define MASP_HIP_AUX_MONTGOMERY 1

/* Number of HIP devices this process can see (0 if the runtime is unusable). */
int masp_hip_device_count(void);
/* PCI address of device `device` as "0000:c1:00.0" (cap >= 13): which card of the box a context proves on — its clock and power are
 * the files under /sys/bus/pci/devices/<address>/hwmon (bench.py's clock watch reads them during the timed regions). */
int masp_hip_device_pci_bus_id(int device, char* out, size_t cap);

/* Tuning of a prover, fixed when the context is created (masp_hip_ctx_create_ex).  Every field: 0 = the default.  The
 * library reads NO environment variables; bench.py and the tools translate their MASP_HIP_* variables into this. */
typedef struct {
    uint32_t struct_size;            /* sizeof(masp_hip_options) of the caller's header (versioning) */
    int32_t slots;                   /* batches in flight per device, each on its own HIP streams + scratch: 1..64 (default 4 since round 6: +1.7 % host to
                                        host over 3 at 16 hardware queues — a batch uploads while three compute; 42 GB of scratch per slot
                                        for Spend batches; profiles/r06_slots_3_4_5_at_16_hardware_queues.txt) */
    int32_t batch_cap;               /* proofs per launch sequence: 1..256 (default 256 = BASELINE.json configs[3]) */
    int32_t ntt_sub_batch;           /* proofs per sub-batch of the quotient's transforms (default 8: 160 MiB of work buffers
                                        stay in the Infinity Cache); -1 = the whole batch at once.  A batch in evaluation form on the
                                        three-kernel schedule (masp_hip_ctx_set_quotient_schedule) works in one buffer where the
                                        separate passes need two, and takes TWICE this many proofs per sub-batch: the same bytes */
    int32_t window_bits_h;           /* window width of the h query (default: 16 from 49 152 points, 15 from 16 384) */
    int32_t window_bits_la;          /* ... of the l and a queries (default: from the expected non-trivial scalars) */
    int32_t window_bits_b;           /* ... of b_g1 / b_g2 */
    int32_t window_bits_b2_lone;     /* ... of the second b_g2 table set used by lone proofs (default 8); -1 = not built */
    int32_t witness_nontrivial_percent; /* share of a witness that is neither 0 nor 1, for window selection (default 30) */
    int32_t bucket_tree_levels;      /* levels of shared-inversion affine additions in front of the bucket accumulation of a batch
                                        (default 4, fewer for very short bucket runs); -1 = none (XYZZ accumulation only) */
    int32_t bucket_tree_sub_batch;   /* proofs that go through the tree at a time, at most, for every MSM (its scratch is ~0.3 GB per Spend proof).  Default 0:
                                        every MSM of a batch in as few equal sub-batches as fit the scratch that 86 proofs of ITS worst case would take
                                        — the merged h + l MSM of 256 Spend proofs in three, the witness queries in one; masp_hip_ctx_get_options
                                        reports the smallest in use */
    int32_t bucket_tree_levels_g2;   /* the same for the G2 MSM if it should differ (default: bucket_tree_levels) */
    int32_t bucket_tree_scratch_mb;  /* upper bound of the tree's scratch per slot in MiB (default 0: whatever the device gives).  If the
                                        scratch of a sub-batch does not fit — this bound, or the device is out of memory — the sub-batch
                                        is halved (down to 8 proofs), then the rest of the batch goes through the XYZZ accumulation: same
                                        bytes, fewer proofs per second, never an error */
    int32_t bucket_tree_fallback_proofs; /* OUTPUT of masp_hip_ctx_get_options (ignored on input): proofs whose bucket runs went through
                                        the XYZZ accumulation for lack of tree scratch, or for more entries than masp_hip_ctx_set_tree_entry_share allows; bucket_tree_sub_batch there = the sub-batch in use now */
    int32_t lone_proof_graph;        /* 1: a batch of fewer than 8 proofs replays a captured HIP graph of its ~250 launches from its third
                                        call on.  Default off: with ROCm 7.2 the replay of this five-stream graph takes 11.5 ms where the
                                        launches enqueued one by one take 5.7 (profiles/r04_lone_proof_graph_ab.txt); the bytes are the same */
    int32_t hw_queues;               /* OUTPUT of masp_hip_ctx_get_options (ignored on input; was reserved[0]): the hardware queues the HIP
                                        runtime of this process spreads its streams over, MEASURED when the context was created (as many
                                        single-wave kernels as the context's slots have streams, at most 21, launched at once on streams of
                                        their own, once per process and device: how many ran concurrently).  A slot works on five streams; with
                                        fewer queues than streams, independent kernels wait for each other (round 4, 8 queues: -3 ... -10 %
                                        proofs/s) — and with MORE than MASP_HIP_MAX_USEFUL_HW_QUEUES in the process every dispatch is slower
                                        (see there).  The runtime's default is FOUR (profiles/r05_hw_queues_probe.txt); it reads
                                        GPU_MAX_HW_QUEUES at its first call — see masp_hip_runtime_prepare */
    int32_t window_bits_h_lone;      /* (round 5, appended: struct_size tells) window width of the h query's OWN table, which only lone
                                        proofs use — a batch runs h and l as one MSM over the merged table on window_bits_h.  Narrower
                                        windows mean more additions in the chip-filling accumulation and far fewer buckets in the
                                        latency-bound tails a lone proof waits for.  Default: see resolve_options (ctx.hip) */
    int32_t digit_recoding;          /* RESERVED, must be 0.  (Round 5: 1 = width-(c + 1) non-adjacent-form digits over a table of 2^t P for every
                                        bit position t — 8 - 15 % fewer bucket additions for 16.6 GB of tables per Spend circuit, which is beyond
                                        the ~3.5 GiB of randomly gathered table an XCD's L2 TLB reaches: Spend -8 %, Output +2 % proofs/s.  Built,
                                        bit-exact, measured, removed in round 6: EXPERIMENTS.md, profiles/r05_naf_digits_*.txt.)  A context is
                                        created with 0 here whatever the caller passes; masp_hip_ctx_get_options returns 0 */
    int32_t window_bits_b2;          /* (round 6, appended) window width of the b_g2 query's batch tables when it should differ from
                                        window_bits_b: a G2 addition costs three G1 additions, so b_g2's optimum is wider than b_g1's —
                                        at the price of a sort of its own (with equal widths b_g2 is reduced from b_g1's sorted digit
                                        list).  0 = the default (resolve_options, ctx.hip); -1 = as window_bits_b */
} masp_hip_options;
void masp_hip_options_default(masp_hip_options* opt);
/* More hardware queues than this make a process SLOWER (round 6, profiles/r06_second_context_root_cause.txt): the runtime creates a
 * hardware queue for every new stream until GPU_MAX_HW_QUEUES exist and never gives one back, and once a process holds 24 / 32 of them
 * every kernel dispatch — also of a lone launch sequence on an idle chip — is 7 / 21 % slower (up to 20: nothing).  A context owns
 * 5 x slots + 1 streams (a slot's four side streams only work during lone proofs). */
#define MASP_HIP_MAX_USEFUL_HW_QUEUES 20
/* The HIP runtime gives a process four hardware queues unless GPU_MAX_HW_QUEUES says otherwise, and reads the variable ONCE, at the
 * process's first HIP call.  Loading this library sets GPU_MAX_HW_QUEUES=16 if the variable is not set (a constructor: the only write to
 * the environment the library ever does, and it reads nothing else from it) — enough for a process whose first HIP call comes after the
 * library is loaded, i.e. a Rust binary linking it.  A process that initialises HIP earlier (another HIP library's static initialisers)
 * sets the variable itself, or calls this function before that point: hw_queues <= 0 means 16, more than
 * MASP_HIP_MAX_USEFUL_HW_QUEUES is cut to it; an existing value is kept unless `overwrite`.  Returns the value now in the environment.  What the runtime really uses is reported per context:
 * masp_hip_options::hw_queues. */
int masp_hip_runtime_prepare(int hw_queues, int overwrite);

int masp_hip_ctx_create(int device, masp_hip_ctx** out);
/* The general constructor: n_devices == 1 gives a single-device context, more give the multi-device front described
 * below; opt == NULL means defaults. */
int masp_hip_ctx_create_ex(const int* devices, int n_devices, const masp_hip_options* opt, masp_hip_ctx** out);
/* the options a context runs with, defaults resolved (ntt_sub_batch / window_bits_b2_lone: 0 here means "whole batch" / "not built") */
int masp_hip_ctx_get_options(const masp_hip_ctx* ctx, masp_hip_options* out);
/* One prover over several GPUs of a node (SURVEY.md §8b "devices, n_dev"): the serial per-description loops of
 * SaplingBuilder::build (/root/reference/masp_primitives/src/transaction/components/sapling/builder.rs:935-1140) become one
 * masp_hip_prove_batch call whose jobs are dealt to the devices in full batches, one host thread per device inside
 * the library — a Rust caller reaches all GPUs without any Python / torch.distributed.  masp_hip_circuit_load
 * replicates the CRS on every device (side by side).  A device may be listed more than once (two contexts on one
 * GPU).  The building-block and measurement entry points of such a context run on devices[0]. */
int masp_hip_ctx_create_multi(const int* devices, int n_devices, masp_hip_ctx** out);
/* Subset rows behind the window tables ("boolean blocks").  A third of a MASP witness is the scalar 1, and every such scalar is one entry
 * of the MSM's bucket 0.  With block width k = 2^bits the loader also stores, for every aligned block of k consecutive points of the a,
 * b_g1, b_g2 queries and of the l part of the merged h + l table, the 2^k - 1 sums of its non-empty subsets; a block whose k scalars are
 * all 0 or 1 then costs one entry instead of up to k.  Same proof bytes (the same group elements summed in another order); a block in
 * which some subset sums to the point at infinity is left to the plain path.  bits: 0 = the build's default, -1 = off, 2 or 3.
 * Applies to circuits loaded AFTER the call.  Extra table memory for Spend, from the row counts: k = 4 ~0.1 GB,
 * k = 8 ~1.5 GB.  (A call and not a field of masp_hip_options: that struct's size is part of the ABI older callers are checked against.) */
int masp_hip_ctx_set_boolean_block_bits(masp_hip_ctx* ctx, int32_t bits);
/* the resolved setting: 0 = no subset rows, 2 or 3 */
int masp_hip_ctx_get_boolean_block_bits(const masp_hip_ctx* ctx, int32_t* out);
/* Doubled window rows.  Next to every window row 2^(c j) P the loader also stores 2 * 2^(c j) P; a window digit of odd 2-adic valuation is
 * then an entry of the doubled row in the bucket of half its magnitude, and an MSM needs a bucket only for the magnitudes of even
 * valuation: two thirds as many buckets (21 845 instead of 32 768 on 16-bit windows), so two thirds of the per-bucket work — the bucket
 * tails, the sort's padding of every bucket's run —, for the same additions per scalar.  Same proof bytes.  The rows of a table that opts in
 * double (Spend: the merged h + l table 0.47 -> 0.94 GB).  v: 0 = the build's default, -1 = off, 1 = every table that batches use (the
 * merged h + l tables, a, b_g1, b_g2), 2 = the merged h + l tables only.  The tables only lone proofs use are never doubled; a table with
 * a point at infinity stays as it is.  Applies to circuits loaded AFTER the call; the building-block MSMs (masp_hip_msm_g1_multi and
 * its kin) build their table per call and double its rows only after an explicit v = 1.  (A call and not a field of masp_hip_options, as
 * masp_hip_ctx_set_boolean_block_bits.) */
int masp_hip_ctx_set_window_row_multiples(masp_hip_ctx* ctx, int32_t v);
/* the resolved setting as a mask: bit 0 = the merged h + l tables, bit 1 = a, b_g1, b_g2 */
int masp_hip_ctx_get_window_row_multiples(const masp_hip_ctx* ctx, int32_t* out);
/* The form in which a BATCH (eight proofs or more of a circuit's own a, b, c) computes its quotient.  Only the group element
 * sum_k h_k H_k enters a proof, and it is linear in h: in EVALUATION form the loader derives, once per circuit, a second merged base set —
 * the h query carried through a group-valued inverse DFT, and C's share of the quotient folded into the l query — and a proof then needs
 * four transforms of size m instead of six, no evaluation of C w and no coefficient vector at all; its MSM runs over the coset
 * evaluations a b / (g^m - 1), the aux assignment and the few inputs C uses.  Same proof bytes for every witness, satisfying or not (exact
 * linear algebra, the same group element).  Costs, per circuit: a second merged window table (Spend: 0.47 GB by its row count) and two group transforms
 * at load time.  form: MASP_HIP_QUOTIENT_EVALUATION (0, the default) or MASP_HIP_QUOTIENT_COEFFICIENT (1, six transforms
 * over the h and l queries as they come).  Applies to circuits loaded AFTER the call.  Lone proofs and jobs with caller-supplied a, b, c
 * use the coefficient form whatever is set.  (A call and not a field of masp_hip_options, as masp_hip_ctx_set_boolean_block_bits.) */
#define MASP_HIP_QUOTIENT_EVALUATION 0
#define MASP_HIP_QUOTIENT_COEFFICIENT 1
int masp_hip_ctx_set_quotient_form(masp_hip_ctx* ctx, int32_t form);
int masp_hip_ctx_get_quotient_form(const masp_hip_ctx* ctx, int32_t* out);
/* How a batch in evaluation form schedules its four transforms per proof.  MASP_HIP_QUOTIENT_FUSED (0, the default): for domains of 2^11 to
 * 2^20 points, three launches per sub-batch and no permutation pass — the inverse transforms as decimation in frequency, both transforms'
 * low stages in one kernel with the coset scale between them, the forward transforms' top stages fused with the product.
 * MASP_HIP_QUOTIENT_SEPARATE (1): seven launches — every transform behind a bit-reversal pass — which is also what other domain sizes run.
 * Same scalars, same proof bytes.  Read when a batch is enqueued: one context can be tested and profiled both ways.  (A call and not a
 * field of masp_hip_options, as masp_hip_ctx_set_boolean_block_bits.) */
#define MASP_HIP_QUOTIENT_FUSED 0
#define MASP_HIP_QUOTIENT_SEPARATE 1
int masp_hip_ctx_set_quotient_schedule(masp_hip_ctx* ctx, int32_t schedule);
int masp_hip_ctx_get_quotient_schedule(const masp_hip_ctx* ctx, int32_t* out);
/* The scratch of the bucket tree (masp_hip_options::bucket_tree_levels) is cut for the entries a witness can put into an MSM's digit list, not
 * for every scalar at full width: one window digit per window for a quotient value, a coset evaluation, an input and a witness value that
 * can be anything; one entry for a witness value that the R1CS proves boolean (masp_hip_r1cs_boolean_variables).  percent: of the witness
 * values NOT proven boolean, the share taken to be full width — 1..100, 0 = the default (see MEASUREMENTS.md "Entry bound": the largest share
 * observed over the three MASP circuits, a quarter added).  A proof with more entries than that is found on the device and goes through the
 * XYZZ accumulation alone: the same bytes, counted in masp_hip_options::bucket_tree_fallback_proofs, never an error.  Applies to circuits
 * loaded AFTER the call.  (A call and not a field of masp_hip_options, as masp_hip_ctx_set_boolean_block_bits.) */
int masp_hip_ctx_set_tree_entry_share(masp_hip_ctx* ctx, int32_t percent);
int masp_hip_ctx_get_tree_entry_share(const masp_hip_ctx* ctx, int32_t* out);
/* out[v] = 1 for every variable v < n_inputs + n_aux that `cs` proves boolean — ONE, and every v with a constraint k v (c - c v) = 0 whose C
 * row is empty (bellman's AllocatedBit) — else 0.  Host only: needs no device. */
int masp_hip_r1cs_boolean_variables(const masp_hip_r1cs* cs, uint8_t* out);
/* The entry bound of a base set of n points on windows of window_bits (2..16): ceil(256 / window_bits) entries for each scalar that can be full
 * width — the n - n_witness that are no witness values and ceil((n_witness - n_boolean) share_percent / 100) more — and one for each of the
 * others.  share_percent 0 = the default.  Host only; 0 for arguments out of range. */
uint64_t masp_hip_tree_entry_bound(uint32_t n, int32_t window_bits, uint32_t n_witness, uint32_t n_boolean, int32_t share_percent);
/* the entry bounds a loaded circuit's batch MSMs go by, and their window widths (may be NULL): the merged h + l set in use, a, b_g1, b_g2 */
int masp_hip_circuit_tree_entry_bounds(const masp_hip_ctx* ctx, uint32_t slot, uint64_t bounds[4], int32_t window_bits[4]);
/* number of device contexts behind `ctx` (1 for masp_hip_ctx_create) */
int masp_hip_ctx_device_count(const masp_hip_ctx* ctx);
/* counts[d] = proofs written so far by device context d (d < min(cap, masp_hip_ctx_device_count)): lets a caller (and the
 * configs[4] test) see that a multi-device prover really deals its batches to all of its devices */
int masp_hip_ctx_device_proofs(const masp_hip_ctx* ctx, uint64_t* counts, int cap);
/* A multi-device prover survives a device that fails: masp_hip_prove_batch deals its blocks (<= batch_cap jobs of one circuit, the most
 * expensive first) from ONE queue that every device's host thread takes from when it is free — no static shares —; when a device's call
 * returns MASP_HIP_E_HIP the device is taken out, its unfinished block goes back on the queue and the other devices finish the list
 * (the reference's per-description loop fails per description, not per transaction batch:
 * /root/reference/masp_primitives/src/transaction/components/sapling/builder.rs:955-969).  The call fails only when NO device is left
 * (or for an error of the input, which no other device would cure).  status[d] (d < min(cap, device count)) = MASP_HIP_OK or the
 * error code that took device context d out; a device that is out stays out for the life of the context, and masp_hip_last_error
 * keeps its text.  requeued (may be NULL): proofs that were put back on the queue so far.  A single-device context reports status[0]
 * = MASP_HIP_OK. */
int masp_hip_ctx_device_status(const masp_hip_ctx* ctx, int32_t* status, int cap, uint64_t* requeued);
/* TEST HOOK (tests/test_gpu_device_failure.py): the `nth` masp_hip_prove_batch call (1 = the next) that device context `device` of a
 * multi-device prover receives fails with MASP_HIP_E_HIP before it touches the device, as a lost GPU would.  nth = 0 disarms. */
int masp_hip_ctx_inject_fault(masp_hip_ctx* ctx, int device, uint32_t nth);
/* How many of THIS context's own streams (mains_only: only the ones that work side by side — the context's, the slots' main streams, the
 * verifier's two) run a kernel at the same time, measured now (the context must be idle).  *concurrent < *n_streams means two of them
 * share a hardware queue and run their work one after the other.  Which queue the runtime gives a stream depends on everything the PROCESS
 * created before, so a context creates all of its streams when it is created (and destroys them with itself) — 15 with the default four
 * slots (slots 2 and up use slot 1's side streams), one queue each of the default 16 —, measures the ones that work side by side and
 * replaces any that share a queue: a first, second and third context of a process prove at the same rate
 * (profiles/r06_slot_streams_creation_order.txt, profiles/r06_second_context_root_cause.txt). */
int masp_hip_ctx_stream_concurrency(masp_hip_ctx* ctx, int mains_only, int* n_streams, int* concurrent);
/* *out = calls of masp_hip_prove_batch groups so far that were replayed from a captured launch graph
 * (masp_hip_options::lone_proof_graph); a caller that proves one description at a time sees it grow from its third proof on */
int masp_hip_ctx_lone_graph_launches(const masp_hip_ctx* ctx, uint64_t* out);
void masp_hip_ctx_destroy(masp_hip_ctx* ctx);
const char* masp_hip_strerror(int code);
/* last HIP runtime error text seen by this context ("" if none); the pointer belongs to the calling thread and stays
 * valid until the same thread calls this function again */
const char* masp_hip_last_error(const masp_hip_ctx* ctx);

/* Parse `params` (bellman Parameters wire format; trailing bytes such as the MPC transcript are ignored),
 * check the length invariants against `cs`, upload the CRS and build the window tables. */
int masp_hip_circuit_load(masp_hip_ctx* ctx, uint32_t slot, const uint8_t* params, size_t params_len, const masp_hip_r1cs* cs);
/* What the loader found out about the circuit in `slot` (MASP_HIP_E_NOT_LOADED if empty).  *flags:
 *   bit 0  alpha_g1, beta_g1, delta_g1 and every a / b_g1 query point lie in the prime-order subgroup: the multiplications
 *          s*A and r*B1 of every proof go through the curve endomorphism (half the doublings).  Clear for a CRS with a curve
 *          point outside the subgroup — Parameters::read(_, false) does not look, lib.rs:343-347 — whose proofs then come from
 *          the plain double-and-add, with the bytes the reference computes. */
#define MASP_HIP_CIRCUIT_G1_ENDOMORPHISM 1u
int masp_hip_circuit_flags(const masp_hip_ctx* ctx, uint32_t slot, uint32_t* flags);

/* *form = the form the batches of the circuit in `slot` really use.  MASP_HIP_QUOTIENT_COEFFICIENT also where the evaluation form was asked
 * for and a derived base came out as the point at infinity (negligible for a real CRS, possible for a toy one): such a circuit loads
 * without error and keeps the coefficient form. */
int masp_hip_circuit_quotient_form(const masp_hip_ctx* ctx, uint32_t slot, int32_t* form);
/* *sets = the tables of the circuit in `slot` that really have doubled window rows (masp_hip_ctx_set_window_row_multiples): bit 0 the merged
 * h + l table, bit 1 the merged table of the evaluation form, bit 2 a, bit 3 b_g1, bit 4 b_g2.  A table with a point at infinity stays
 * plain whatever was asked for. */
int masp_hip_circuit_window_row_multiples(const masp_hip_ctx* ctx, uint32_t slot, int32_t* sets);
/* The derived bases of the circuit in `slot`, uncompressed (96 bytes each), in table order: m = 2^logm points T'_i, then n_aux points L'_j,
 * then one point per input column that C uses — input_cols lists those columns, ascending.  *n_points / *n_input_cols always receive the
 * counts (both 0 for a circuit in coefficient form); bases == NULL and input_cols == NULL asks for the counts only; a capacity that is
 * too small gives MASP_HIP_E_CAPACITY and writes nothing.  Exists so that the derivation can be checked on its own. */
int masp_hip_circuit_eval_bases(const masp_hip_ctx* ctx, uint32_t slot, uint8_t* bases, size_t cap_points, size_t* n_points, uint32_t* input_cols,
                                size_t cap_inputs, size_t* n_input_cols);

/* One proof, blocking.  proof_out: 192 bytes = A (48, G1 compressed) | B (96, G2 compressed) | C (48). */
int masp_hip_prove(masp_hip_ctx* ctx, uint32_t slot, const uint8_t* inputs, const uint8_t* aux, const uint8_t* a,
                   const uint8_t* b, const uint8_t* c, const uint8_t r[32], const uint8_t s[32], uint8_t proof_out[192]);
/* n independent jobs, results in job order; proofs_out: n x 192 bytes. */
int masp_hip_prove_batch(masp_hip_ctx* ctx, size_t n, const masp_hip_job* jobs, uint8_t* proofs_out);

/* Groth16 parameters for `cs` from explicit toxic waste (tau | alpha | beta | gamma | delta, 5 x 32 bytes LE),
 * written in the bellman Parameters wire format.  Mirrors bellperson `generate_random_parameters`, which the
 * reference's benches call (/root/reference/masp_proofs/benches/sapling.rs:24-36); needed because the real
 * MPC parameters cannot be downloaded here.  *out_len receives the size; if cap is too small nothing is
 * written and MASP_HIP_E_INVALID_ARG is returned (upper bound: masp_hip_parameters_max_size).
 * MASP_HIP_E_UNEXPECTED_IDENTITY if gamma or delta is 0, or if tau lies on the circuit's evaluation domain
 * (tau^m = 1 for m = 2^ceil(log2(n_constraints + n_inputs)); tau = 1 and tau = r - 1 always do): Z(tau) = 0
 * there, so every h point would be the identity, which masp_hip_circuit_load and bellman both refuse. */
int masp_hip_generate_parameters(masp_hip_ctx* ctx, const masp_hip_r1cs* cs, const uint8_t toxic[160], uint8_t* out, size_t cap,
                                 size_t* out_len);
size_t masp_hip_parameters_max_size(const masp_hip_r1cs* cs);

/* ---- building blocks (same kernels the prover uses) ---- */
/* sum_i scalars[i] * bases[i]; bases uncompressed (96 / 192 B each), result uncompressed */
int masp_hip_msm_g1(masp_hip_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]);
int masp_hip_msm_g2(masp_hip_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[192]);
/* np MSMs over ONE set of n G1 bases, launched the way a batch of proofs launches them (one kernel sequence,
 * gridDim.y = np): scalars np x n x 32, out np x 96.  window_bits: 0 = chosen from n, else 2..16 (the prover's buckets: 16 for
 * the h query and 12 for the witness queries).  Exists so that the batched code path can be checked on its own. */
int masp_hip_msm_g1_multi(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits,
                          uint8_t* out);
/* the same over G2 (bases n x 192, out np x 192) */
int masp_hip_msm_g2_multi(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits,
                          uint8_t* out);
/* The two above with subset rows behind the window tables, chosen per call: block_bits = 0 (none), 2 or 3 — blocks of 4 / 8 consecutive bases
 * by absolute index, those that lie wholly inside [sub_lo, sub_hi) (both cut to n) — see masp_hip_ctx_set_boolean_block_bits.  The plain
 * entry points build no subset rows.  bucket0_entries (np words, may be NULL): the entries of every proof's bucket 0 after
 * the sort — digits of magnitude 1, unit scalars outside an all-boolean block, and one per all-boolean block with a 1 in it. */
int masp_hip_msm_g1_multi_ex(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits,
                             int block_bits, size_t sub_lo, size_t sub_hi, uint8_t* out, uint32_t* bucket0_entries);
int masp_hip_msm_g2_multi_ex(masp_hip_ctx* ctx, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t np, int window_bits,
                             int block_bits, size_t sub_lo, size_t sub_hi, uint8_t* out, uint32_t* bucket0_entries);
/* h = ((A*B - C)/Z) coefficients from evaluation vectors a,b,c (nrows x 32 each, zero-padded to 2^logm);
 * h_out: (2^logm - 1) x 32 */
int masp_hip_quotient_h(masp_hip_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* c, size_t nrows,
                        uint32_t logm, uint8_t* h_out);
/* in-place radix-2 NTT over Fr of 2^logm elements, natural order in and out */
int masp_hip_ntt(masp_hip_ctx* ctx, uint8_t* data, uint32_t logm, int inverse);

/* ---- Groth16 batch verification on the GPU ----
 * <- bellman `verify_proofs_batch` (/root/reference/masp_proofs/src/sapling/verifier/batch.rs:24-31,201-239) and, batched, the
 *    prover's own `verify_proof` self-checks (/root/reference/masp_proofs/src/sapling/prover.rs:148,266) with the
 *    `PreparedVerifyingKey` of /root/reference/masp_proofs/src/lib.rs:391-393.
 * masp_hip_vk_prepare: `params` = Parameters bytes (only the verifying-key prefix is read).
 * masp_hip_verify_batch: n proofs (192 B each) of ONE circuit, their public inputs (n x n_public x 32 B, excluding ONE) and
 * n x 16 B of caller-supplied randomness z (one random linear combination, as bellman does).  Proof decompression, the
 * z_i-multiples and the n Miller loops (one wavefront per pairing) run on the device; the public-input combination, two
 * pairings and the single final exponentiation on the host.  *all_valid = 1 iff every proof verifies (up to 2^-127);
 * 0 says at least one does not, not which (masp_hip_verify_each below says which).  Re-entrant: runs next to proving calls on one of the context's two verifier streams (one
 * verification at a time per key; keys beyond two share a stream).  A key must be freed before its context is destroyed. */
typedef struct masp_hip_vk masp_hip_vk;
int masp_hip_vk_prepare(masp_hip_ctx* ctx, const uint8_t* params, size_t params_len, masp_hip_vk** out);
void masp_hip_vk_free(masp_hip_vk* vk);
int masp_hip_verify_batch(masp_hip_ctx* ctx, masp_hip_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs,
                          uint32_t n_public, const uint8_t* z, int* all_valid);
/* Per-proof verdicts <- `verify_proof` as SaplingVerificationContext calls it (masp_proofs/src/sapling/verifier/single.rs): what a
 * mempool needs for every bundle, and a block validator once a batch has failed.  Same arguments as the batch call without z: nothing
 * is randomised, the result is deterministic.  verdicts[i] (n bytes) is what masp_host_vk_verify returns for proof i alone:
 *    1  the pairing equation holds                     (host: 1)
 *    0  it does not                                    (host: 0)
 *    2  `Proof::read` refuses the proof: flags, a non-canonical coordinate, off the curve, outside the subgroup, the identity  (host: -2)
 *    3  a public input >= r                            (host: -3; 2 comes before 3)
 * All of it runs on the device: decoding, IC_0 + sum_j x_ij IC_j from a table of the key's multiples (uploaded by the first call),
 * three Miller loops per proof (one wavefront per pairing) and one final exponentiation per proof (one wavefront each, the same
 * interpreter).  n = 0 is MASP_HIP_OK; n <= 2^20, processed 2^16 proofs at a time; a wrong n_public gives MASP_HIP_E_PARAMS_SHAPE.
 * Runs on the key's verifier stream, one verification at a time per key, next to proving calls. */
int masp_hip_verify_each(masp_hip_ctx* ctx, masp_hip_vk* vk, size_t n, const uint8_t* proofs, const uint8_t* public_inputs,
                         uint32_t n_public, uint8_t* verdicts);
/* of the key's last masp_hip_verify_each call, summed over its chunks from HIP events on its stream: ms[0] the copies in and the decoding,
 * ms[1] the public-input combination, ms[2] the Miller loops, ms[3] the products and final exponentiations, ms[4] the copy out */
int masp_hip_verify_each_last_timing(masp_hip_vk* vk, double ms[5]);

/* ---- RedJubjub batch verification on the GPU ----
 * masp_hip_jubjub_msm — building block: out32 = the encoding of sum_i [scalars_i] points_i; points n x 32 (Jubjub encodings),
 * scalars n x 32 (little-endian integers below 2^256).  n <= 2^22; n = 0 gives the identity.  A point that does not decode (v >= r,
 * u^2 not a square, u = 0 with the sign bit set: what the host's JPoint::from_bytes refuses) -> MASP_HIP_E_POINT_ENCODING with
 * *bad_index = the first such index (bad_index may be NULL; -1 otherwise).
 * masp_hip_redjubjub_verify_batch <- redjubjub::batch::Verifier::verify as BatchValidator uses it
 *    (masp_proofs/src/sapling/verifier/batch.rs:100-113, 188-200, 213).  n items: vk (n x 32), sig = Rbar || Sbar
 * (n x 64), sighash (n x 32), kind (n bytes: 0 spend authorisation, basepoint spending_key_generator; 1 binding, basepoint
 * value_commitment_randomness_generator; anything else MASP_HIP_E_INVALID_ARG) and n x 16 B of caller-supplied randomness z (bit 0 of
 * each z_i is set, so that no item drops out).  c_i = H*(Rbar_i || vk_i || sighash_i) (BLAKE2b-512, personal "MASP__RedJubjubH",
 * reduced mod r_J).  *all_valid = 1 iff every Rbar_i and vk_i decodes (ZIP 216), every S_i < r_J and
 *    [8] ( sum_i [z_i] R_i + [z_i c_i] vk_i - [sum_{spend auth} z_i S_i] G_spend - [sum_{binding} z_i S_i] G_binding ) = O,
 * i.e. (up to 2^-127) every signature verifies; 0 says at least one does not, not which (masp_hip_redjubjub_verify_each does).  n = 0 is valid; n <= 2^20.  H* and the
 * coefficients are computed on the host; the 2n + 2 point decodings, scalar multiplications and the sum run on the device.
 * Both: re-entrant next to proving and Groth16 verification calls, on the context's second verifier stream (one call at a time per context). */
int masp_hip_jubjub_msm(masp_hip_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* scalars, uint8_t out32[32], int64_t* bad_index);
int masp_hip_redjubjub_verify_batch(masp_hip_ctx* ctx, size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* sighashes,
                                    const uint8_t* kinds, const uint8_t* z, int* all_valid);
/* Per-signature verdicts <- redjubjub::PublicKey::verify (ZIP 216 on): the batch call's arguments without z.  verdicts[i] (n bytes) = 1
 * iff Rbar_i and vk_i decode, S_i < r_J and [8] (R_i + [c_i] vk_i - [S_i] G_kind) = O, else 0.  c_i is computed on the host as in the
 * batch call; everything else runs one lane per signature on the context's second verifier stream, under the batch call's lock. */
int masp_hip_redjubjub_verify_each(masp_hip_ctx* ctx, size_t n, const uint8_t* vks, const uint8_t* sigs, const uint8_t* sighashes,
                                   const uint8_t* kinds, uint8_t* verdicts);

/* ---- The consensus pre-checks of a block's bundles on the GPU ----
 * masp_hip_sapling_check_bundles <- what BatchValidator::check_bundle decides before it queues a proof or a signature
 *    (masp_proofs/src/sapling/verifier/batch.rs:78-193 over SaplingVerificationContextInner, verifier.rs:20-204), for all bundles of a
 * block at once: per description whether cv / rk / epk decode (ZIP 216) and are not of small order and whether `Proof::read` accepts the
 * proof, the description's public inputs (verifier.rs:71-95, 120-128, 151-165), and per bundle the binding verification key
 *    bvk = sum cv(spends) + sum cv(converts) - sum cv(outputs) - sum_entries sign(value) [|value|] [8] asset_generator(identifier)
 * (verifier.rs:167-204 with masp_compute_value_balance, sapling/mod.rs:14-38).  The caller rebuilds the validator's queues from the
 * statuses; signatures and proofs are then verified by the calls above.
 * Arguments: one struct of counts and pointers.  counts: n_bundles x 4, the spends, converts, outputs and value-balance entries of each
 * bundle; the items of each kind lie bundle after bundle in their arrays.  Spends: cv, anchor, nullifier, rk (32 bytes each) and
 * zkproof (192); converts: cv, anchor, zkproof; outputs: cv, cmu, epk, zkproof; value balance: asset identifiers (32 bytes) and values as
 * 16-byte little-endian two's-complement i128.
 * Limits: each of the four totals <= 2^20, n_bundles <= 2^22.  MASP_HIP_E_INVALID_ARG, with nothing written, when a limit is passed, when
 * the column sums of counts differ from the four totals, or when an array with a nonzero total (counts, bvk and bundle_status with a
 * nonzero n_bundles) is NULL.  n_bundles = 0: MASP_HIP_OK, no GPU work, nothing read.
 * Results, all written on success:
 *  - one status byte per description, 0 or the first reason that applies in this order (the reference tells none apart: each makes
 *    check_bundle return false at that description):
 *       1  cv does not decode (v >= r, u^2 not a square, u = 0 with the sign bit set: JPoint::from_bytes)
 *       2  rk (spend) or epk (output) does not decode
 *       3  `Proof::read` refuses the proof: flags, a non-canonical coordinate, off the curve, outside the subgroup, the identity
 *          (exactly masp_host_proof_read)
 *       4  cv has small order
 *       5  rk / epk has small order
 *  - the public inputs as canonical 32-byte little-endian scalars, ready for masp_hip_verify_batch / masp_hip_verify_each: spends n x 7
 *    (rk.u, rk.v, cv.u, cv.v, anchor, the nullifier multipacked into two 254-bit chunks), converts n x 3 (cv.u, cv.v, anchor), outputs
 *    n x 5 (cv.u, cv.v, epk.u, epk.v, cmu).  Anchor and cmu are copied, not range-checked (the verifier's verdict 3 covers them).  The
 *    rows of a description with a nonzero status are zeros.
 *  - bvk (32 bytes) and one status byte per bundle:
 *       0  bvk is valid
 *       1  a description of the bundle has a nonzero status (bvk zeros)
 *       2  an entry's value is i128::MIN: no absolute value (bvk zeros)
 *       3  an entry's identifier has no generator (bvk zeros)
 *    1 before 2 before 3; among the entries the first failing one decides.  An empty bundle has status 0 and the identity's encoding;
 *    entries with the same identifier are independent.
 * The result is deterministic.  Device: one lane per Jubjub encoding, per value-balance entry, per proof point and per bundle (KERNELS.md);
 * proofs go through 2^16 at a time; the other arrays are resident for the call (about 100 bytes a point, 180 an entry).  Re-entrant next
 * to proving and verification calls, on the context's second verifier stream under the RedJubjub calls' lock (one at a time per context);
 * the call creates no stream; on a multi-device context it runs on the first device.
 * masp_hip_check_bundles_last_timing — of the context's last call, from HIP events on its stream: ms[0] the host-to-device copies,
 * ms[1] the kernels, ms[2] the device-to-host copies. */
typedef struct masp_hip_bundle_check {
    size_t n_bundles, n_spends, n_converts, n_outputs, n_balance;
    const uint32_t* counts;                                                             /* n_bundles x 4 */
    const uint8_t *spend_cv, *spend_anchor, *spend_nullifier, *spend_rk, *spend_zkproof;
    const uint8_t *convert_cv, *convert_anchor, *convert_zkproof;
    const uint8_t *output_cv, *output_cmu, *output_epk, *output_zkproof;
    const uint8_t *balance_asset, *balance_value;                                       /* n_balance x 32, n_balance x 16 */
    uint8_t *spend_status, *convert_status, *output_status;                             /* a byte per description */
    uint8_t *spend_inputs, *convert_inputs, *output_inputs;                             /* n x 7 x 32, n x 3 x 32, n x 5 x 32 */
    uint8_t *bvk, *bundle_status;                                                       /* n_bundles x 32, n_bundles */
} masp_hip_bundle_check;
int masp_hip_sapling_check_bundles(masp_hip_ctx* ctx, const masp_hip_bundle_check* args);
int masp_hip_check_bundles_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- Batch trial decryption of Sapling notes on the GPU ----
 * masp_hip_sapling_trial_decrypt <- the device half of masp_note_encryption::batch::try_note_decryption over SaplingDomain
 *    (masp_note_encryption/src/batch.rs:43-86): for each of the n_out x n_ivk (output, ivk) pairs the key agreement [8 ivk] epk, the KDF
 * (BLAKE2b-256, personal "MASP__SaplingKDF", over the secret's encoding and the epk bytes) and the Poly1305 tag of the AEAD over the
 * ciphertext.  ivks: n_ivk x 32, canonical scalars below r_J, anything else MASP_HIP_E_INVALID_ARG (a SaplingIvk is a canonical scalar);
 * epks: n_out x 32; enc_ciphertexts: n_out x 612 (596 bytes under ChaCha20, then the tag).  n_ivk <= 4096, n_out <= 2^26.
 * epk_status (n_out bytes, may be NULL): 0, or why output i's epk does not decode (1 v >= r, 2 not on the curve, 3 u = 0 with the sign bit
 * set: Domain::epk gives None, ZIP 216); such an output takes no part and has no hit.
 * Result: *n_hits pairs whose tag verifies, sorted by (output, ivk): hit_output[i], hit_ivk[i], and the symmetric key hit_keys[32 i ..].
 * The device does NOT decrypt: a hit goes on to masp_host_sapling_finish_note_decryption (include/masp_host.h) with its key, which decrypts,
 * parses and checks the commitment; of an output's hits the first whose finish succeeds is the reference's answer.  If *n_hits >
 * hit_capacity the call returns MASP_HIP_E_CAPACITY with *n_hits = the number of pairs found and writes no hit (nothing is dropped
 * silently: call again with room; n_out x n_ivk always suffices).  n_ivk = 0 or n_out = 0: no hits, no GPU work (epk_status all 0).
 * The result is deterministic.  Large calls are cut into chunks of outputs whose upload overlaps the chunk before's kernels.  Re-entrant next
 * to proving and verification calls, on the context's two verifier streams (one scan at a time per context); on a multi-device context the
 * scan runs on the first device.
 * masp_hip_note_scan_configure — measurement knobs, kept because the A/B they serve is repeated on every new compiler: signed_digits 1 = the
 * ivks' non-adjacent forms (a third fewer additions), 0 = their plain bits; inversion 0 = the divstep inverse, 1 = the binary-gcd inverse
 * for the encoding of the shared secret.  Results do not depend on either.  KERNELS.md records what was measured and the defaults.
 * masp_hip_note_scan_last_timing — of the last scan of this context, summed over its chunks from HIP events on their streams: ms[0] the
 * host-to-device copies, ms[1] the kernels (with two chunks in flight a chunk's kernels may wait for the other's: stream time). */
int masp_hip_sapling_trial_decrypt(masp_hip_ctx* ctx, size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks,
                                   const uint8_t* enc_ciphertexts, uint8_t* epk_status, size_t hit_capacity, uint32_t* hit_output,
                                   uint32_t* hit_ivk, uint8_t* hit_keys, size_t* n_hits);
int masp_hip_note_scan_configure(masp_hip_ctx* ctx, int signed_digits, int inversion);
int masp_hip_note_scan_last_timing(masp_hip_ctx* ctx, double ms[2]);

/* ---- Compact (ZIP 307) batch trial decryption of Sapling notes on the GPU ----
 * masp_hip_sapling_compact_trial_decrypt <- masp_note_encryption::batch::try_compact_note_decryption over SaplingDomain
 *    (masp_note_encryption/src/batch.rs:35, lib.rs:589-624), ALL of it.  A compact output carries epk, cmu and the first 84 bytes of
 * enc_ciphertext (the note plaintext without its memo) and so no tag: the only cheap test of a pair is the lead byte, which one pair of noise
 * in 256 passes.  Stage 1 does for every pair the key agreement, the KDF and ChaCha20 block 1 and compares decrypted byte 0 with lead_byte;
 * stage 2 does for the pairs that pass (the candidates) everything else the reference does: decryption of the 84 bytes, parsing,
 * AssetType::from_identifier, a canonical rcm for lead byte 1, g_d, pk_d = [ivk] g_d != identity, the Pedersen note commitment against cmu
 * and, for lead byte 2, [esk] g_d against epk.
 * ivks, epks, epk_status, n_ivk / n_out limits, hit_capacity / MASP_HIP_E_CAPACITY, the (output, ivk) order, empty lists, determinism, streams
 * and locking: as masp_hip_sapling_trial_decrypt (the two scans of a context exclude each other).  cmus: n_out x 32; enc_compact: n_out x 84;
 * lead_byte: 1 or 2, the one valid at the outputs' height, anything else MASP_HIP_E_INVALID_ARG.
 * Result: *n_hits pairs for which the WHOLE check succeeds: hit_output[i], hit_ivk[i], the note plaintext hit_plaintexts[84 i ..] and
 * pk_d hit_pk_d[32 i ..].  The hits are final: the host finishes nothing, and of an output's hits the first is the reference's answer.
 * *n_candidates (may be NULL): the pairs whose epk decodes and whose decrypted byte 0 equals lead_byte
 * (= masp_host_sapling_try_compact_note_decryption_batch's count).
 * masp_hip_note_scan_compact_last_timing - of the last compact scan of this context, summed over its chunks from HIP events on their streams:
 * ms[0] the host-to-device copies, ms[1] stage 1 (decode and trial), ms[2] stage 2. */
int masp_hip_sapling_compact_trial_decrypt(masp_hip_ctx* ctx, size_t n_ivk, const uint8_t* ivks, size_t n_out, const uint8_t* epks,
                                           const uint8_t* cmus, const uint8_t* enc_compact, int lead_byte, uint8_t* epk_status,
                                           size_t hit_capacity, uint32_t* hit_output, uint32_t* hit_ivk, uint8_t* hit_plaintexts,
                                           uint8_t* hit_pk_d, size_t* n_hits, size_t* n_candidates);
int masp_hip_note_scan_compact_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- Batch output recovery with outgoing viewing keys on the GPU ----
 * masp_hip_sapling_output_recovery_scan <- the device half of try_sapling_output_recovery
 *    (masp_primitives/src/sapling/note_encryption.rs:539-551 over masp_note_encryption/src/lib.rs:635-718) for n_out outputs x n_ovk ovks:
 * for each (output, ovk) pair PRF^ock (BLAKE2b-256, personal "MASP__Derive_ock", over ovk | cv | cmu | epk) and the Poly1305 tag of the
 * AEAD over the 64 ciphertext bytes of out_ciphertext.  No decryption and no curve arithmetic on the device.
 * ovks: n_ovk x 32, any bytes (an OutgoingViewingKey has no range); cvs, epks, cmus: n_out x 32, as they stand in the output descriptions;
 * out_ciphertexts: n_out x 80.
 * Result: *n_hits pairs whose tag verifies, sorted by (output, ovk): hit_output[i], hit_ovk[i] and the pair's ock in hit_ocks[32 i ..],
 * ready for masp_host_sapling_try_output_recovery_with_ock, which decides.  A pair that is not reported is not a note sent under that ovk;
 * of an output's reported pairs the first the host accepts is try_sapling_output_recovery's answer for the first such ovk of the list.
 * n_ovk / n_out limits, hit_capacity / MASP_HIP_E_CAPACITY (*n_hits set, nothing written), empty lists (MASP_HIP_OK, no hits), determinism,
 * chunks, streams and locking: as masp_hip_sapling_trial_decrypt (a context runs one scan of any kind at a time).
 * masp_hip_out_recovery_last_timing - of the last such scan of this context, summed over its chunks from HIP events on their streams:
 * ms[0] the host-to-device copies, ms[1] the kernels. */
int masp_hip_sapling_output_recovery_scan(masp_hip_ctx* ctx, size_t n_ovk, const uint8_t* ovks, size_t n_out, const uint8_t* cvs,
                                          const uint8_t* epks, const uint8_t* cmus, const uint8_t* out_ciphertexts, size_t hit_capacity,
                                          uint32_t* hit_output, uint32_t* hit_ovk, uint8_t* hit_ocks, size_t* n_hits);
int masp_hip_out_recovery_last_timing(masp_hip_ctx* ctx, double ms[2]);

/* ---- Frozen commitment trees on the GPU: batched Merkle hashing ----
 * masp_hip_merkle_tree_complete <- FrozenCommitmentTree::complete, root and path (masp_primitives/src/merkle_tree.rs:177-251) over a row
 * of n nodes at level height0 (0: the leaves, what FrozenCommitmentTree::new passes; above 0: what merge passes once the rows of its full
 * subtrees are stitched).  row: n x 32, canonical encodings below the BLS12-381 scalar modulus (Node::read accepts nothing else);
 * 0 <= height0 <= 32, n <= min(2^22, 2^(32 - height0)), n_paths <= 2^22.
 * The node vector is exactly the one complete appends to, from the given row on: every row padded to an even width with
 * empty_root(level), the width-1 rows near the top included, the next row directly behind it, the last row the single node of level 32;
 * *n_nodes (may be NULL) is its length in nodes.  n = 0: the vector is empty, the root is empty_root(32), no GPU work.
 * nodes_out (nodes_capacity x 32 bytes) may be NULL: a caller that wants its witnesses does not download 64 bytes per leaf.  If it is given
 * and nodes_capacity < *n_nodes the call returns MASP_HIP_E_CAPACITY with *n_nodes set and writes nothing else.
 * root32: the node of level 32.  positions: n_paths indices into the given row, each below n (MASP_HIP_E_INVALID_ARG otherwise);
 * paths_out: n_paths x (32 - height0) x 32 bytes, position by position the siblings from level height0 up, gathered on the device.  Whether
 * sibling i is a left node is bit i of the position and is not returned.
 * A node of the row that is not canonical: MASP_HIP_E_INVALID_ARG with *bad_index (may be NULL) the smallest such index, else -1; no output
 * buffer is written and the context stays usable.
 * The result is deterministic.  Re-entrant next to proving and verification calls; on the context's first verifier stream, under the lock
 * of the note scans (a context runs one scan or one tree at a time: they share the Pedersen table); on a multi-device context on the first
 * device.  masp_host_merkle_tree_complete (include/masp_host.h) is the same on the host.
 * masp_hip_merkle_last_timing - of the last tree of this context, from HIP events on its stream: ms[0] the host-to-device copies, ms[1] the
 * kernels, ms[2] the device-to-host copies. */
int masp_hip_merkle_tree_complete(masp_hip_ctx* ctx, unsigned height0, size_t n, const uint8_t* row, uint8_t* nodes_out, size_t nodes_capacity,
                                  size_t* n_nodes, uint8_t root32[32], size_t n_paths, const uint64_t* positions, uint8_t* paths_out,
                                  int64_t* bad_index);
int masp_hip_merkle_last_timing(masp_hip_ctx* ctx, double ms[3]);
/* masp_hip_merkle_tree_append - a block of leaves at an arbitrary offset of the depth-32 tree: what advances a CommitmentTree and its
 * IncrementalWitnesses (masp_primitives/src/merkle_tree.rs:271-723) by that block with one call instead of one hash chain per leaf and
 * witness.  row: n x 32, the leaves at positions start .. start + n - 1, canonical encodings; start even or odd, start + n <= 2^32,
 * n <= 2^22.  frontier: 32 x 32 bytes, entry h the node (level h, index (start >> h) - 1), the root of the complete 2^h-leaf subtree that
 * ends just before start; entry h is read, and has to be canonical, only where bit h of start is set, the others are ignored (frontier may
 * be NULL with start = 0).
 * nodes_out: level by level for h = 1 .. 32 the nodes (h, i) with start >> h <= i < (start + n) >> h, 32 bytes each: exactly the complete
 * nodes whose last leaf lies in the block, nothing padded.  *n_nodes (may be NULL) is their number, fewer than n + 32.  nodes_out NULL:
 * *n_nodes alone, no GPU work.  nodes_capacity < *n_nodes: MASP_HIP_E_CAPACITY, nothing written.
 * A node that is not canonical: MASP_HIP_E_INVALID_ARG with *bad_index (may be NULL) = -2 - h for the lowest used frontier entry h, else
 * the smallest such index of the row; nothing is written and the context stays usable.  *bad_index is -1 otherwise.
 * Deterministic; same stream, lock, table and scratch as the frozen tree's call, and masp_hip_merkle_last_timing reports the last call of
 * either kind.  masp_host_merkle_tree_append (include/masp_host.h) is the same on the host. */
int masp_hip_merkle_tree_append(masp_hip_ctx* ctx, uint64_t start, const uint8_t frontier[32 * 32], size_t n, const uint8_t* row,
                                uint8_t* nodes_out, size_t nodes_capacity, size_t* n_nodes, int64_t* bad_index);

/* ---- Nullifiers and note commitments of a wallet's notes on the GPU ----
 * masp_hip_sapling_note_nullifiers <- Note::cmu and Note::nf(&nk, position) (masp_primitives/src/sapling.rs:828) for n notes:
 *    g = the asset generator of the identifier (cofactor not cleared), g_d = diversifier.g_d(),
 *    rcm = the 32 bytes (lead byte 1) | PRF^expand(rseed, [4]) mod r_J (lead byte 2),
 *    cm = PedersenHash(NoteCommitment, repr(g) | value | repr(g_d) | pk_d) + [rcm] G_ncr, cmu = its affine u,
 *    rho = cm + [position] G_nf (all 64 bits of position count), nf = BLAKE2s-256(personal "MASP__nf", nk | repr(rho)).
 * asset_identifiers, pk_ds, rseeds (rcm or rseed), nks: n x 32; diversifiers: n x 11; values, positions: n; lead_bytes: n, each 1
 * (BeforeZip212) or 2 (AfterZip212).  n <= 2^22 a call; the device works through them in chunks of 2^19, a few hundred MB of state.
 * Result: status (n bytes), cmus_out (n x 32, may be NULL: not downloaded) and nfs_out (n x 32).  status[i] is 0, or the first check that
 * fails, in this order: 1 the asset identifier has no generator, 2 the diversifier has no g_d, 3 pk_d is not the canonical encoding of a
 * curve point, 4 the lead byte is neither 1 nor 2, or lead byte 1 with rcm >= r_J, 5 nk is not the canonical encoding of a curve point.
 * A note with status != 0 has 32 zero bytes in either output and changes neither the return code nor its neighbours' results.
 * What is checked of pk_d and nk is what masp_host_note_cmu checks of pk_d: the encoding is canonical and on the curve.  The reference's
 * types make both of them points of the prime-order subgroup; that is NOT tested here, and the bytes hashed are the bytes given.
 * n = 0: MASP_HIP_OK, no GPU work, no array is read.  A NULL array (cmus_out apart) with n > 0, or n > 2^22: MASP_HIP_E_INVALID_ARG.
 * The result is deterministic, and the same for either number of lanes per note.  Re-entrant next to proving and verification calls; on
 * the context's first verifier stream, under the lock of the note scans and the trees (a context runs one of them at a time: they share
 * the Pedersen table), no stream or hardware queue of its own; on a multi-device context on the first device.
 * masp_host_sapling_note_nullifiers (include/masp_host.h) is the same on the host.
 * masp_hip_note_nullifiers_configure - lanes_per_note: 1 or 8 lanes add a note's table points, 0 (the default) = by the number of notes
 * (DESIGN.md 13); for measurements and tests, the bytes do not depend on it.  Anything else: MASP_HIP_E_INVALID_ARG.
 * masp_hip_note_nullifiers_last_timing - of the last such call of this context, summed over its chunks from HIP events on its stream:
 * ms[0] the host-to-device copies, ms[1] the kernels, ms[2] the device-to-host copies. */
int masp_hip_sapling_note_nullifiers(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                     const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                     const uint8_t* nks, const uint64_t* positions, uint8_t* status, uint8_t* cmus_out, uint8_t* nfs_out);
int masp_hip_note_nullifiers_configure(masp_hip_ctx* ctx, int lanes_per_note);
int masp_hip_note_nullifiers_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- A conversion tree's leaves on the GPU: allowed conversions in batches ----
 * masp_hip_sapling_allowed_conversions <- AllowedConversion::from(I128Sum) and AllowedConversion::cmu (masp_primitives/src/convert.rs:39-64,
 * 86-118) for n_conv conversions.  The terms are in CSR form: conversion c owns the terms term_offsets[c] .. term_offsets[c + 1] - 1, a term
 * an identifier (32 bytes) and a value (16 bytes, little-endian two's-complement i128).  For every conversion
 *    generator = sum_j sign(v_j) [|v_j| as u64] G_j, G_j the asset generator of identifier j (cofactor not cleared), |v_j| as u64 the LOW
 *                64 bits of the absolute value, as the reference's cast keeps them,
 *    cmu       = the affine u of PedersenHash(NoteCommitment, the 256 bits of repr(generator)): the conversion tree's leaf.
 * The terms are summed as given: equal identifiers are not merged, zeros are not dropped (the caller merges, as the reference's I128Sum
 * does; with the truncation, merging before and after summing differ).  A conversion without terms has the identity as its generator.
 * Result: status (n_conv bytes), generators_out (n_conv x 32, may be NULL: not downloaded) and cmus_out (n_conv x 32).  status[c] is 0, or
 * 1: one of its terms' identifiers has no generator, or 2: no such term, but one of its terms' values is i128::MIN (which has no absolute
 * value); it does not depend on the terms' order.  A conversion with status != 0 has 32 zero bytes in either output and changes neither the
 * return code nor its neighbours' results.
 * Requirements: term_offsets[0] = 0, non-decreasing, term_offsets[n_conv] = n_terms, n_conv <= 2^22, n_terms <= 2^24; they are checked on
 * the host before any GPU work, and anything else, or a NULL array (generators_out apart; identifiers and values may be NULL with
 * n_terms = 0), is MASP_HIP_E_INVALID_ARG with nothing written.  n_conv = 0: MASP_HIP_OK, no GPU work, no array is read.
 * The device works through chunks cut at conversion boundaries, of at most 2^19 conversions and at most 2^20 terms (about 180 MB of term
 * points and inputs); ONE conversion with more terms than a chunk holds is MASP_HIP_E_INVALID_ARG before any work.  A conversion's terms are
 * added by the lanes of its group one after the other: there is no reduction across lane groups, a very long conversion is a serial loop.
 * The result is deterministic, and the same for either number of lanes and any chunk size.  Re-entrant next to proving and verification
 * calls; on the context's first verifier stream, under the lock of the note scans, the trees and the nullifiers (a context runs one of
 * them at a time: they share the Pedersen table), no stream or hardware queue of its own; on a multi-device context on the first device.
 * masp_host_allowed_conversions (include/masp_host.h) is the same on the host.
 * masp_hip_allowed_conversions_configure - for measurements and tests, the bytes depend on none of it.  lanes_per_conversion: 1 or 8
 * lanes add a conversion's points, 0 (the default) = by the number of conversions; chunk_conversions, chunk_terms: a
 * chunk's limits, 0 = the defaults.  Other lane counts, or limits above the defaults: MASP_HIP_E_INVALID_ARG.
 * masp_hip_allowed_conversions_last_timing - of the last such call of this context, summed over its chunks from HIP events on its stream:
 * ms[0] the host-to-device copies, ms[1] the kernels, ms[2] the device-to-host copies. */
int masp_hip_sapling_allowed_conversions(masp_hip_ctx* ctx, size_t n_conv, const uint64_t* term_offsets, size_t n_terms,
                                         const uint8_t* identifiers, const uint8_t* values, uint8_t* status, uint8_t* generators_out,
                                         uint8_t* cmus_out);
int masp_hip_allowed_conversions_configure(masp_hip_ctx* ctx, int lanes_per_conversion, size_t chunk_conversions, size_t chunk_terms);
int masp_hip_allowed_conversions_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- Output descriptions without their proofs on the GPU: cv, cmu, epk and the two ciphertexts in batches ----
 * masp_hip_sapling_build_outputs <- what SaplingOutputInfo::build (masp_primitives/src/transaction/components/sapling/builder.rs:533-575)
 * puts around an Output proof, for n outputs.  The call draws no randomness: the caller supplies every random value, and the result is a
 * function of the inputs.  Per output:
 *    rcm = the 32 bytes of rseeds (lead byte 1) | PRF^expand(rseed, [4]) mod r_J (lead byte 2)            (Note::rcm),
 *    esk = the 32 bytes of esks (lead byte 1) | PRF^expand(rseed, [5]) mod r_J (lead byte 2)              (Note::derive_esk),
 *    cv  = what masp_host_value_commitment(id, value, rcv) returns, cmu = what masp_host_note_cmu(id, value, diversifier, pk_d, rcm) returns,
 *    epk = [esk] g_d,
 *    enc_ciphertext (612 bytes) = AEAD(KDF([8 esk] pk_d, epk), lead | d | value | id | rseed | memo): masp_host_sapling_note_encrypt,
 *    out_ciphertext (80 bytes) = AEAD(PRF^ock(ovk, cv, cmu, epk), pk_d | esk) with an ovk, or AEAD(r[0:32], r[32:96]) of the output's 96
 *    bytes of out_randoms without one (the ovk = bottom case of encrypt_outgoing_plaintext).
 * asset_identifiers, pk_ds, rseeds, esks, rcvs, ovks: n x 32; diversifiers: n x 11; values, lead_bytes: n; memos: n x 512; ovk_flags: n,
 * 0 = the ovk is absent; out_randoms: n x 96, read only where the ovk is absent; esks are read only where the lead byte is 1.
 * May be NULL: memos (every memo is the empty memo, 0xf6 then zeros, and nothing is uploaded for it), ovk_flags (every ovk is present),
 * out_randoms when no flag is 0, esks when no lead byte is 1; these conditions are checked on the host before any GPU work.
 * Result: status (n bytes), cvs_out, cmus_out, epks_out (n x 32), encs_out (n x 612), couts_out (n x 80).  status[i] is 0, or the first check
 * that fails, in this order: 1 the asset identifier has no generator, 2 the diversifier has no g_d, 3 pk_d is not the canonical encoding of
 * a curve point, 4 the lead byte is neither 1 nor 2, or lead byte 1 with rcm >= r_J (1 to 4 as in masp_hip_sapling_note_nullifiers),
 * 5 lead byte 1 with esk >= r_J, 6 rcv >= r_J.  An output with status != 0 has zeros in all five outputs and changes neither the return
 * code nor its neighbours' results.  A zero esk is NOT refused, as on the host, and the subgroup membership of pk_d is NOT tested, as in
 * the nullifier call: it is decoded, canonical and on the curve, and the bytes encrypted are the bytes given.
 * n <= 2^20 a call; n = 0: MASP_HIP_OK, no GPU work, no array is read.  Any other NULL array, or n > 2^20: MASP_HIP_E_INVALID_ARG with
 * nothing written.  The device works through chunks of at most 2^16 outputs (about 225 MB of inputs, state and ciphertexts), one after the
 * other.  The result is deterministic and the same for any chunk size.  Re-entrant next to proving and verification calls; on the context's
 * first verifier stream, under the lock of the note scans, the trees, the nullifiers and the conversions (a context runs one of them at a
 * time: they share the Pedersen and nullifier tables), no stream or hardware queue of its own; on a multi-device context on the first device.
 * masp_host_sapling_build_outputs (include/masp_host.h) is the same on the host.
 * masp_hip_build_outputs_configure - chunk_outputs: outputs per chunk, 0 = the default; for measurements and tests, the bytes do not
 * depend on it.  Values above the default: MASP_HIP_E_INVALID_ARG.
 * masp_hip_build_outputs_last_timing - of the last such call of this context, summed over its chunks from HIP events on its stream:
 * ms[0] the host-to-device copies, ms[1] the kernels, ms[2] the device-to-host copies. */
int masp_hip_sapling_build_outputs(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                   const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                   const uint8_t* esks, const uint8_t* rcvs, const uint8_t* memos, const uint8_t* ovks, const uint8_t* ovk_flags,
                                   const uint8_t* out_randoms, uint8_t* status, uint8_t* cvs_out, uint8_t* cmus_out, uint8_t* epks_out,
                                   uint8_t* encs_out, uint8_t* couts_out);
int masp_hip_build_outputs_configure(masp_hip_ctx* ctx, size_t chunk_outputs);
int masp_hip_build_outputs_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- Spend descriptions without their proofs, and RedJubjub signatures, on the GPU: cv, rk, nf and sig in batches ----
 * Both calls draw no randomness: the caller supplies every random byte, and the result is a function of the inputs.
 * masp_hip_redjubjub_sign_batch <- PrivateKey::randomize, PublicKey::from_private and PrivateKey::sign as spend_sig_internal composes them
 *    (masp_primitives/src/sapling.rs:167-195, sapling/redjubjub.rs:121-160), over either basepoint, for n items:
 *    rsk  = sk + alpha mod r_J,  vk = [rsk] G_kind                      (rk for kind 0, bvk for kind 1),
 *    r    = H*(T || vk || sighash),  Rbar = repr([r] G_kind),  S = r + H*(Rbar || vk || sighash) rsk mod r_J,
 *    H* = BLAKE2b-512, personal "MASP__RedJubjubH", reduced mod r_J.
 * sks, alphas, sighashes: n x 32; kinds: n bytes, 0 spend authorisation on spending_key_generator, 1 binding on
 * value_commitment_randomness_generator (as in masp_hip_redjubjub_verify_each), anything else MASP_HIP_E_INVALID_ARG before any work;
 * randoms: n x 80, the reference's T.  alphas may be NULL: no randomisation (the binding signature's case).
 * Result: status (n bytes), vks_out (n x 32, may be NULL: not downloaded), sigs_out (n x 64, Rbar || Sbar).  status[i] is 0, or the first
 * check that fails: 1 sk >= r_J (what PrivateKey::read refuses), 2 alpha >= r_J.  A refused item has zeros in both outputs and changes
 * neither the return code nor its neighbours' results.  rsk = 0 is NOT refused: the reference signs with it, so this call does too, and vk
 * is then the identity's encoding.
 * masp_hip_sapling_build_spends <- what the builder (masp_primitives/src/transaction/components/sapling/builder.rs) puts around a Spend
 * proof, for n spends:
 *    nk = [nsk] G_pgk (ProofGenerationKey::to_viewing_key),  rk = ak + [ar] G_spend (ViewingKey::rk),
 *    cv = what masp_host_value_commitment(id, value, rcv) returns,
 *    cmu, nf = what masp_hip_sapling_note_nullifiers gives for (note, nk, position).
 * The six note arrays are that call's (asset_identifiers, pk_ds, rseeds: n x 32; diversifiers: n x 11; values, lead_bytes: n); aks, nsks,
 * ars, rcvs: n x 32; positions: n.  The anchor is the caller's, from the tree, and is not an input.
 * Result: status (n bytes), cvs_out, rks_out, nfs_out (n x 32), cmus_out and nks_out (n x 32, either may be NULL: not downloaded).
 * status[i] is 0, or the first check that fails, in this order: 1 to 4 as in masp_hip_sapling_note_nullifiers, 5 ak is not the canonical
 * encoding of a curve point, 6 [8] ak is the identity (the Spend circuit asserts that ak is not of small order: a spend built here is
 * provable), 7 nsk >= r_J, 8 ar >= r_J, 9 rcv >= r_J.  A refused spend has zeros in all five outputs and changes neither the return code
 * nor its neighbours' results.  Beyond check 6 the membership of ak in the prime-order subgroup is NOT tested, and that of pk_d is NOT
 * tested either, as in the neighbouring calls: both are decoded, canonical and on the curve.
 * Both: n <= 2^20 a call; n = 0: MASP_HIP_OK, no GPU work, no array is read.  A NULL array other than those named, or n > 2^20:
 * MASP_HIP_E_INVALID_ARG with nothing written.  The device works through chunks of at most 2^16 items, one after the other; the result is
 * deterministic and the same for any chunk size.  Re-entrant next to proving and verification calls; on the context's first verifier
 * stream, under the lock of the note scans, the trees, the nullifiers, the conversions and the outputs, no stream or hardware queue of
 * their own; on a multi-device context on the first device.
 * Secrets: sks, alphas, randoms, nsks, ars and rcvs pass through pinned staging memory of the context; that staging memory, every uploaded
 * input and the per-item state on the device (rsk and r among it) are zeroed on the call's stream before the call releases the lock, on
 * success and on every error path.  This is a guarantee of the call, not a best effort; memory of the caller's is the caller's.
 * masp_host_redjubjub_sign_batch and masp_host_sapling_build_spends (include/masp_host.h) are the same on the host.
 * masp_hip_redjubjub_sign_configure, masp_hip_build_spends_configure - items per chunk, 0 = the default; for measurements and tests, the
 * bytes do not depend on it.  Values above the default: MASP_HIP_E_INVALID_ARG.
 * masp_hip_redjubjub_sign_last_timing, masp_hip_build_spends_last_timing - of the last such call of this context, summed over its chunks
 * from HIP events on its stream: ms[0] the host-to-device copies, ms[1] the kernels, ms[2] the device-to-host copies. */
int masp_hip_redjubjub_sign_batch(masp_hip_ctx* ctx, size_t n, const uint8_t* sks, const uint8_t* alphas, const uint8_t* sighashes,
                                  const uint8_t* kinds, const uint8_t* randoms, uint8_t* status, uint8_t* vks_out, uint8_t* sigs_out);
int masp_hip_redjubjub_sign_configure(masp_hip_ctx* ctx, size_t chunk_items);
int masp_hip_redjubjub_sign_last_timing(masp_hip_ctx* ctx, double ms[3]);
int masp_hip_sapling_build_spends(masp_hip_ctx* ctx, size_t n, const uint8_t* asset_identifiers, const uint64_t* values,
                                  const uint8_t* diversifiers, const uint8_t* pk_ds, const uint8_t* lead_bytes, const uint8_t* rseeds,
                                  const uint8_t* aks, const uint8_t* nsks, const uint8_t* ars, const uint8_t* rcvs, const uint64_t* positions,
                                  uint8_t* status, uint8_t* cvs_out, uint8_t* rks_out, uint8_t* nfs_out, uint8_t* cmus_out, uint8_t* nks_out);
int masp_hip_build_spends_configure(masp_hip_ctx* ctx, size_t chunk_spends);
int masp_hip_build_spends_last_timing(masp_hip_ctx* ctx, double ms[3]);

/* ---- measurement hooks (bench.py): device-resident workloads, HIP-event timing on the ctx stream ---- */
/* Keeps `n` jobs' assignments resident in HBM; returns a handle (>= 0) or a negative error code. */
int masp_hip_batch_upload(masp_hip_ctx* ctx, size_t n, const masp_hip_job* jobs);
/* Proves every resident job of `handle` once; proofs_out n x 192.  elapsed_ms (may be NULL) = HIP-event time
 * from first kernel to last proof written, inputs already in HBM. */
int masp_hip_batch_prove_resident(masp_hip_ctx* ctx, int handle, uint8_t* proofs_out, float* elapsed_ms);
/* The same, `steps` times over: step k proves every resident job with the blinding scalars rs[(k * n + job) * 64 ...]
 * (r | s, 32 + 32 bytes; NULL = the uploaded ones), all steps enqueued back to back without host synchronisation — one
 * step = one pass of the hot path over one batch of n jobs.  proofs_out: steps x n x 192 bytes. */
int masp_hip_batch_prove_resident_steps(masp_hip_ctx* ctx, int handle, size_t steps, const uint8_t* rs, uint8_t* proofs_out,
                                        float* elapsed_ms);
int masp_hip_batch_free(masp_hip_ctx* ctx, int handle);
/* Runs the G1 MSM of query `which` (0 h, 1 l, 2 a, 3 b_g1) of circuit `slot` `iters` times on resident job
 * `job` of `handle`; returns average kernel-sequence time per MSM in ms and the number of bases. */
int masp_hip_bench_msm(masp_hip_ctx* ctx, int handle, size_t job, int which, int iters, float* avg_ms, uint32_t* n_bases);

/* Live timing of the dominant kernel, k_msm_accumulate over G1 (bucket accumulation): when enabled, every launch
 * is bracketed by HIP events on its own stream.  read: summed duration, launch count and the algorithmic bytes
 * (n x (96 + 32) per G1 MSM of n points) of all launches since enable/reset. */
int masp_hip_profile_enable(masp_hip_ctx* ctx, int on);
int masp_hip_profile_read(masp_hip_ctx* ctx, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
/* The same launches by kernel group, summed milliseconds since enable / reset: ms[0] plan / records / copies of the bucket tree,
 * ms[1] its denominators pass (k_tree_pass1), ms[2] the shared inversions (k_binv_*), ms[3] its additions pass (k_tree_pass2),
 * ms[4] the XYZZ accumulation of what is left (k_msm_accumulate_pts, or k_msm_accumulate without a tree); ms[5..7] = 0. */
int masp_hip_profile_read_split(masp_hip_ctx* ctx, double ms[8]);
/* Where the chains of the last LONE proof (a batch of fewer than 8 proofs) proved with profiling on ended, in milliseconds of GPU time
 * after its first kernel could start — HIP events behind the stages, no profiler in the way: ms[1] MSM a, [2] s*A, [3] MSM b_g1, [4] r*B1,
 * [5] MSM b_g2, [6] g_b written, [7] quotient, [8] MSM h, [9] MSM l, [10] g_a / g_c written, [11] the proof complete; -1 = not recorded. */
int masp_hip_profile_read_lone(masp_hip_ctx* ctx, double ms[12]);
/* Page-locked host memory for assignments.  masp_hip_prove_batch recognises `aux` pointers that lie in page-locked
 * memory (from here or from the caller's own hipHostMalloc / hipHostRegister) and copies them to the device directly;
 * anything else goes through the library's own pinned staging buffer first (one extra host copy of ~3 MB per Spend).
 * The reference keeps the assignment in ordinary Vec<Scalar>s inside bellperson's ProvingAssignment; a binding that
 * synthesizes into a buffer obtained here saves that copy.  NULL on failure. */
void* masp_hip_host_alloc(masp_hip_ctx* ctx, size_t bytes);
void masp_hip_host_free(masp_hip_ctx* ctx, void* ptr);
/* hipDeviceSynchronize on the context's device */
int masp_hip_sync(masp_hip_ctx* ctx);

#ifdef __cplusplus
}
#endif

/* ---- the layout a binding relies on, checked wherever this header is compiled (LP64: the only ABI the library is built for).  A Rust
 * `#[repr(C)]` mirror must give the same numbers; tests/native/capi_harness.c repeats them with offsetof ---- */
#if defined(__cplusplus) && __cplusplus >= 201103L
#define MASP_HIP_STATIC_ASSERT(c, m) static_assert(c, m)
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define MASP_HIP_STATIC_ASSERT(c, m) _Static_assert(c, m)
#else
#define MASP_HIP_SA_CAT2(a, b) a##b
#define MASP_HIP_SA_CAT(a, b) MASP_HIP_SA_CAT2(a, b)
#define MASP_HIP_STATIC_ASSERT(c, m) typedef char MASP_HIP_SA_CAT(masp_hip_static_assert_, __LINE__)[(c) ? 1 : -1]
#endif
#if defined(__LP64__) || defined(_LP64)
MASP_HIP_STATIC_ASSERT(sizeof(masp_hip_job) == 120, "masp_hip_job: 4 + 4 pad + 5 pointers + r[32] + s[32] + aux_form + reserved");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_job, inputs) == 8 && offsetof(masp_hip_job, c) == 40, "masp_hip_job pointers");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_job, r) == 48 && offsetof(masp_hip_job, s) == 80, "masp_hip_job r | s");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_job, aux_form) == 112 && offsetof(masp_hip_job, reserved) == 116, "masp_hip_job tail");
MASP_HIP_STATIC_ASSERT(sizeof(masp_hip_r1cs) == 88 && offsetof(masp_hip_r1cs, a_rowptr) == 16 && offsetof(masp_hip_r1cs, c_coef) == 80,
                       "masp_hip_r1cs: three counts + 4 pad + nine pointers");
MASP_HIP_STATIC_ASSERT(sizeof(masp_hip_options) == 76 && offsetof(masp_hip_options, window_bits_b2) == 72,
                       "masp_hip_options: struct_size + 18 int32 fields (appended-only: struct_size versions it)");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_options, hw_queues) == 60 && offsetof(masp_hip_options, digit_recoding) == 68, "masp_hip_options tail");
MASP_HIP_STATIC_ASSERT(sizeof(masp_hip_bundle_check) == 224 && offsetof(masp_hip_bundle_check, counts) == 40, "masp_hip_bundle_check: five counts + 23 pointers");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_bundle_check, convert_cv) == 88 && offsetof(masp_hip_bundle_check, output_cv) == 112 &&
                           offsetof(masp_hip_bundle_check, balance_asset) == 144,
                       "masp_hip_bundle_check inputs");
MASP_HIP_STATIC_ASSERT(offsetof(masp_hip_bundle_check, spend_status) == 160 && offsetof(masp_hip_bundle_check, spend_inputs) == 184 &&
                           offsetof(masp_hip_bundle_check, bvk) == 208,
                       "masp_hip_bundle_check results");
#endif
#endif
