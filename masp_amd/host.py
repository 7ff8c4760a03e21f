"""ctypes binding of libmasp_host.so: the host-side witness generator and native primitives
(masp_amd/csrc/host).  CPU-only code; the Groth16 hot path itself lives in libmasp_hip.so."""
import ctypes as C
import os

import numpy as np

from .r1cs import R1cs

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

SPEND, OUTPUT, CONVERT = 0, 1, 2
KINDS = {"spend": SPEND, "output": OUTPUT, "convert": CONVERT}
JUBJUB_ORDER = 6554484396890773809930967563523245729705921265872317281365359162392183254199
FR_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TREE_DEPTH = 32
ERRORS = {1: "invalid encoding", 2: "invalid diversifier", 3: "synthesis error", 4: "assignment does not satisfy the circuit",
          5: "not a note of this key", 6: "an output buffer is too small"}
E_NO_NOTE = 5
E_CAPACITY = 6
NOTE_PLAINTEXT_SIZE, ENC_CIPHERTEXT_SIZE = 596, 612
COMPACT_NOTE_SIZE = 84     # the note plaintext without its memo: what a compact (ZIP 307) output carries of enc_ciphertext
OUT_PLAINTEXT_SIZE, OUT_CIPHERTEXT_SIZE = 64, 80     # op = pk_d | esk; out_ciphertext = op under the AEAD and the 16-byte tag


class HostError(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__("masp_host error %d: %s" % (code, ERRORS.get(code, "?")))


def load_library():
    global _lib
    if _lib is None:
        # MASP_HOST_LIBRARY: another build of the same library (tools/sanitize_host.sh runs the CPU tests over an ASan / UBSan build)
        path = os.environ.get("MASP_HOST_LIBRARY") or os.path.join(_HERE, "libmasp_host.so")
        if not os.path.exists(path):
            raise ImportError("libmasp_host.so is not built: run `make -C masp_amd/csrc`")
        L = C.CDLL(path)
        L.masp_host_circuit_setup.restype = C.c_void_p
        L.masp_host_circuit_setup.argtypes = [C.c_int]
        L.masp_host_circuit_free.argtypes = [C.c_void_p]
        L.masp_host_circuit_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.masp_host_circuit_matrix.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.masp_host_circuit_hash.argtypes = [C.c_void_p, C.c_char_p]
        cp, vp, u64 = C.c_char_p, C.c_void_p, C.c_uint64
        L.masp_host_spend_assignment.argtypes = [cp, cp, cp, cp, cp, cp, u64, cp, vp, u64, cp, C.c_int, vp, vp, cp, cp, cp]
        L.masp_host_output_assignment.argtypes = [cp, cp, cp, cp, cp, u64, cp, C.c_int, vp, vp, cp]
        L.masp_host_convert_assignment.argtypes = [cp, u64, cp, vp, u64, cp, C.c_int, vp, vp, cp]
        L.masp_host_spend_assignments.argtypes = [C.c_size_t, vp, C.c_int]
        L.masp_host_fr_from_montgomery.argtypes = [vp, vp, C.c_size_t]
        L.masp_host_fr_from_montgomery.restype = None
        L.masp_host_convert_assignments.argtypes = [C.c_size_t, vp, C.c_int]
        L.masp_host_generator.argtypes = [C.c_int, cp]
        L.masp_host_pedersen_hash.argtypes = [C.c_int, vp, C.c_size_t, cp]
        L.masp_host_asset_identifier.argtypes = [cp, C.c_size_t, cp]
        L.masp_host_asset_generator.argtypes = [cp, cp]
        L.masp_host_value_commitment.argtypes = [cp, u64, cp, cp, cp]
        L.masp_host_note_cmu.argtypes = [cp, u64, cp, cp, cp, cp]
        L.masp_host_sapling_note_nullifiers.argtypes = [C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
        L.masp_host_sapling_build_outputs.argtypes = [C.c_size_t] + [vp] * 18 + [C.c_int]
        L.masp_host_redjubjub_sign_batch.argtypes = [C.c_size_t] + [vp] * 8 + [C.c_int]
        L.masp_host_sapling_build_spends.argtypes = [C.c_size_t] + [vp] * 17 + [C.c_int]
        L.masp_host_merkle_hash.argtypes = [C.c_uint, cp, cp, cp]
        L.masp_host_merkle_empty_roots.argtypes = [vp]
        L.masp_host_merkle_empty_roots.restype = None
        L.masp_host_merkle_tree_complete.argtypes = [C.c_uint, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, vp, vp,
                                                     C.POINTER(C.c_int64), C.c_int]
        if hasattr(L, "masp_host_merkle_tree_append"):
            L.masp_host_merkle_tree_append.argtypes = [u64, vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int64), C.c_int]
        L.masp_host_jubjub_mul.argtypes = [cp, cp, cp]
        L.masp_host_convert_cmu.argtypes = [cp, cp]
        L.masp_host_vk_prepare.restype = vp
        L.masp_host_vk_prepare.argtypes = [vp, C.c_size_t]
        L.masp_host_vk_free.argtypes = [vp]
        L.masp_host_vk_verify.argtypes = [vp, cp, cp, C.c_uint32]
        L.masp_host_vk_verify_batch.argtypes = [vp, C.c_size_t, cp, cp, C.c_uint32, cp]
        L.masp_host_proof_read.argtypes = [cp]
        L.masp_host_point_uv.argtypes = [cp, cp]
        L.masp_host_jubjub_add.argtypes = [cp, cp, C.c_int, cp]
        L.masp_host_jubjub_sum.argtypes = [cp, cp, C.c_size_t, cp, cp]
        L.masp_host_spend_leaf.argtypes = [cp, cp, cp, cp, cp, u64, cp, cp]
        L.masp_host_allowed_conversion.argtypes = [C.c_size_t, cp, cp, cp]
        if hasattr(L, "masp_host_allowed_conversions"):      # (an older build passed as MASP_HOST_LIBRARY lacks it)
            L.masp_host_allowed_conversions.argtypes = [C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int]
        L.masp_host_sapling_ka_agree.argtypes = [cp, cp, cp]
        L.masp_host_diversifier_base.argtypes = [cp, cp]
        L.masp_host_kdf_sapling.argtypes = [cp, cp, cp]
        L.masp_host_kdf_sapling.restype = None
        L.masp_host_prf_expand.argtypes = [cp, C.c_size_t, cp, C.c_size_t, cp]
        L.masp_host_prf_expand.restype = None
        L.masp_host_sapling_rseed_scalar.argtypes = [cp, C.c_int, cp]
        L.masp_host_sapling_rseed_scalar.restype = None
        L.masp_host_chacha20poly1305_encrypt.argtypes = [cp, cp, cp, C.c_size_t, cp, cp]
        L.masp_host_chacha20poly1305_encrypt.restype = None
        L.masp_host_chacha20poly1305_decrypt.argtypes = [cp, cp, cp, C.c_size_t, cp, cp]
        L.masp_host_sapling_note_encrypt.argtypes = [cp, cp, cp, cp, cp, cp]
        L.masp_host_sapling_try_note_decryption.argtypes = [cp, cp, cp, cp, C.c_int, cp, cp]
        L.masp_host_sapling_finish_note_decryption.argtypes = [cp, cp, cp, cp, cp, C.c_int, cp, cp]
        L.masp_host_sapling_try_note_decryption_batch.argtypes = [C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.masp_host_sapling_try_compact_note_decryption.argtypes = [cp, cp, cp, cp, C.c_int, cp, cp]
        L.masp_host_sapling_try_compact_note_decryption_batch.argtypes = [C.c_size_t, vp, C.c_size_t, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp,
                                                                         C.POINTER(C.c_uint64)]
        L.masp_host_prf_ock.argtypes = [cp, cp, cp, cp, cp]
        L.masp_host_prf_ock.restype = None
        L.masp_host_sapling_encrypt_outgoing.argtypes = [cp, cp, cp, cp]
        L.masp_host_sapling_encrypt_outgoing.restype = None
        L.masp_host_sapling_try_output_recovery_with_ock.argtypes = [cp, cp, cp, cp, cp, C.c_int, cp, cp]
        L.masp_host_sapling_try_output_recovery.argtypes = [cp, cp, cp, cp, cp, cp, C.c_int, cp, cp]
        L.masp_host_sapling_try_output_recovery_batch.argtypes = [C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        _lib = L
    return _lib


def effective_cpus():
    """Host threads worth starting: the scheduler affinity, capped by a cgroup CPU quota when one is set (a container
    that sees 256 logical CPUs may be entitled to 16 of them; oversubscribing it only adds contention)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0 and period > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return n


_circuits = {}


def circuit(kind):
    """Static R1CS of a MASP circuit ("spend" | "output" | "convert") and its TestConstraintSystem hash."""
    if kind not in _circuits:
        L = load_library()
        h = L.masp_host_circuit_setup(KINDS[kind])
        if not h:
            raise RuntimeError("circuit setup failed")
        cnt = (C.c_uint32 * 6)()
        L.masp_host_circuit_counts(h, cnt)
        n_in, n_aux, n_con = cnt[0], cnt[1], cnt[2]
        mats = []
        for mi in range(3):
            nnz = cnt[3 + mi]
            rp = np.zeros(n_con + 1, np.uint32)
            col = np.zeros(nnz, np.uint32)
            coef = np.zeros((nnz, 32), np.uint8)
            L.masp_host_circuit_matrix(h, mi, rp.ctypes.data, col.ctypes.data, coef.ctypes.data)
            mats.append((rp, col, coef))
        buf = C.create_string_buffer(65)
        L.masp_host_circuit_hash(h, buf)
        L.masp_host_circuit_free(h)
        _circuits[kind] = (R1cs(n_in, n_aux, n_con, mats), buf.value.decode())
    return _circuits[kind]


def _b(x, n=32):
    if isinstance(x, int):
        return x.to_bytes(n, "little")
    x = bytes(x)
    assert len(x) == n, (len(x), n)
    return x


def _path(siblings):
    assert len(siblings) == TREE_DEPTH
    return np.frombuffer(b"".join(_b(s) for s in siblings), dtype=np.uint8).copy()


def _check(rc):
    if rc:
        raise HostError(rc)


def _aux_buffer(cs, aux_out):
    """The aux assignment is written into `aux_out` when given (e.g. page-locked memory from hip.Context.host_alloc)."""
    if aux_out is None:
        return np.zeros((cs.n_aux, 32), np.uint8)
    assert aux_out.dtype == np.uint8 and aux_out.shape == (cs.n_aux, 32) and aux_out.flags["C_CONTIGUOUS"]
    return aux_out


def spend_assignment(ak, nsk, diversifier, rcm, ar, asset_identifier, value, anchor, path_siblings, position, rcv, check=False,
                     aux_out=None, montgomery=False):
    """-> (inputs u8[8,32], aux u8[100497,32], cv, rk, nf)   — SaplingProvingContext::spend_proof up to the prover call.
    montgomery: aux leaves as Montgomery residues (blst_fr memory; masp_hip_job.aux_form = 1) instead of canonical bytes."""
    L = load_library()
    cs, _ = circuit("spend")
    inputs = np.zeros((cs.n_inputs, 32), np.uint8)
    aux = _aux_buffer(cs, aux_out)
    cv, rk, nf = (C.create_string_buffer(32) for _ in range(3))
    p = _path(path_siblings)
    _check(L.masp_host_spend_assignment(_b(ak), _b(nsk), _b(diversifier, 11), _b(rcm), _b(ar), _b(asset_identifier), value, _b(anchor),
                                        p.ctypes.data, position, _b(rcv), (1 if check else 0) | (2 if montgomery else 0), inputs.ctypes.data,
                                        aux.ctypes.data, cv, rk, nf))
    return inputs, aux, cv.raw, rk.raw, nf.raw


def output_assignment(esk, diversifier, pk_d, rcm, asset_identifier, value, rcv, check=False, aux_out=None, montgomery=False):
    L = load_library()
    cs, _ = circuit("output")
    inputs = np.zeros((cs.n_inputs, 32), np.uint8)
    aux = _aux_buffer(cs, aux_out)
    cv = C.create_string_buffer(32)
    _check(L.masp_host_output_assignment(_b(esk), _b(diversifier, 11), _b(pk_d), _b(rcm), _b(asset_identifier), value, _b(rcv),
                                         (1 if check else 0) | (2 if montgomery else 0), inputs.ctypes.data, aux.ctypes.data, cv))
    return inputs, aux, cv.raw


def convert_assignment(generator, value, anchor, path_siblings, position, rcv, check=False, aux_out=None, montgomery=False):
    L = load_library()
    cs, _ = circuit("convert")
    inputs = np.zeros((cs.n_inputs, 32), np.uint8)
    aux = _aux_buffer(cs, aux_out)
    cv = C.create_string_buffer(32)
    p = _path(path_siblings)
    _check(L.masp_host_convert_assignment(_b(generator), value, _b(anchor), p.ctypes.data, position, _b(rcv),
                                          (1 if check else 0) | (2 if montgomery else 0), inputs.ctypes.data, aux.ctypes.data, cv))
    return inputs, aux, cv.raw


def aux_from_montgomery(aux):
    """u8[n,32] of Montgomery residues (what the synthesizers write with montgomery=True) -> u8[n,32] canonical little-endian values."""
    L = load_library()
    aux = np.ascontiguousarray(aux, dtype=np.uint8)
    out = np.zeros_like(aux)
    L.masp_host_fr_from_montgomery(aux.ctypes.data, out.ctypes.data, aux.shape[0])
    return out


# ---- several witnesses per call: their Merkle blocks run in lockstep (csrc/host/circuits.h merkle_block_batch) ----
GROUP = 16      # witnesses per call: 3 x 16 chains of affine additions share every field inversion; 256 witnesses = 16 calls


class _SpendJob(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ak", "nsk", "diversifier", "rcm", "ar", "asset_identifier")] + [("value", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("anchor", "path_siblings")] + [("position", C.c_uint64), ("rcv", C.c_void_p)] + \
               [(n, C.c_void_p) for n in ("inputs", "aux", "cv_out", "rk_out", "nf_out")] + [("rc", C.c_int)]


class _ConvertJob(C.Structure):
    _fields_ = [("generator", C.c_void_p), ("value", C.c_uint64), ("anchor", C.c_void_p), ("path_siblings", C.c_void_p), ("position", C.c_uint64),
                ("rcv", C.c_void_p), ("inputs", C.c_void_p), ("aux", C.c_void_p), ("cv_out", C.c_void_p), ("rc", C.c_int)]


def _pin(keep, data, n=32):
    buf = C.create_string_buffer(_b(data, n), n)
    keep.append(buf)
    return C.addressof(buf)


def spend_assignments(items, check=False, aux_outs=None, montgomery=False):
    """items: list of (ak, nsk, diversifier, rcm, ar, asset_identifier, value, anchor, path_siblings, position, rcv) — the arguments of
    spend_assignment — synthesised in ONE native call (masp_host_spend_assignments: the Merkle blocks of the witnesses run side
    by side, ~1.8x the witnesses per second of the one-by-one call).  -> list of (inputs, aux, cv, rk, nf) or HostError instances."""
    L = load_library()
    cs, _ = circuit("spend")
    n = len(items)
    jobs = (_SpendJob * n)()
    keep, outs = [], []
    for j, (ak, nsk, d, rcm, ar, ident, value, anchor, sib, pos, rcv) in enumerate(items):
        inputs = np.zeros((cs.n_inputs, 32), np.uint8)
        aux = _aux_buffer(cs, aux_outs[j] if aux_outs else None)
        path = _path(sib)
        keep.append(path)
        o = C.create_string_buffer(96)
        J = jobs[j]
        J.ak, J.nsk, J.diversifier, J.rcm, J.ar, J.asset_identifier = (_pin(keep, ak), _pin(keep, nsk), _pin(keep, d, 11), _pin(keep, rcm),
                                                                       _pin(keep, ar), _pin(keep, ident))
        J.value, J.anchor, J.path_siblings, J.position, J.rcv = value, _pin(keep, anchor), path.ctypes.data, pos, _pin(keep, rcv)
        J.inputs, J.aux = inputs.ctypes.data, aux.ctypes.data
        J.cv_out, J.rk_out, J.nf_out = C.addressof(o), C.addressof(o) + 32, C.addressof(o) + 64
        outs.append((inputs, aux, o))
    L.masp_host_spend_assignments(n, jobs, (1 if check else 0) | (2 if montgomery else 0))
    return [HostError(jobs[j].rc) if jobs[j].rc else (i, a, o.raw[:32], o.raw[32:64], o.raw[64:]) for j, (i, a, o) in enumerate(outs)]


def convert_assignments(items, check=False, aux_outs=None, montgomery=False):
    """items: list of (generator, value, anchor, path_siblings, position, rcv) -> list of (inputs, aux, cv) or HostError instances."""
    L = load_library()
    cs, _ = circuit("convert")
    n = len(items)
    jobs = (_ConvertJob * n)()
    keep, outs = [], []
    for j, (gen, value, anchor, sib, pos, rcv) in enumerate(items):
        inputs = np.zeros((cs.n_inputs, 32), np.uint8)
        aux = _aux_buffer(cs, aux_outs[j] if aux_outs else None)
        path = _path(sib)
        keep.append(path)
        o = C.create_string_buffer(32)
        J = jobs[j]
        J.generator, J.value, J.anchor, J.path_siblings, J.position, J.rcv = _pin(keep, gen), value, _pin(keep, anchor), path.ctypes.data, pos, _pin(keep, rcv)
        J.inputs, J.aux, J.cv_out = inputs.ctypes.data, aux.ctypes.data, C.addressof(o)
        outs.append((inputs, aux, o))
    L.masp_host_convert_assignments(n, jobs, (1 if check else 0) | (2 if montgomery else 0))
    return [HostError(jobs[j].rc) if jobs[j].rc else (i, a, o.raw) for j, (i, a, o) in enumerate(outs)]


class PreparedVerifyingKey:
    """= bellman `prepare_verifying_key(&params.vk)` (lib.rs:391-393) + `verify_proof` (sapling/prover.rs:148,266)."""

    def __init__(self, params):
        buf = np.frombuffer(params, dtype=np.uint8) if isinstance(params, (bytes, bytearray, memoryview)) else np.ascontiguousarray(params, dtype=np.uint8)
        n_ic = int.from_bytes(buf[864:868].tobytes(), "big")
        self._buf = buf[:868 + 96 * n_ic].copy()
        self._L = load_library()
        self._h = self._L.masp_host_vk_prepare(self._buf.ctypes.data, self._buf.size)
        if not self._h:
            raise ValueError("malformed verifying key")

    def verify(self, proof, public_inputs):
        """public_inputs: ints or 32-byte LE values, excluding ONE -> True / False"""
        pi = b"".join(_b(x) for x in public_inputs)
        rc = self._L.masp_host_vk_verify(self._h, bytes(proof), pi, len(public_inputs))
        if rc < 0:
            return False
        return rc == 1

    def verify_batch(self, proofs, public_inputs, randomness=None):
        """= bellman `verify_proofs_batch` (sapling/verifier/batch.rs:24-31): one random linear combination, n + 2 Miller
        loops and a single final exponentiation for n proofs.  public_inputs: one list per proof.  True iff all verify
        (up to 2^-128); False says at least one is invalid, not which."""
        import secrets
        n = len(proofs)
        if n == 0:
            return True
        k = len(public_inputs[0])
        if any(len(pi) != k for pi in public_inputs) or len(public_inputs) != n:
            return False
        pi = b"".join(_b(x) for row in public_inputs for x in row)
        z = randomness if randomness is not None else secrets.token_bytes(16 * n)
        assert len(z) == 16 * n
        return self._L.masp_host_vk_verify_batch(self._h, n, b"".join(bytes(p) for p in proofs), pi, k, z) == 1

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.masp_host_vk_free(self._h)
            self._h = None


def proof_read(proof):
    """bellman `Proof::read` alone (masp_host_proof_read): True if the 192 bytes are three points it accepts."""
    proof = bytes(proof)
    return len(proof) == 192 and load_library().masp_host_proof_read(proof) == 1


# ---- native primitives ----
GENERATOR_NAMES = ["proof_generation_key_generator", "note_commitment_randomness_generator", "nullifier_position_generator",
                   "value_commitment_randomness_generator", "spending_key_generator"]


def generator_uv(which):
    out = C.create_string_buffer(64)
    load_library().masp_host_generator(which, out)
    return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def point_bytes(u, v):
    return (v | ((u & 1) << 255)).to_bytes(32, "little")


def pedersen_hash(personalization, bits):
    """personalization: -1 for NoteCommitment, else MerkleTree depth; bits: iterable of 0/1 -> (u, v)"""
    b = np.array(list(bits), dtype=np.uint8)
    out = C.create_string_buffer(64)
    load_library().masp_host_pedersen_hash(personalization, b.ctypes.data, b.size, out)
    return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def asset_identifier(name):
    out = C.create_string_buffer(32)
    if load_library().masp_host_asset_identifier(bytes(name), len(name), out):
        raise ValueError("no valid asset identifier")
    return out.raw


def asset_generator(identifier):
    out = C.create_string_buffer(32)
    if load_library().masp_host_asset_generator(_b(identifier), out):
        raise ValueError("invalid asset identifier")
    return out.raw


def value_commitment(identifier, value, rcv):
    out, uv = C.create_string_buffer(32), C.create_string_buffer(64)
    if load_library().masp_host_value_commitment(_b(identifier), value, _b(rcv), out, uv):
        raise ValueError("invalid asset identifier")
    return out.raw, int.from_bytes(uv.raw[:32], "little"), int.from_bytes(uv.raw[32:], "little")


def note_cmu(identifier, value, diversifier, pk_d, rcm):
    out = C.create_string_buffer(32)
    if load_library().masp_host_note_cmu(_b(identifier), value, _b(diversifier, 11), _b(pk_d), _b(rcm), out):
        raise ValueError("invalid note")
    return out.raw


def note_nullifier_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, nks, positions):
    """the arguments of either note_nullifiers as contiguous arrays: uint8[n, 32] (bytes or arrays), uint64[n], uint8[n, 11], uint8[n]"""
    def u8(a, w):
        if isinstance(a, (bytes, bytearray, memoryview)):
            a = np.frombuffer(a, dtype=np.uint8)
        return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, w) if w else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    out = (u8(asset_identifiers, 32), np.ascontiguousarray(values, dtype=np.uint64).reshape(-1), u8(diversifiers, 11), u8(pk_ds, 32),
           u8(lead_bytes, 0), u8(rseeds, 32), u8(nks, 32), np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1))
    n = out[0].shape[0]
    if any(a.shape[0] != n for a in out):
        raise ValueError("note_nullifiers: the arrays differ in length: %s" % ([a.shape[0] for a in out],))
    return out


def note_nullifiers(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, nks, positions, threads=None, want_cmus=True):
    """masp_host_sapling_note_nullifiers: Note::cmu and Note::nf(&nk, position) for n notes on host threads (default: effective_cpus()).
    Arrays in (n x 32 bytes each, diversifiers n x 11, values / positions / lead bytes n) -> (status uint8[n], cmus uint8[n, 32] or None
    with want_cmus=False, nfs uint8[n, 32]).  status: 0, or 1 asset identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 nk; such a note's
    outputs are zeros."""
    args = note_nullifier_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, nks, positions)
    n = args[0].shape[0]
    status, nfs = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    cmus = np.zeros((n, 32), np.uint8) if want_cmus else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _check(load_library().masp_host_sapling_note_nullifiers(n, *[vp(a) for a in args], vp(status), vp(cmus), vp(nfs),
                                                           int(threads or effective_cpus())))
    return status, cmus, nfs


def build_output_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, esks, rcvs, memos, ovks, ovk_flags, out_randoms):
    """the arguments of either build_outputs as contiguous arrays, in the C ABI's order: uint8[n, 32] (bytes or arrays), uint64[n],
    uint8[n, 11], uint8[n], uint8[n, 512], uint8[n, 96]; esks, memos, ovk_flags and out_randoms may be None and stay None"""
    def u8(a, w):
        if a is None:
            return None
        if isinstance(a, (bytes, bytearray, memoryview)):
            a = np.frombuffer(a, dtype=np.uint8)
        return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, w) if w else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    out = (u8(asset_identifiers, 32), np.ascontiguousarray(values, dtype=np.uint64).reshape(-1), u8(diversifiers, 11), u8(pk_ds, 32),
           u8(lead_bytes, 0), u8(rseeds, 32), u8(esks, 32), u8(rcvs, 32), u8(memos, 512), u8(ovks, 32), u8(ovk_flags, 0), u8(out_randoms, 96))
    n = out[0].shape[0]
    if any(a is not None and a.shape[0] != n for a in out):
        raise ValueError("build_outputs: the arrays differ in length: %s" % ([None if a is None else a.shape[0] for a in out],))
    return out


def build_output_results(n):
    """(status uint8[n], cvs, cmus, epks uint8[n, 32], encs uint8[n, 612], couts uint8[n, 80]), zeroed"""
    return (np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8),
            np.zeros((n, ENC_CIPHERTEXT_SIZE), np.uint8), np.zeros((n, OUT_CIPHERTEXT_SIZE), np.uint8))


def build_outputs(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, esks, rcvs, memos, ovks, ovk_flags=None, out_randoms=None,
                  threads=None):
    """masp_host_sapling_build_outputs: cv, cmu, epk, enc_ciphertext and out_ciphertext of n outputs on host threads (default:
    effective_cpus()).  Arrays in, in the C ABI's order (n x 32 bytes each, diversifiers n x 11, values / lead bytes / ovk flags n, memos
    n x 512, out_randoms n x 96); esks (no lead byte is 1), memos (every memo empty), ovk_flags (every ovk present) and out_randoms (no flag
    is 0) may be None -> (status uint8[n], cvs, cmus, epks uint8[n, 32], encs uint8[n, 612], couts uint8[n, 80]).  status: 0, or 1 asset
    identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 esk, 6 rcv; such an output's outputs are zeros.  No randomness is drawn."""
    args = build_output_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, esks, rcvs, memos, ovks, ovk_flags, out_randoms)
    n = args[0].shape[0]
    res = build_output_results(n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _check(load_library().masp_host_sapling_build_outputs(n, *[vp(a) for a in args], *[vp(a) for a in res], int(threads or effective_cpus())))
    return res


def _rows(a, w):
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, w) if w else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def sign_batch_args(sks, alphas, sighashes, kinds, randoms):
    """the arguments of either redjubjub_sign_batch as contiguous arrays, in the C ABI's order: uint8[n, 32] (bytes or arrays), uint8[n],
    uint8[n, 80]; alphas may be None and stays None"""
    out = (_rows(sks, 32), _rows(alphas, 32), _rows(sighashes, 32), _rows(kinds, 0), _rows(randoms, 80))
    n = out[0].shape[0]
    if any(a is not None and a.shape[0] != n for a in out):
        raise ValueError("redjubjub_sign_batch: the arrays differ in length: %s" % ([None if a is None else a.shape[0] for a in out],))
    return out


def redjubjub_sign_batch(sks, alphas, sighashes, kinds, randoms, threads=None, want_vks=True):
    """masp_host_redjubjub_sign_batch: n RedJubjub signatures on host threads (default: effective_cpus()): rsk = sk + alpha, vk = [rsk] G_kind,
    sig = Rbar | S with the nonce from the item's 80 bytes of randoms.  sks, alphas (or None: no randomisation), sighashes n x 32, kinds n
    (0 spend authorisation, 1 binding), randoms n x 80 -> (status uint8[n], vks uint8[n, 32] or None with want_vks=False, sigs uint8[n, 64]).
    status: 0, or 1 sk >= r_J, 2 alpha >= r_J; such an item's outputs are zeros.  No randomness is drawn."""
    args = sign_batch_args(sks, alphas, sighashes, kinds, randoms)
    n = args[0].shape[0]
    status, sigs = np.zeros(n, np.uint8), np.zeros((n, 64), np.uint8)
    vks = np.zeros((n, 32), np.uint8) if want_vks else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _check(load_library().masp_host_redjubjub_sign_batch(n, *[vp(a) for a in args], vp(status), vp(vks), vp(sigs), int(threads or effective_cpus())))
    return status, vks, sigs


def build_spend_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, positions):
    """the arguments of either build_spends as contiguous arrays, in the C ABI's order: uint8[n, 32] (bytes or arrays), uint64[n],
    uint8[n, 11], uint8[n]"""
    out = (_rows(asset_identifiers, 32), np.ascontiguousarray(values, dtype=np.uint64).reshape(-1), _rows(diversifiers, 11), _rows(pk_ds, 32),
           _rows(lead_bytes, 0), _rows(rseeds, 32), _rows(aks, 32), _rows(nsks, 32), _rows(ars, 32), _rows(rcvs, 32),
           np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1))
    n = out[0].shape[0]
    if any(a.shape[0] != n for a in out):
        raise ValueError("build_spends: the arrays differ in length: %s" % ([a.shape[0] for a in out],))
    return out


def build_spend_results(n, want_cmus=True, want_nks=True):
    """(status uint8[n], cvs, rks, nfs uint8[n, 32], cmus, nks uint8[n, 32] or None), zeroed"""
    z = lambda: np.zeros((n, 32), np.uint8)
    return (np.zeros(n, np.uint8), z(), z(), z(), z() if want_cmus else None, z() if want_nks else None)


def build_spends(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, positions, threads=None,
                 want_cmus=True, want_nks=True):
    """masp_host_sapling_build_spends: cv, rk, nf, cmu and nk of n spends on host threads (default: effective_cpus()).  Arrays in, in the C
    ABI's order (n x 32 bytes each, diversifiers n x 11, values / lead bytes / positions n) -> (status uint8[n], cvs, rks, nfs uint8[n, 32],
    cmus, nks uint8[n, 32] or None where not wanted).  status: 0, or 1 asset identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 ak does
    not decode, 6 ak of small order, 7 nsk, 8 ar, 9 rcv; such a spend's outputs are zeros.  No randomness is drawn."""
    args = build_spend_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, positions)
    n = args[0].shape[0]
    res = build_spend_results(n, want_cmus, want_nks)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _check(load_library().masp_host_sapling_build_spends(n, *[vp(a) for a in args], *[vp(a) for a in res], int(threads or effective_cpus())))
    return res


def merkle_hash(depth, lhs, rhs):
    out = C.create_string_buffer(32)
    if load_library().masp_host_merkle_hash(depth, _b(lhs), _b(rhs), out):
        raise ValueError("non-canonical node")
    return out.raw


def merkle_empty_roots():
    """empty_root(0..32) as a (33, 32) uint8 array: the uncommitted leaf 1 and the roots of the empty subtrees above it"""
    out = np.zeros((33, 32), np.uint8)
    load_library().masp_host_merkle_empty_roots(out.ctypes.data_as(C.c_void_p))
    return out


def merkle_tree_complete(row, height0=0, positions=(), want_nodes=True, threads=None, nodes_capacity=None):
    """masp_host_merkle_tree_complete: FrozenCommitmentTree::complete over `row` (n x 32 bytes, nodes of level height0) on host threads
    -> (nodes uint8[N, 32] or None, root bytes, paths uint8[len(positions), 32 - height0, 32]).  A node that is not canonical or a
    position >= n raises ValueError (with .bad_index); nodes_capacity: room for that many nodes (default: what the call asks for)."""
    L = load_library()
    row = np.ascontiguousarray(np.frombuffer(row, np.uint8) if isinstance(row, (bytes, bytearray, memoryview)) else row, dtype=np.uint8).reshape(-1, 32)
    pos = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
    n, depth = row.shape[0], max(0, TREE_DEPTH - int(height0))
    paths = np.zeros((pos.shape[0], depth, 32), np.uint8)
    root = np.zeros(32, np.uint8)
    nn, bad = C.c_size_t(0), C.c_int64(-1)
    threads = effective_cpus() if threads is None else int(threads)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    if want_nodes and nodes_capacity is None:
        nodes_capacity = merkle_node_count(n, height0)
    nodes =np.zeros((int(nodes_capacity), 32), np.uint8) if want_nodes else None
    rc = L.masp_host_merkle_tree_complete(int(height0), n, vp(row), nodes.ctypes.data_as(C.c_void_p) if want_nodes else None,
                                          int(nodes_capacity or 0), C.byref(nn), root.ctypes.data_as(C.c_void_p), pos.shape[0], vp(pos),
                                          paths.ctypes.data_as(C.c_void_p), C.byref(bad), threads)
    if rc:
        e = ValueError("merkle_tree_complete: %s" % ("node %d is not canonical" % bad.value if bad.value >= 0 else ERRORS.get(rc, rc)))
        e.code, e.bad_index, e.needed = rc, bad.value, nn.value
        raise e
    return (nodes[:nn.value] if want_nodes else None), root.tobytes(), paths


def merkle_node_count(n, height0=0):
    """the length of the node vector FrozenCommitmentTree::complete builds over n nodes of level height0"""
    if n == 0:
        return 0
    total, width = 0, n
    for _ in range(TREE_DEPTH - height0):
        width += width & 1
        total += width
        width //= 2
    return total + width


def merkle_append_node_count(start, n):
    """the number of nodes merkle_tree_append returns: the complete nodes of levels 1..32 whose last leaf is in [start, start + n)"""
    return sum(((start + n) >> h) - (start >> h) for h in range(1, TREE_DEPTH + 1))


def merkle_append_args(start, frontier, row):
    """the arguments of either merkle_tree_append as arrays: (row uint8[n, 32], frontier uint8[32, 32])"""
    if not 0 <= int(start) <= 1 << TREE_DEPTH:
        raise ValueError("merkle_tree_append: start %d is not a position of the depth-%d tree" % (start, TREE_DEPTH))
    row = np.ascontiguousarray(np.frombuffer(row, np.uint8) if isinstance(row, (bytes, bytearray, memoryview)) else row, dtype=np.uint8).reshape(-1, 32)
    if frontier is None:
        frontier = np.zeros((TREE_DEPTH, 32), np.uint8)
    elif isinstance(frontier, (bytes, bytearray, memoryview)):
        frontier = np.frombuffer(frontier, np.uint8)
    frontier = np.ascontiguousarray(frontier, dtype=np.uint8).reshape(TREE_DEPTH, 32)
    return row, frontier


def merkle_append_error(name, bad):
    return "%s: %s" % (name, "node %d is not canonical" % bad if bad >= 0 else "frontier entry %d is not canonical" % (-2 - bad))


def merkle_tree_append(start, frontier, row, threads=None, nodes_capacity=None):
    """masp_host_merkle_tree_append: the leaves `row` (n x 32 bytes) at positions start .. start + n - 1 of the depth-32 tree; frontier
    (32 x 32 bytes or None with start = 0): entry h the node (h, (start >> h) - 1), read where bit h of start is set -> uint8[N, 32], for
    h = 1..32 in turn the nodes (h, i) with start >> h <= i < (start + n) >> h.  A node that is not canonical raises ValueError with
    .bad_index (the row's index, or -2 - h for frontier entry h); start + n > 2^32 raises ValueError too."""
    L = load_library()
    row, frontier = merkle_append_args(start, frontier, row)
    n = row.shape[0]
    if nodes_capacity is None:
        nodes_capacity = merkle_append_node_count(int(start), n)
    nodes = np.zeros((max(1, int(nodes_capacity)), 32), np.uint8)
    nn, bad = C.c_size_t(0), C.c_int64(-1)
    threads = effective_cpus() if threads is None else int(threads)
    rc = L.masp_host_merkle_tree_append(int(start), frontier.ctypes.data_as(C.c_void_p), n, row.ctypes.data_as(C.c_void_p) if n else None,
                                        nodes.ctypes.data_as(C.c_void_p), int(nodes_capacity), C.byref(nn), C.byref(bad), threads)
    if rc:
        e = ValueError(merkle_append_error("merkle_tree_append", bad.value) if bad.value != -1 else
                       "merkle_tree_append: %s" % ERRORS.get(rc, rc))
        e.code, e.bad_index, e.needed = rc, bad.value, nn.value
        raise e
    return nodes[:nn.value]


def jubjub_mul(point, scalar):
    out = C.create_string_buffer(32)
    if load_library().masp_host_jubjub_mul(_b(point), _b(scalar), out):
        raise ValueError("invalid point")
    return out.raw


def point_uv(point):
    out = C.create_string_buffer(64)
    if load_library().masp_host_point_uv(_b(point), out):
        raise ValueError("invalid point")
    return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def multipack(data):
    """bellman multipack::compute_multipacking(bytes_to_bits_le(data)): 254-bit little-endian chunks (sapling/prover.rs:138-139)"""
    # (bit i of the little-endian integer is bit i of bytes_to_bits_le: the chunks are 254-bit digits of that integer — 49 us per
    # nullifier as a list of bits, under the GIL of the thread that is about to start a chunk's self-verification)
    v, nbits = int.from_bytes(bytes(data), "little"), 8 * len(data)
    return [(v >> o) & ((1 << 254) - 1) for o in range(0, nbits, 254)]


def jubjub_add(p, q, subtract=False):
    out = C.create_string_buffer(32)
    if load_library().masp_host_jubjub_add(_b(p), _b(q), 1 if subtract else 0, out):
        raise ValueError("invalid point")
    return out.raw


JUBJUB_IDENTITY = (1).to_bytes(32, "little")   # (u, v) = (0, 1)


def jubjub_sum(points, subtract=None, acc=JUBJUB_IDENTITY):
    """acc + sum of the compressed points (those with a true `subtract` flag subtracted) in one native call."""
    pts = b"".join(_b(p) for p in points)
    flags = bytes(1 if f else 0 for f in subtract) if subtract is not None else None
    out = C.create_string_buffer(32)
    if load_library().masp_host_jubjub_sum(_b(acc), pts, len(points), flags, out):
        raise ValueError("invalid point")
    return out.raw


def convert_cmu(generator):
    out = C.create_string_buffer(32)
    if load_library().masp_host_convert_cmu(_b(generator), out):
        raise ValueError("invalid point")
    return out.raw


def compact_size(n):
    """zcash_encoding's CompactSize::write"""
    if n < 253:
        return bytes([n])
    for lead, width in ((253, 2), (254, 4), (255, 8)):
        if n < 1 << (8 * width):
            return bytes([lead]) + n.to_bytes(width, "little")
    raise ValueError("no CompactSize holds %d" % n)


def read_compact_size(data, at=0):
    """CompactSize::read at data[at:] -> (value, the offset behind it); ValueError for a short or non-canonical encoding"""
    if len(data) <= at:
        raise ValueError("CompactSize: no bytes left")
    lead = data[at]
    if lead < 253:
        return lead, at + 1
    width = {253: 2, 254: 4, 255: 8}[lead]
    if len(data) < at + 1 + width:
        raise ValueError("CompactSize: no bytes left")
    n = int.from_bytes(data[at + 1:at + 1 + width], "little")
    if n < (253, 1 << 16, 1 << 32)[lead - 253]:
        raise ValueError("non-canonical CompactSize")
    return n, at + 1 + width


def allowed_conversion_args(term_offsets, identifiers, values):
    """the arguments of either allowed_conversions as contiguous arrays: uint64[n_conv + 1], uint8[n_terms, 32], uint8[n_terms, 16].
    values: n_terms x 16 bytes (bytes or a uint8 array), or a sequence of Python integers, written as little-endian i128."""
    off = np.ascontiguousarray(term_offsets, dtype=np.uint64).reshape(-1)
    if isinstance(identifiers, (bytes, bytearray, memoryview)):
        identifiers = np.frombuffer(identifiers, dtype=np.uint8)
    ids = np.ascontiguousarray(identifiers, dtype=np.uint8).reshape(-1, 32)
    if isinstance(values, (bytes, bytearray, memoryview)):
        values = np.frombuffer(values, dtype=np.uint8)
    elif not isinstance(values, np.ndarray):
        values = np.frombuffer(b"".join(int(v).to_bytes(16, "little", signed=True) for v in values), dtype=np.uint8)
    vals = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 16)
    if ids.shape[0] != vals.shape[0]:
        raise ValueError("allowed_conversions: %d identifiers, %d values" % (ids.shape[0], vals.shape[0]))
    return off, ids, vals


def allowed_conversions(term_offsets, identifiers, values, threads=None, want_generators=True):
    """masp_host_allowed_conversions: generator and tree leaf of n_conv conversions on host threads (default: effective_cpus()).
    Conversion c owns the terms term_offsets[c] .. term_offsets[c + 1] - 1, summed as given -> (status uint8[n_conv], generators
    uint8[n_conv, 32] or None with want_generators=False, cmus uint8[n_conv, 32]).  status: 0, or 1 an identifier without a generator,
    else 2 a value that is i128::MIN; such a conversion's outputs are zeros."""
    off, ids, vals = allowed_conversion_args(term_offsets, identifiers, values)
    n = max(off.shape[0] - 1, 0)
    status, cmus = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    gens = np.zeros((n, 32), np.uint8) if want_generators else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    _check(load_library().masp_host_allowed_conversions(n, vp(off), ids.shape[0], vp(ids), vp(vals), vp(status), vp(gens), vp(cmus),
                                                        int(threads or effective_cpus())))
    return status, gens, cmus


class AllowedConversion:
    """= masp_primitives::convert::AllowedConversion (/root/reference/masp_primitives/src/convert.rs:22-84,86-118).

    `AllowedConversion(assets)` mirrors `From<I128Sum>`: assets = iterable of (asset identifier[32], signed 128-bit
    value) — the components of the reference's I128Sum; generator = sum_i sign(v_i) [|v_i| as u64] asset_generator_i,
    cofactor not cleared.  i128::MIN raises ValueError (the reference panics "invalid conversion")."""

    def __init__(self, assets):
        merged = {}
        for ident, value in (assets.items() if isinstance(assets, dict) else assets):
            ident = _b(ident)
            merged[ident] = merged.get(ident, 0) + int(value)          # ValueSum addition merges equal asset types
        self.assets = {k: v for k, v in sorted(merged.items()) if v != 0}
        for v in self.assets.values():
            if not -(1 << 127) <= v < (1 << 127):
                raise OverflowError("value does not fit an i128")
        ids = b"".join(self.assets.keys())
        vals = b"".join(v.to_bytes(16, "little", signed=True) for v in self.assets.values())
        out = C.create_string_buffer(32)
        if load_library().masp_host_allowed_conversion(len(self.assets), ids, vals, out):
            raise ValueError("invalid conversion")
        self.generator = out.raw

    _cmu = None

    @classmethod
    def from_parts(cls, assets, generator, cmu=None):
        """The conversion of an already merged value sum (a dict or pairs of identifier and value) whose generator, and leaf if given, are
        already known — from allowed_conversions, which computes many in one call — without any native call."""
        self = cls.__new__(cls)
        self.assets = {_b(k): int(v) for k, v in sorted(dict(assets).items()) if int(v) != 0}
        self.generator = _b(generator)
        self._cmu = _b(cmu) if cmu is not None else None
        return self

    def cmu(self):
        """u-coordinate of PedersenHash(NoteCommitment, repr(generator)) (convert.rs:39-64), 32 bytes LE."""
        return self._cmu if self._cmu is not None else convert_cmu(self.generator)

    def write(self):
        """BorshSerialize (convert.rs:138-144): I128Sum::write (amount.rs:361-368: a CompactSize count, then identifier 32 | value i128 LE 16
        per component in identifier order) and the generator's 32 bytes."""
        return compact_size(len(self.assets)) + b"".join(k + v.to_bytes(16, "little", signed=True) for k, v in self.assets.items()) + \
            self.generator

    @staticmethod
    def parse(data, check_identifiers=True):
        """-> (merged assets, generator bytes) of a serialised conversion, as UncheckedAllowedConversion reads it (convert.rs:219-232): the
        pairs summed as I128Sum::read sums them (amount.rs:345-357), the generator decoded.  ValueError: the bytes end early or go on, the
        count is not a canonical CompactSize, a sum leaves the i128, the generator does not decode — and, with check_identifiers, an
        identifier has no generator (a batch leaves that to its one call)."""
        data = bytes(data)
        n, at = read_compact_size(data)
        if len(data) != at + 48 * n + 32:
            raise ValueError("allowed conversion: %d bytes for %d components" % (len(data), n))
        merged = {}
        for i in range(n):
            ident = data[at + 48 * i:at + 48 * i + 32]
            if check_identifiers:
                asset_generator(ident)
            total = merged.get(ident, 0) + int.from_bytes(data[at + 48 * i + 32:at + 48 * i + 48], "little", signed=True)
            if not -(1 << 127) <= total < (1 << 127):
                raise ValueError("allowed conversion: the sum does not fit an i128")
            merged[ident] = total
        generator = data[at + 48 * n:]
        point_uv(generator)
        return {k: v for k, v in sorted(merged.items()) if v != 0}, generator

    @classmethod
    def read_unchecked(cls, data):
        """UncheckedAllowedConversion's read (convert.rs:219-232): the generator is decoded and otherwise believed."""
        return cls.from_parts(*cls.parse(data))

    @classmethod
    def read(cls, data):
        """BorshDeserialize (convert.rs:146-160): the generator is recomputed from the value sum; ValueError if it is another."""
        assets, generator = cls.parse(data)
        conv = cls(assets)
        if conv.generator != generator:
            raise ValueError("allowed conversion: the generator is not the value sum's")
        return conv

    commitment = cmu      # Node::from_scalar(self.cmu()) (convert.rs:80-84): the leaf of the conversion tree

    def value_commitment(self, value, randomness):
        """-> the commitment point cv = [value]([8]generator) + [randomness]G_vcr, 32 bytes (convert.rs:70-77, sapling.rs:204-209)."""
        h = jubjub_mul(jubjub_mul(self.generator, 8), value)
        g_rcv = point_bytes(*generator_uv(3))
        return jubjub_add(h, jubjub_mul(g_rcv, randomness))

    @staticmethod
    def uncommitted():
        return 1          # bls12_381::Scalar::ONE (convert.rs:32-36)


def spend_leaf(ak, nsk, diversifier, rcm, asset_identifier, value):
    """(cmu, pk_d) of the note a Spend proves knowledge of: nk = [nsk]G, ivk = CRH(ak, nk), pk_d = [ivk] g_d."""
    cmu, pk_d = C.create_string_buffer(32), C.create_string_buffer(32)
    _check(load_library().masp_host_spend_leaf(_b(ak), _b(nsk), _b(diversifier, 11), _b(rcm), _b(asset_identifier), value, cmu, pk_d))
    return cmu.raw, pk_d.raw


def merkle_root(leaf, path_siblings, position):
    """Root of the depth-32 tree from a leaf, its siblings (leaf level first) and its position."""
    cur = _b(leaf)
    for i, sib in enumerate(path_siblings):
        cur = merkle_hash(i, _b(sib), cur) if (position >> i) & 1 else merkle_hash(i, cur, _b(sib))
    return cur


# ---- Sapling note encryption and trial decryption (csrc/host/note_encryption.h) ----
def sapling_ka_agree(sk, point):
    """[8 sk] P as 32 bytes (sapling_ka_agree)"""
    out = C.create_string_buffer(32)
    _check(load_library().masp_host_sapling_ka_agree(_b(sk), _b(point), out))
    return out.raw


def diversifier_base(diversifier):
    """Diversifier::g_d as 32 bytes; HostError(2) if the diversifier has none"""
    out = C.create_string_buffer(32)
    _check(load_library().masp_host_diversifier_base(_b(diversifier, 11), out))
    return out.raw


def kdf_sapling(secret, epk):
    out = C.create_string_buffer(32)
    load_library().masp_host_kdf_sapling(_b(secret), _b(epk), out)
    return out.raw


def prf_expand(sk, t):
    out = C.create_string_buffer(64)
    sk, t = bytes(sk), bytes(t)
    load_library().masp_host_prf_expand(sk, len(sk), t, len(t), out)
    return out.raw


def sapling_rseed_scalar(rseed, domain):
    """PRF^expand(rseed, [domain]) mod r_J as 32 bytes: domain 4 = rcm, 5 = esk"""
    out = C.create_string_buffer(32)
    load_library().masp_host_sapling_rseed_scalar(_b(rseed), domain, out)
    return out.raw


def chacha20poly1305_encrypt(key, nonce, plaintext):
    """-> (ciphertext, tag); no associated data"""
    plaintext = bytes(plaintext)
    ct, tag = C.create_string_buffer(max(1, len(plaintext))), C.create_string_buffer(16)
    load_library().masp_host_chacha20poly1305_encrypt(_b(key), _b(nonce, 12), plaintext, len(plaintext), ct, tag)
    return ct.raw[:len(plaintext)], tag.raw


def chacha20poly1305_decrypt(key, nonce, ciphertext, tag):
    """-> plaintext, or None if the tag does not verify"""
    ciphertext = bytes(ciphertext)
    pt = C.create_string_buffer(max(1, len(ciphertext)))
    rc = load_library().masp_host_chacha20poly1305_decrypt(_b(key), _b(nonce, 12), ciphertext, len(ciphertext), _b(tag, 16), pt)
    return pt.raw[:len(ciphertext)] if rc == 0 else None


def sapling_note_encrypt(esk, diversifier, pk_d, plaintext):
    """-> (epk, enc_ciphertext) of a 596-byte note plaintext under the given esk"""
    epk, enc = C.create_string_buffer(32), C.create_string_buffer(ENC_CIPHERTEXT_SIZE)
    _check(load_library().masp_host_sapling_note_encrypt(_b(esk), _b(diversifier, 11), _b(pk_d), _b(plaintext, NOTE_PLAINTEXT_SIZE), epk, enc))
    return epk.raw, enc.raw


def sapling_try_note_decryption(ivk, epk, cmu, enc_ciphertext, lead_byte=2):
    """-> (plaintext[596], pk_d[32]) or None"""
    pt, pk = C.create_string_buffer(NOTE_PLAINTEXT_SIZE), C.create_string_buffer(32)
    rc = load_library().masp_host_sapling_try_note_decryption(_b(ivk), _b(epk), _b(cmu), _b(enc_ciphertext, ENC_CIPHERTEXT_SIZE), lead_byte, pt, pk)
    if rc == E_NO_NOTE:
        return None
    _check(rc)
    return pt.raw, pk.raw


def sapling_finish_note_decryption(key, ivk, epk, cmu, enc_ciphertext, lead_byte=2):
    """the same from the symmetric key on -> (plaintext[596], pk_d[32]) or None"""
    pt, pk = C.create_string_buffer(NOTE_PLAINTEXT_SIZE), C.create_string_buffer(32)
    rc = load_library().masp_host_sapling_finish_note_decryption(_b(key), _b(ivk), _b(epk), _b(cmu), _b(enc_ciphertext, ENC_CIPHERTEXT_SIZE),
                                                                 lead_byte, pt, pk)
    if rc == E_NO_NOTE:
        return None
    _check(rc)
    return pt.raw, pk.raw


def sapling_try_note_decryption_batch(ivks, epks, cmus, enc_ciphertexts, lead_byte=2, threads=None):
    """batch::try_note_decryption on host threads: (hit_ivk int32[n_out] (-1: none), plaintexts uint8[n_out, 596], pk_ds uint8[n_out, 32])"""
    def arr(x, w):
        a = np.frombuffer(b"".join(bytes(i) for i in x), dtype=np.uint8) if isinstance(x, (list, tuple)) else np.ascontiguousarray(x, dtype=np.uint8)
        return a.reshape(-1, w)
    ivks, epks, cmus, encs = arr(ivks, 32), arr(epks, 32), arr(cmus, 32), arr(enc_ciphertexts, ENC_CIPHERTEXT_SIZE)
    n = epks.shape[0]
    assert cmus.shape[0] == n and encs.shape[0] == n
    hit = np.full(n, -1, np.int32)
    pts, pks = np.zeros((n, NOTE_PLAINTEXT_SIZE), np.uint8), np.zeros((n, 32), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load_library().masp_host_sapling_try_note_decryption_batch(ivks.shape[0], vp(ivks), n, vp(epks), vp(cmus), vp(encs), lead_byte,
                                                                       threads or effective_cpus(), vp(hit), vp(pts), vp(pks)))
    return hit, pts, pks


def sapling_try_compact_note_decryption(ivk, epk, cmu, enc_compact, lead_byte=2):
    """the compact (ZIP 307) form: enc_compact = the first 84 bytes of enc_ciphertext -> (plaintext[84], pk_d[32]) or None"""
    pt, pk = C.create_string_buffer(COMPACT_NOTE_SIZE), C.create_string_buffer(32)
    rc = load_library().masp_host_sapling_try_compact_note_decryption(_b(ivk), _b(epk), _b(cmu), _b(enc_compact, COMPACT_NOTE_SIZE), lead_byte, pt, pk)
    if rc == E_NO_NOTE:
        return None
    _check(rc)
    return pt.raw, pk.raw


def sapling_try_compact_note_decryption_batch(ivks, epks, cmus, enc_compacts, lead_byte=2, threads=None):
    """batch::try_compact_note_decryption on host threads: (hit_ivk int32[n_out] (-1: none), plaintexts uint8[n_out, 84], pk_ds uint8[n_out, 32],
    the number of pairs whose epk decodes and whose decrypted byte 0 is lead_byte)"""
    def arr(x, w):
        a = np.frombuffer(b"".join(bytes(i) for i in x), dtype=np.uint8) if isinstance(x, (list, tuple)) else np.ascontiguousarray(x, dtype=np.uint8)
        return a.reshape(-1, w)
    ivks, epks, cmus, encs = arr(ivks, 32), arr(epks, 32), arr(cmus, 32), arr(enc_compacts, COMPACT_NOTE_SIZE)
    n = epks.shape[0]
    assert cmus.shape[0] == n and encs.shape[0] == n
    hit = np.full(n, -1, np.int32)
    pts, pks = np.zeros((n, COMPACT_NOTE_SIZE), np.uint8), np.zeros((n, 32), np.uint8)
    cand = C.c_uint64(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load_library().masp_host_sapling_try_compact_note_decryption_batch(ivks.shape[0], vp(ivks), n, vp(epks), vp(cmus), vp(encs), lead_byte,
                                                                               threads or effective_cpus(), vp(hit), vp(pts), vp(pks),
                                                                               C.byref(cand)))
    return hit, pts, pks, cand.value


# ---- the sender's side: out_ciphertext and recovery with an outgoing viewing key ----
def prf_ock(ovk, cv, cmu, epk):
    """PRF^ock: BLAKE2b-256 personalised "MASP__Derive_ock" over ovk | cv | cmu | epk -> the 32-byte outgoing cipher key"""
    out = C.create_string_buffer(32)
    load_library().masp_host_prf_ock(_b(ovk), _b(cv), _b(cmu), _b(epk), out)
    return out.raw


def sapling_encrypt_outgoing(ock, pk_d, esk):
    """-> out_ciphertext[80] = AEAD(ock, pk_d | esk)"""
    out = C.create_string_buffer(OUT_CIPHERTEXT_SIZE)
    load_library().masp_host_sapling_encrypt_outgoing(_b(ock), _b(pk_d), _b(esk), out)
    return out.raw


def sapling_try_output_recovery_with_ock(ock, epk, cmu, enc_ciphertext, out_ciphertext, lead_byte=2):
    """try_sapling_output_recovery_with_ock -> (plaintext[596], pk_d[32]) or None"""
    pt, pk = C.create_string_buffer(NOTE_PLAINTEXT_SIZE), C.create_string_buffer(32)
    rc = load_library().masp_host_sapling_try_output_recovery_with_ock(_b(ock), _b(epk), _b(cmu), _b(enc_ciphertext, ENC_CIPHERTEXT_SIZE),
                                                                       _b(out_ciphertext, OUT_CIPHERTEXT_SIZE), lead_byte, pt, pk)
    if rc == E_NO_NOTE:
        return None
    _check(rc)
    return pt.raw, pk.raw


def sapling_try_output_recovery(ovk, cv, epk, cmu, enc_ciphertext, out_ciphertext, lead_byte=2):
    """try_sapling_output_recovery -> (plaintext[596], pk_d[32]) or None"""
    pt, pk = C.create_string_buffer(NOTE_PLAINTEXT_SIZE), C.create_string_buffer(32)
    rc = load_library().masp_host_sapling_try_output_recovery(_b(ovk), _b(cv), _b(epk), _b(cmu), _b(enc_ciphertext, ENC_CIPHERTEXT_SIZE),
                                                              _b(out_ciphertext, OUT_CIPHERTEXT_SIZE), lead_byte, pt, pk)
    if rc == E_NO_NOTE:
        return None
    _check(rc)
    return pt.raw, pk.raw


def sapling_try_output_recovery_batch(ovks, cvs, epks, cmus, enc_ciphertexts, out_ciphertexts, lead_byte=2, threads=None):
    """try_sapling_output_recovery over outputs x ovks on host threads: (hit_ovk int32[n_out] (-1: none), plaintexts uint8[n_out, 596],
    pk_ds uint8[n_out, 32])"""
    def arr(x, w):
        a = np.frombuffer(b"".join(bytes(i) for i in x), dtype=np.uint8) if isinstance(x, (list, tuple)) else np.ascontiguousarray(x, dtype=np.uint8)
        return a.reshape(-1, w)
    ovks, cvs, epks, cmus = arr(ovks, 32), arr(cvs, 32), arr(epks, 32), arr(cmus, 32)
    encs, couts = arr(enc_ciphertexts, ENC_CIPHERTEXT_SIZE), arr(out_ciphertexts, OUT_CIPHERTEXT_SIZE)
    n = epks.shape[0]
    assert cvs.shape[0] == n and cmus.shape[0] == n and encs.shape[0] == n and couts.shape[0] == n
    hit = np.full(n, -1, np.int32)
    pts, pks = np.zeros((n, NOTE_PLAINTEXT_SIZE), np.uint8), np.zeros((n, 32), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load_library().masp_host_sapling_try_output_recovery_batch(ovks.shape[0], vp(ovks), n, vp(cvs), vp(epks), vp(cmus), vp(encs), vp(couts),
                                                                       lead_byte, threads or effective_cpus(), vp(hit), vp(pts), vp(pks)))
    return hit, pts, pks
