"""ctypes binding of libmasp_hip.so (C ABI: include/masp_hip.h)."""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

ERRORS = {1: "invalid argument", 2: "Parameters bytes are malformed", 3: "Parameters do not match the circuit shape",
          4: "no usable HIP device (there is no CPU fallback)", 5: "HIP runtime error", 6: "UnexpectedIdentity",
          7: "circuit slot is empty", 8: "scalar is not a canonical field element", 9: "a Jubjub point encoding does not decode",
          10: "an output buffer is too small"}
E_POINT_ENCODING = 9
E_CAPACITY = 10
SPEND_AUTH, BINDING = 0, 1      # masp_hip_redjubjub_verify_batch kinds

SPEND, OUTPUT, CONVERT = 0, 1, 2


class MaspHipError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__("masp_hip error %d: %s%s" % (code, ERRORS.get(code, "?"), (" — " + detail) if detail else ""))


OPTION_FIELDS = ("slots", "batch_cap", "ntt_sub_batch", "window_bits_h", "window_bits_la", "window_bits_b", "window_bits_b2_lone",
                 "witness_nontrivial_percent", "bucket_tree_levels", "bucket_tree_sub_batch", "bucket_tree_levels_g2", "bucket_tree_scratch_mb", "lone_proof_graph", "window_bits_h_lone",
                 "window_bits_b2")


class OptionsStruct(C.Structure):
    """masp_hip_options (include/masp_hip.h): every field 0 = the default."""
    _fields_ = ([("struct_size", C.c_uint32)] + [(f, C.c_int32) for f in OPTION_FIELDS[:OPTION_FIELDS.index("lone_proof_graph")]] +
                [("bucket_tree_fallback_proofs", C.c_int32), ("lone_proof_graph", C.c_int32), ("hw_queues", C.c_int32), ("window_bits_h_lone", C.c_int32),
                 ("digit_recoding", C.c_int32),     # reserved since round 6 (was: NAF digits over per-bit tables), must be 0
                 ("window_bits_b2", C.c_int32)])


assert C.sizeof(OptionsStruct) == 76 and OptionsStruct.window_bits_b2.offset == 72        # include/masp_hip.h asserts the same


class JobStruct(C.Structure):
    _fields_ = [("circuit", C.c_uint32), ("inputs", C.c_void_p), ("aux", C.c_void_p), ("a", C.c_void_p),
                ("b", C.c_void_p), ("c", C.c_void_p), ("r", C.c_uint8 * 32), ("s", C.c_uint8 * 32), ("aux_form", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(JobStruct) == 120 and JobStruct.r.offset == 48 and JobStruct.aux_form.offset == 112   # include/masp_hip.h asserts the same
AUX_CANONICAL, AUX_MONTGOMERY = 0, 1     # masp_hip_job::aux_form
QUOTIENT_EVALUATION, QUOTIENT_COEFFICIENT = 0, 1     # masp_hip_ctx_set_quotient_form
QUOTIENT_FUSED, QUOTIENT_SEPARATE = 0, 1             # masp_hip_ctx_set_quotient_schedule


class BundleCheckStruct(C.Structure):
    """masp_hip_bundle_check (include/masp_hip.h): the arrays of one masp_hip_sapling_check_bundles call"""
    _fields_ = ([(f, C.c_size_t) for f in ("n_bundles", "n_spends", "n_converts", "n_outputs", "n_balance")] +
                [(f, C.c_void_p) for f in ("counts", "spend_cv", "spend_anchor", "spend_nullifier", "spend_rk", "spend_zkproof",
                                           "convert_cv", "convert_anchor", "convert_zkproof",
                                           "output_cv", "output_cmu", "output_epk", "output_zkproof", "balance_asset", "balance_value",
                                           "spend_status", "convert_status", "output_status", "spend_inputs", "convert_inputs", "output_inputs",
                                           "bvk", "bundle_status")])


assert C.sizeof(BundleCheckStruct) == 224 and BundleCheckStruct.counts.offset == 40 and BundleCheckStruct.bvk.offset == 208   # include/masp_hip.h asserts the same
BundleCheckResult = collections.namedtuple("BundleCheckResult", "spend_status convert_status output_status spend_inputs convert_inputs output_inputs "
                                                                "bvk bundle_status")


def bundle_check_args(counts, spends, converts, outputs, balance):
    """The struct of one check_bundles call over the caller's arrays -> (BundleCheckStruct, BundleCheckResult of zeroed numpy arrays the
    struct points into, the input arrays to keep alive).  Arguments as Context.check_bundles takes them."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 4)
    widths = ((32, 32, 32, 32, 192), (32, 32, 192), (32, 32, 32, 192), (32, 16))
    groups = [[_u8(a, w) for a, w in zip(g, ws)] for g, ws in zip((spends, converts, outputs, balance), widths)]
    assert all(len(g) == len(ws) for g, ws in zip(groups, widths))
    n = [g[0].shape[0] for g in groups]
    assert all(a.shape[0] == k for g, k in zip(groups, n) for a in g), "arrays of one kind differ in length"
    nb = counts.shape[0]
    res = BundleCheckResult(np.zeros(n[0], np.uint8), np.zeros(n[1], np.uint8), np.zeros(n[2], np.uint8), np.zeros((n[0], 7, 32), np.uint8),
                            np.zeros((n[1], 3, 32), np.uint8), np.zeros((n[2], 5, 32), np.uint8), np.zeros((nb, 32), np.uint8), np.zeros(nb, np.uint8))
    s = BundleCheckStruct()
    s.n_bundles, s.n_spends, s.n_converts, s.n_outputs, s.n_balance = nb, n[0], n[1], n[2], n[3]
    ptr = lambda a: a.ctypes.data if a.size else None       # noqa: E731  (an empty array goes as NULL: nothing of it is read)
    s.counts = ptr(counts)
    names = [f for f, _ in BundleCheckStruct._fields_[6:]]
    for name, a in zip(names, [a for g in groups for a in g] + list(res)):
        setattr(s, name, ptr(a))
    return s, res, (counts, groups)


def library_path():
    # MASP_HIP_LIBRARY: an alternative build of the same library (A/B measurements of compile-time parameters)
    return os.environ.get("MASP_HIP_LIBRARY") or os.path.join(_HERE, "libmasp_hip.so")


def load_library():
    """Loads the HIP extension; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("libmasp_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C masp_amd/csrc` (hipcc, --offload-arch=gfx950)")
    # batches in flight on different HIP streams only overlap if the runtime gives them their own hardware queues
    # (ROCm's default is 4); read once, when the HIP runtime initialises.  16: the slots' main streams and the context's own need a queue each; with 8
    # queues about one bench process in four landed in a mode 3 % slower (streams of two slots sharing a queue), with 16 none of
    # twelve did (profiles/r04e_hw_queues_and_the_two_modes.txt)
    # (the library's constructor does the same for a process that links it directly — masp_hip_runtime_prepare, include/masp_hip.h —;
    # here it is said before the load because an A/B run may load an older build.  What the runtime really uses is MEASURED per context:
    # Context.options["hw_queues"])
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    L = C.CDLL(path)
    if hasattr(L, "masp_hip_runtime_prepare"):
        L.masp_hip_runtime_prepare.argtypes = [C.c_int, C.c_int]
        # more than 20 hardware queues make a process SLOWER once its runtime has created them (the cap is what counts: the pool only
        # grows) — masp_hip_runtime_prepare(0, 0) changes nothing and returns what the environment says
        q = L.masp_hip_runtime_prepare(0, 0)
        if q > 20:
            import warnings
            warnings.warn("masp_amd: GPU_MAX_HW_QUEUES=%d: once this process holds more than 20 hardware queues every kernel dispatch gets "
                          "slower (24: -7 %%, 32: -21 %% proofs/s; profiles/r06_second_context_root_cause.txt) — use 16" % q)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    L.masp_hip_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.masp_hip_ctx_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.masp_hip_ctx_create_ex.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(OptionsStruct), C.POINTER(vp)]
    L.masp_hip_ctx_get_options.argtypes = [vp, C.POINTER(OptionsStruct)]
    L.masp_hip_device_count.argtypes = []
    L.masp_hip_options_default.argtypes = [C.POINTER(OptionsStruct)]
    L.masp_hip_options_default.restype = None
    L.masp_hip_ctx_device_count.argtypes = [vp]
    L.masp_hip_ctx_device_proofs.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(L, "masp_hip_ctx_stream_concurrency"):
        L.masp_hip_ctx_stream_concurrency.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "masp_hip_ctx_device_status"):            # (round 6; an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_ctx_device_status.argtypes = [vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint64)]
        L.masp_hip_ctx_inject_fault.argtypes = [vp, C.c_int, C.c_uint32]
    # (introspection added in round 4: an older build passed as MASP_HIP_LIBRARY for an A/B run lacks them; calling them then raises)
    if hasattr(L, "masp_hip_ctx_lone_graph_launches"):
        L.masp_hip_ctx_lone_graph_launches.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "masp_hip_circuit_flags"):
        L.masp_hip_circuit_flags.argtypes = [vp, u32, C.POINTER(C.c_uint32)]
    L.masp_hip_ctx_destroy.argtypes = [vp]
    L.masp_hip_ctx_destroy.restype = None
    L.masp_hip_strerror.restype = C.c_char_p
    L.masp_hip_last_error.argtypes = [vp]
    L.masp_hip_last_error.restype = C.c_char_p
    L.masp_hip_circuit_load.argtypes = [vp, u32, vp, sz, vp]
    L.masp_hip_prove.argtypes = [vp, u32, vp, vp, vp, vp, vp, C.c_char_p, C.c_char_p, vp]
    L.masp_hip_prove_batch.argtypes = [vp, sz, vp, vp]
    L.masp_hip_generate_parameters.argtypes = [vp, vp, C.c_char_p, vp, sz, C.POINTER(sz)]
    L.masp_hip_parameters_max_size.argtypes = [vp]
    L.masp_hip_parameters_max_size.restype = sz
    L.masp_hip_msm_g1.argtypes = [vp, vp, vp, sz, vp]
    L.masp_hip_msm_g2.argtypes = [vp, vp, vp, sz, vp]
    L.masp_hip_msm_g1_multi.argtypes = [vp, vp, sz, vp, sz, C.c_int, vp]
    L.masp_hip_msm_g2_multi.argtypes = [vp, vp, sz, vp, sz, C.c_int, vp]
    if hasattr(L, "masp_hip_msm_g1_multi_ex"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_msm_g1_multi_ex.argtypes = [vp, vp, sz, vp, sz, C.c_int, C.c_int, sz, sz, vp, vp]
        L.masp_hip_msm_g2_multi_ex.argtypes = [vp, vp, sz, vp, sz, C.c_int, C.c_int, sz, sz, vp, vp]
        L.masp_hip_ctx_set_boolean_block_bits.argtypes = [vp, C.c_int32]
        L.masp_hip_ctx_get_boolean_block_bits.argtypes = [vp, C.POINTER(C.c_int32)]
        L.masp_hip_ctx_set_window_row_multiples.argtypes = [vp, C.c_int32]
        L.masp_hip_ctx_get_window_row_multiples.argtypes = [vp, C.POINTER(C.c_int32)]
    if hasattr(L, "masp_hip_ctx_set_quotient_form"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_ctx_set_quotient_form.argtypes = [vp, C.c_int32]
        L.masp_hip_ctx_get_quotient_form.argtypes = [vp, C.POINTER(C.c_int32)]
        L.masp_hip_circuit_quotient_form.argtypes = [vp, u32, C.POINTER(C.c_int32)]
        L.masp_hip_circuit_window_row_multiples.argtypes = [vp, u32, C.POINTER(C.c_int32)]
        L.masp_hip_circuit_eval_bases.argtypes = [vp, u32, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    if hasattr(L, "masp_hip_ctx_set_quotient_schedule"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_ctx_set_quotient_schedule.argtypes = [vp, C.c_int32]
        L.masp_hip_ctx_get_quotient_schedule.argtypes = [vp, C.POINTER(C.c_int32)]
    if hasattr(L, "masp_hip_ctx_set_tree_entry_share"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_ctx_set_tree_entry_share.argtypes = [vp, C.c_int32]
        L.masp_hip_ctx_get_tree_entry_share.argtypes = [vp, C.POINTER(C.c_int32)]
        L.masp_hip_r1cs_boolean_variables.argtypes = [vp, vp]
        L.masp_hip_tree_entry_bound.argtypes = [u32, C.c_int32, u32, u32, C.c_int32]
        L.masp_hip_tree_entry_bound.restype = C.c_uint64
        L.masp_hip_circuit_tree_entry_bounds.argtypes = [vp, u32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.masp_hip_quotient_h.argtypes = [vp, vp, vp, vp, sz, u32, vp]
    L.masp_hip_ntt.argtypes = [vp, vp, u32, C.c_int]
    L.masp_hip_vk_prepare.argtypes = [vp, vp, sz, C.POINTER(vp)]
    L.masp_hip_vk_free.argtypes = [vp]
    L.masp_hip_vk_free.restype = None
    L.masp_hip_verify_batch.argtypes = [vp, vp, sz, vp, vp, u32, vp, C.POINTER(C.c_int)]
    if hasattr(L, "masp_hip_verify_each"):
        L.masp_hip_verify_each.argtypes = [vp, vp, sz, vp, vp, u32, C.c_char_p]
        L.masp_hip_verify_each_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
        L.masp_hip_redjubjub_verify_each.argtypes = [vp, sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    if hasattr(L, "masp_hip_redjubjub_verify_batch"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_jubjub_msm.argtypes = [vp, sz, vp, vp, vp, C.POINTER(C.c_int64)]
        L.masp_hip_redjubjub_verify_batch.argtypes = [vp, sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    if hasattr(L, "masp_hip_sapling_trial_decrypt"):
        L.masp_hip_sapling_trial_decrypt.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.POINTER(sz)]
        L.masp_hip_note_scan_configure.argtypes = [vp, C.c_int, C.c_int]
        L.masp_hip_note_scan_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_compact_trial_decrypt"):
        L.masp_hip_sapling_compact_trial_decrypt.argtypes = [vp, sz, vp, sz, vp, vp, vp, C.c_int, vp, sz, vp, vp, vp, vp, C.POINTER(sz), C.POINTER(sz)]
        L.masp_hip_note_scan_compact_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_output_recovery_scan"):
        L.masp_hip_sapling_output_recovery_scan.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, sz, vp, vp, vp, C.POINTER(sz)]
        L.masp_hip_out_recovery_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_merkle_tree_complete"):
        L.masp_hip_merkle_tree_complete.argtypes = [vp, C.c_uint, sz, vp, vp, sz, C.POINTER(sz), vp, sz, vp, vp, C.POINTER(C.c_int64)]
        L.masp_hip_merkle_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_merkle_tree_append"):
        L.masp_hip_merkle_tree_append.argtypes = [vp, C.c_uint64, vp, sz, vp, vp, sz, C.POINTER(sz), C.POINTER(C.c_int64)]
    if hasattr(L, "masp_hip_sapling_note_nullifiers"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_sapling_note_nullifiers.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.masp_hip_note_nullifiers_configure.argtypes = [vp, C.c_int]
        L.masp_hip_note_nullifiers_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_allowed_conversions"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_sapling_allowed_conversions.argtypes = [vp, sz, vp, sz, vp, vp, vp, vp, vp]
        L.masp_hip_allowed_conversions_configure.argtypes = [vp, C.c_int, sz, sz]
        L.masp_hip_allowed_conversions_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_build_outputs"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_sapling_build_outputs.argtypes = [vp, sz] + [vp] * 18
        L.masp_hip_build_outputs_configure.argtypes = [vp, sz]
        L.masp_hip_build_outputs_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_build_spends"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_redjubjub_sign_batch.argtypes = [vp, sz] + [vp] * 8
        L.masp_hip_redjubjub_sign_configure.argtypes = [vp, sz]
        L.masp_hip_redjubjub_sign_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
        L.masp_hip_sapling_build_spends.argtypes = [vp, sz] + [vp] * 17
        L.masp_hip_build_spends_configure.argtypes = [vp, sz]
        L.masp_hip_build_spends_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_sapling_check_bundles"):      # (an older build passed as MASP_HIP_LIBRARY lacks them)
        L.masp_hip_sapling_check_bundles.argtypes = [vp, C.POINTER(BundleCheckStruct)]
        L.masp_hip_check_bundles_last_timing.argtypes = [vp, C.POINTER(C.c_double)]
    L.masp_hip_batch_upload.argtypes = [vp, sz, vp]
    L.masp_hip_batch_prove_resident.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_float)]
    L.masp_hip_batch_prove_resident_steps.argtypes = [vp, C.c_int, sz, vp, vp, C.POINTER(C.c_float)]
    L.masp_hip_batch_free.argtypes = [vp, C.c_int]
    L.masp_hip_bench_msm.argtypes = [vp, C.c_int, sz, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(u32)]
    L.masp_hip_profile_enable.argtypes = [vp, C.c_int]
    L.masp_hip_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.masp_hip_profile_read_split.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "masp_hip_profile_read_lone"):
        L.masp_hip_profile_read_lone.argtypes = [vp, C.POINTER(C.c_double)]
    L.masp_hip_sync.argtypes = [vp]
    L.masp_hip_host_alloc.argtypes = [vp, sz]
    L.masp_hip_host_alloc.restype = vp
    L.masp_hip_host_free.argtypes = [vp, vp]
    L.masp_hip_host_free.restype = None
    _lib = L
    return L


def device_pci_bus_id(device=0):
    """masp_hip_device_pci_bus_id -> "0000:c1:00.0" (lower case), or None"""
    L = load_library()
    if not hasattr(L, "masp_hip_device_pci_bus_id"):
        return None
    buf = C.create_string_buffer(64)
    L.masp_hip_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    return buf.value.decode().lower() if L.masp_hip_device_pci_bus_id(int(device), buf, 64) == 0 else None


def device_count():
    """HIP devices visible to this process (masp_hip_device_count)."""
    return int(load_library().masp_hip_device_count())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8(a, shape_last=None):
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if shape_last is not None:
        a = a.reshape(-1, shape_last)
    return a


def _scalar32(x):
    if isinstance(x, int):
        return x.to_bytes(32, "little")
    b = bytes(x)
    assert len(b) == 32
    return b


class Context:
    """One GPU (`device` an int) or several GPUs of one node behind one prover (`device` a list of device indices:
    masp_hip_ctx_create_multi — prove_batch then deals its jobs to the devices).  Thread-safe: prove / prove_batch are
    re-entrant, everything else serialises inside the library."""

    def __init__(self, device=0, **options):
        """options: the fields of masp_hip_options (slots, batch_cap, ntt_sub_batch, window_bits_*, ...); unset = default.
        The library reads no environment variables: tuning comes through here."""
        self._L = load_library()
        h = C.c_void_p()
        unknown = set(options) - set(OPTION_FIELDS)
        if unknown:
            raise TypeError("unknown context option(s): %s" % ", ".join(sorted(unknown)))
        opt = OptionsStruct()
        self._L.masp_hip_options_default(C.byref(opt))
        for k, v in options.items():
            if v is not None:
                setattr(opt, k, int(v))
        if isinstance(device, (list, tuple)):
            arr = (C.c_int * len(device))(*[int(d) for d in device])
            if options or len(device) > 1:
                rc = self._L.masp_hip_ctx_create_ex(arr, len(device), C.byref(opt), C.byref(h))
            else:
                rc = self._L.masp_hip_ctx_create_multi(arr, len(device), C.byref(h))
        else:
            arr = (C.c_int * 1)(int(device))
            rc = self._L.masp_hip_ctx_create_ex(arr, 1, C.byref(opt), C.byref(h))
        if rc:
            raise MaspHipError(rc)
        got = OptionsStruct()
        got.struct_size = C.sizeof(OptionsStruct)           # the library writes no more than the caller's struct holds
        self._L.masp_hip_ctx_get_options(h, C.byref(got))
        self.options = {f: int(getattr(got, f)) for f in OPTION_FIELDS}      # defaults resolved
        # hardware queues the runtime spreads this process's streams over, measured at creation (masp_hip_options::hw_queues): fewer than
        # the slots have streams (five each) means independent kernels of a batch wait for each other — the HIP runtime was initialised
        # (by whatever this process loaded first) before GPU_MAX_HW_QUEUES said 16
        self.options["hw_queues"] = int(got.hw_queues)
        want = min(5 * self.options["slots"], 15)
        if 0 < self.options["hw_queues"] < want:
            import warnings
            warnings.warn("masp_amd: the HIP runtime gives this process %d hardware queue(s) for %d slots x 5 streams: set GPU_MAX_HW_QUEUES=16 "
                          "before the process's first HIP call (masp_hip_runtime_prepare)" % (self.options["hw_queues"], self.options["slots"]))

        self._h = h
        self._keep = []
        self._pinned = {}

    def close(self):
        if getattr(self, "_h", None):
            for p in list(getattr(self, "_pinned", {}).values()):
                self._L.masp_hip_host_free(self._h, p)
            self._pinned = {}
            self._L.masp_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise MaspHipError(rc, self._L.masp_hip_last_error(self._h).decode(errors="replace"))

    def _timing(self, fn, n, handle=None):
        """the n stage times in ms that fn(handle, ms) reports (handle: this context's unless given)"""
        ms = (C.c_double * n)()
        self._check(fn(self._h if handle is None else handle, ms))
        return tuple(ms)

    # ---- page-locked host buffers (assignments written here reach the device without a staging copy) ----
    def host_alloc(self, rows, cols=32):
        """-> np.uint8 array [rows, cols] over memory from masp_hip_host_alloc; release with host_free(array)."""
        p = self._L.masp_hip_host_alloc(self._h, rows * cols)
        if not p:
            raise MemoryError("masp_hip_host_alloc(%d bytes) failed" % (rows * cols))
        buf = (C.c_uint8 * (rows * cols)).from_address(p)
        a = np.frombuffer(buf, dtype=np.uint8).reshape(rows, cols)
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, a):
        p = self._pinned.pop(a.ctypes.data, None)
        if p and getattr(self, "_h", None):
            self._L.masp_hip_host_free(self._h, p)

    # ---- circuits / proofs ----
    def load_circuit(self, slot, params, cs):
        params = _u8(params)
        self._check(self._L.masp_hip_circuit_load(self._h, slot, _p(params), params.size, cs.ref))

    def _job(self, slot, inputs, aux, r, s, abc=None, aux_form=AUX_CANONICAL):
        j = JobStruct()
        j.circuit = slot
        j.aux_form = int(aux_form)
        inputs, aux = _u8(inputs, 32), _u8(aux, 32)
        keep = [inputs, aux]
        j.inputs, j.aux = inputs.ctypes.data, aux.ctypes.data
        if abc is not None:
            a, b, c = (_u8(x, 32) for x in abc)
            keep += [a, b, c]
            j.a, j.b, j.c = a.ctypes.data, b.ctypes.data, c.ctypes.data
        j.r[:] = _scalar32(r)
        j.s[:] = _scalar32(s)
        return j, keep

    def prove(self, slot, inputs, aux, r, s, abc=None):
        """-> 192-byte proof (A | B | C compressed)."""
        return self.prove_batch([(slot, inputs, aux, r, s, abc)])[0]

    def marshal_jobs(self, jobs):
        """jobs: iterable of (slot, inputs, aux, r, s[, (a,b,c)[, aux_form]]) -> (masp_hip_job array, n, keep-alive list): the argument
        of masp_hip_prove_batch, built once when the same list is proved repeatedly or timed."""
        jobs = list(jobs)
        arr = (JobStruct * len(jobs))()
        keep = []
        for i, job in enumerate(jobs):
            slot, inputs, aux, r, s = job[:5]
            abc = job[5] if len(job) > 5 else None
            arr[i], k = self._job(slot, inputs, aux, r, s, abc, job[6] if len(job) > 6 else AUX_CANONICAL)
            keep.append(k)
        return arr, len(jobs), keep

    def prove_marshalled(self, arr, n, out=None):
        """One masp_hip_prove_batch call -> u8[n,192]"""
        if out is None:
            out = np.zeros((n, 192), dtype=np.uint8)
        self._check(self._L.masp_hip_prove_batch(self._h, n, arr, _p(out)))
        return out

    def prove_batch(self, jobs):
        """jobs: iterable of (slot, inputs, aux, r, s[, (a,b,c)]) -> list of 192-byte proofs, job order."""
        arr, n, keep = self.marshal_jobs(jobs)
        out = self.prove_marshalled(arr, n)
        return [out[i].tobytes() for i in range(n)]

    def generate_parameters(self, cs, toxic):
        """toxic: (tau, alpha, beta, gamma, delta) ints -> Parameters bytes (bellman wire format), np.uint8."""
        t = b"".join(_scalar32(x) for x in toxic)
        cap = self._L.masp_hip_parameters_max_size(cs.ref)
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._check(self._L.masp_hip_generate_parameters(self._h, cs.ref, t, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    # ---- Groth16 batch verification on the GPU ----
    def prepare_verifying_key(self, params):
        """-> GpuVerifyingKey (= PreparedVerifyingKey, masp_proofs/src/lib.rs:391-393, for masp_hip_verify_batch)"""
        return GpuVerifyingKey(self, params)

    # ---- RedJubjub batch verification on the GPU ----
    def redjubjub_verify_batch(self, items, randomness=None):
        """items: (vk[32], sig[64] = Rbar || Sbar, sighash[32], kind) with kind SPEND_AUTH (basepoint spending_key_generator) or BINDING
        (value_commitment_randomness_generator) -> True iff every signature verifies (up to 2^-127): redjubjub::batch::Verifier::verify
        (masp_hip_redjubjub_verify_batch).  randomness: 16 bytes per item (default: from `secrets`)."""
        import secrets
        items = list(items)
        n = len(items)
        if n == 0:
            return True
        vks, sigs, sighashes = (b"".join(bytes(it[k]) for it in items) for k in range(3))
        if len(vks) != 32 * n or len(sigs) != 64 * n or len(sighashes) != 32 * n:
            return False
        kinds = bytes(int(it[3]) for it in items)
        z = randomness if randomness is not None else secrets.token_bytes(16 * n)
        assert len(z) == 16 * n
        ok = C.c_int(0)
        self._check(self._L.masp_hip_redjubjub_verify_batch(self._h, n, vks, sigs, sighashes, kinds, bytes(z), C.byref(ok)))
        return ok.value == 1

    def redjubjub_verify_each(self, items):
        """items as for redjubjub_verify_batch -> one bool per item: `redjubjub.verify` of each on its own (masp_hip_redjubjub_verify_each).
        An item whose vk, signature or sighash has the wrong length is False."""
        items = [tuple(it) for it in items]
        shaped = [len(bytes(it[0])) == 32 and len(bytes(it[1])) == 64 and len(bytes(it[2])) == 32 for it in items]
        sel = [it for it, ok in zip(items, shaped) if ok]
        n = len(sel)
        out = C.create_string_buffer(max(n, 1))
        if n:
            vks, sigs, sighashes = (b"".join(bytes(it[k]) for it in sel) for k in range(3))
            self._check(self._L.masp_hip_redjubjub_verify_each(self._h, n, vks, sigs, sighashes, bytes(int(it[3]) for it in sel), out))
        got = iter(out.raw[:n])
        return [next(got) == 1 if ok else False for ok in shaped]

    def jubjub_msm(self, points, scalars):
        """sum_i [scalars_i] points_i over Jubjub (masp_hip_jubjub_msm): points = 32-byte encodings, scalars = ints below 2^256 or 32-byte
        little-endian values -> the 32-byte encoding of the sum.  A point that does not decode raises MaspHipError (code 9) with
        `.bad_index` set to the first such index."""
        n = len(points)
        assert len(scalars) == n
        pts = np.frombuffer(b"".join(bytes(p) for p in points), dtype=np.uint8)
        sc = np.frombuffer(b"".join(_scalar32(s) for s in scalars), dtype=np.uint8)
        assert pts.size == 32 * n and sc.size == 32 * n
        out = np.zeros(32, dtype=np.uint8)
        bad = C.c_int64(-1)
        rc = self._L.masp_hip_jubjub_msm(self._h, n, _p(pts), _p(sc), _p(out), C.byref(bad))
        if rc == E_POINT_ENCODING:
            e = MaspHipError(rc, "point %d" % bad.value)
            e.bad_index = bad.value
            raise e
        self._check(rc)
        return out.tobytes()

    # ---- the consensus pre-checks of a block's bundles on the GPU ----
    def check_bundles(self, counts, spends, converts, outputs, balance):
        """What BatchValidator.check_bundle decides per description, with the public inputs and binding verification keys, for all bundles
        of a block in one call (masp_hip_sapling_check_bundles).  counts: uint32[n_bundles, 4], the spends, converts, outputs and
        value-balance entries of each bundle; the items of a kind lie bundle after bundle in their arrays: spends = (cv, anchor, nullifier,
        rk, zkproof), converts = (cv, anchor, zkproof), outputs = (cv, cmu, epk, zkproof), balance = (asset identifiers, values as 16-byte
        little-endian two's-complement i128); 32 bytes an item but zkproof (192) and the values.  -> BundleCheckResult of numpy arrays:
          spend_status, convert_status, output_status   uint8[n]: 0, or the first that applies of 1 cv does not decode, 2 rk / epk does not
                                                        decode, 3 `Proof::read` refuses the proof, 4 cv has small order, 5 rk / epk has;
          spend_inputs [n, 7, 32], convert_inputs [n, 3, 32], output_inputs [n, 5, 32]   the public inputs as canonical little-endian
                                                        scalars (zeros where the status is not 0);
          bvk [n_bundles, 32], bundle_status [n_bundles]   0 bvk is valid, 1 a description has a status, 2 a value is i128::MIN, 3 an
                                                        identifier has no generator (bvk zeros for 1 - 3).
        Counts that do not add up to the arrays' lengths raise MaspHipError (invalid argument)."""
        s, res, keep = bundle_check_args(counts, spends, converts, outputs, balance)
        self._check(self._L.masp_hip_sapling_check_bundles(self._h, C.byref(s)))
        return res

    def check_bundles_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last check_bundles call of this context, from HIP events on its stream"""
        return self._timing(self._L.masp_hip_check_bundles_last_timing, 3)

    # ---- batch trial decryption of Sapling notes on the GPU ----
    def _scan_with_room(self, fn, args, widths, n_out, hit_capacity, tail=()):
        """One output scan fn(ctx, *args, capacity, hit_output, hit_key, <an array of uint8[w] rows per w of widths>, &n_hits, *tail) with
        room for its hits: too little of it (E_CAPACITY) raises MaspHipError with `.needed` if hit_capacity was given, else the call is
        repeated with the room it asked for.  -> the hit arrays, cut to the hits."""
        cap = max(16, n_out // 64) if hit_capacity is None else int(hit_capacity)
        while True:
            hits = [np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)] + [np.zeros((cap, w), np.uint8) for w in widths]
            nh = C.c_size_t(0)
            rc = fn(self._h, *args, cap, *[_p(h) for h in hits], C.byref(nh), *tail)
            if rc == E_CAPACITY and hit_capacity is None:
                cap = nh.value
                continue
            if rc == E_CAPACITY:
                e = MaspHipError(rc, "%d hits" % nh.value)
                e.needed = nh.value
                raise e
            self._check(rc)
            return [h[:nh.value] for h in hits]

    def sapling_trial_decrypt(self, ivks, epks, enc_ciphertexts, hit_capacity=None):
        """The device half of batch::try_note_decryption (masp_hip_sapling_trial_decrypt): ivks n_ivk x 32, epks n_out x 32, enc_ciphertexts
        n_out x 612 (bytes or uint8 arrays) -> (epk_status uint8[n_out], hit_output uint32[h], hit_ivk uint32[h], hit_keys uint8[h, 32]): the
        pairs whose tag verifies, sorted by (output, ivk), each with its symmetric key.  hit_capacity: room for that many hits (default: grown
        to what the call asks for)."""
        ivks, epks, encs = _u8(ivks, 32), _u8(epks, 32), _u8(enc_ciphertexts, 612)
        n_ivk, n_out = ivks.shape[0], epks.shape[0]
        assert encs.shape[0] == n_out
        status = np.zeros(n_out, dtype=np.uint8)
        ho, hi, hk = self._scan_with_room(self._L.masp_hip_sapling_trial_decrypt, (n_ivk, _p(ivks), n_out, _p(epks), _p(encs), _p(status)), (32,),
                                          n_out, hit_capacity)
        return status, ho, hi, hk

    def note_scan_configure(self, signed_digits=1, inversion=0):
        """measurement knobs of the note scan (masp_hip_note_scan_configure); results do not depend on them"""
        self._check(self._L.masp_hip_note_scan_configure(self._h, int(signed_digits), int(inversion)))

    def note_scan_last_timing(self):
        """(upload ms, kernel ms) of the last scan, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_note_scan_last_timing, 2)

    def sapling_compact_trial_decrypt(self, ivks, epks, cmus, enc_compact, lead_byte=2, hit_capacity=None, count_candidates=True):
        """batch::try_compact_note_decryption on the GPU, all of it (masp_hip_sapling_compact_trial_decrypt): ivks n_ivk x 32, epks and cmus
        n_out x 32, enc_compact n_out x 84 (bytes or uint8 arrays) -> (epk_status uint8[n_out], hit_output uint32[h], hit_ivk uint32[h],
        hit_plaintexts uint8[h, 84], hit_pk_d uint8[h, 32], n_candidates): the pairs for which the whole check succeeds, sorted by
        (output, ivk); n_candidates: the pairs that passed the lead-byte test (None with count_candidates=False: a NULL pointer)."""
        ivks, epks, cmus, encs = _u8(ivks, 32), _u8(epks, 32), _u8(cmus, 32), _u8(enc_compact, 84)
        n_ivk, n_out = ivks.shape[0], epks.shape[0]
        assert encs.shape[0] == n_out and cmus.shape[0] == n_out
        status = np.zeros(n_out, dtype=np.uint8)
        nc = C.c_size_t(0)
        ho, hi, hp, hk = self._scan_with_room(self._L.masp_hip_sapling_compact_trial_decrypt,
                                              (n_ivk, _p(ivks), n_out, _p(epks), _p(cmus), _p(encs), int(lead_byte), _p(status)), (84, 32), n_out,
                                              hit_capacity, tail=(C.byref(nc) if count_candidates else None,))
        return status, ho, hi, hp, hk, (nc.value if count_candidates else None)

    def note_scan_compact_last_timing(self):
        """(upload ms, stage 1 ms, stage 2 ms) of the last compact scan, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_note_scan_compact_last_timing, 3)

    # ---- batch output recovery with outgoing viewing keys on the GPU ----
    def sapling_output_recovery_scan(self, ovks, cvs, epks, cmus, c_outs, hit_capacity=None):
        """The device half of try_sapling_output_recovery over outputs x ovks (masp_hip_sapling_output_recovery_scan): ovks n_ovk x 32, cvs,
        epks and cmus n_out x 32, c_outs n_out x 80 (bytes or uint8 arrays) -> (hit_output uint32[h], hit_ovk uint32[h], hit_ocks uint8[h, 32]):
        the pairs whose out_ciphertext tag verifies, sorted by (output, ovk), each with its ock.  hit_capacity: room for that many hits
        (default: grown to what the call asks for)."""
        ovks, cvs, epks, cmus, couts = _u8(ovks, 32), _u8(cvs, 32), _u8(epks, 32), _u8(cmus, 32), _u8(c_outs, 80)
        n_ovk, n_out = ovks.shape[0], epks.shape[0]
        assert cvs.shape[0] == n_out and cmus.shape[0] == n_out and couts.shape[0] == n_out
        return tuple(self._scan_with_room(self._L.masp_hip_sapling_output_recovery_scan,
                                          (n_ovk, _p(ovks), n_out, _p(cvs), _p(epks), _p(cmus), _p(couts)), (32,), n_out, hit_capacity))

    def out_recovery_last_timing(self):
        """(upload ms, kernel ms) of the last output recovery scan, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_out_recovery_last_timing, 2)

    # ---- frozen commitment trees on the GPU ----
    def merkle_tree_complete(self, row, height0=0, positions=(), want_nodes=True, nodes_capacity=None):
        """FrozenCommitmentTree::complete, root and paths on the GPU (masp_hip_merkle_tree_complete): row n x 32 (bytes or a uint8 array), the
        nodes of level height0; positions: indices into the row -> (nodes uint8[N, 32] or None with want_nodes=False: no download of the
        vector, root bytes, paths uint8[len(positions), 32 - height0, 32] siblings lowest level first).  A node that is not canonical raises
        MaspHipError with .bad_index; nodes_capacity: room for that many nodes (default: what the vector needs), too little raises with
        .needed."""
        row = _u8(row, 32)
        pos = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1)
        n, depth = row.shape[0], max(0, 32 - int(height0))
        paths = np.zeros((pos.shape[0], depth, 32), np.uint8)
        root = np.zeros(32, np.uint8)
        nn, bad = C.c_size_t(0), C.c_int64(-1)
        if want_nodes and nodes_capacity is None:
            from .host import merkle_node_count
            nodes_capacity = merkle_node_count(n, int(height0))
        nodes = np.zeros((int(nodes_capacity), 32), np.uint8) if want_nodes else None
        rc = self._L.masp_hip_merkle_tree_complete(self._h, int(height0), n, _p(row) if n else None, _p(nodes), int(nodes_capacity or 0),
                                                   C.byref(nn), _p(root), pos.shape[0], _p(pos) if pos.shape[0] else None, _p(paths),
                                                   C.byref(bad))
        if rc:
            detail = "node %d is not canonical" % bad.value if bad.value >= 0 else \
                "%d nodes" % nn.value if rc == E_CAPACITY else self._L.masp_hip_last_error(self._h).decode(errors="replace")
            e = MaspHipError(rc, detail)
            e.bad_index, e.needed = bad.value, nn.value
            raise e
        return (nodes[:nn.value] if want_nodes else None), root.tobytes(), paths

    def merkle_tree_append(self, start, frontier, row, nodes_capacity=None):
        """A block of leaves at an arbitrary offset on the GPU (masp_hip_merkle_tree_append): row n x 32 (bytes or a uint8 array), the leaves
        at positions start .. start + n - 1 of the depth-32 tree; frontier 32 x 32 (or None with start = 0), entry h the node
        (h, (start >> h) - 1), read where bit h of start is set -> uint8[N, 32]: for h = 1..32 in turn the nodes (h, i) with
        start >> h <= i < (start + n) >> h.  A node that is not canonical raises MaspHipError with .bad_index (the row's index, or -2 - h
        for frontier entry h); nodes_capacity: room for that many nodes (default: what the call needs), too little raises with .needed."""
        from .host import merkle_append_args, merkle_append_error, merkle_append_node_count
        row, frontier = merkle_append_args(start, frontier, row)
        n = row.shape[0]
        if nodes_capacity is None:
            nodes_capacity = merkle_append_node_count(int(start), n)
        nodes = np.zeros((max(1, int(nodes_capacity)), 32), np.uint8)
        nn, bad = C.c_size_t(0), C.c_int64(-1)
        rc = self._L.masp_hip_merkle_tree_append(self._h, int(start), _p(frontier), n, _p(row) if n else None, _p(nodes), int(nodes_capacity),
                                                 C.byref(nn), C.byref(bad))
        if rc:
            detail = merkle_append_error("merkle_tree_append", bad.value) if bad.value != -1 else \
                "%d nodes" % nn.value if rc == E_CAPACITY else self._L.masp_hip_last_error(self._h).decode(errors="replace")
            e = MaspHipError(rc, detail)
            e.bad_index, e.needed = bad.value, nn.value
            raise e
        return nodes[:nn.value]

    def merkle_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last tree of this context, from HIP events on its stream"""
        return self._timing(self._L.masp_hip_merkle_last_timing, 3)

    # ---- nullifiers and note commitments of a wallet's notes on the GPU ----
    def note_nullifiers(self, asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, nks, positions, want_cmus=True):
        """Note::cmu and Note::nf(&nk, position) for n notes on the GPU (masp_hip_sapling_note_nullifiers): arrays in (n x 32 bytes each,
        diversifiers n x 11, values / positions / lead bytes n) -> (status uint8[n], cmus uint8[n, 32] or None with want_cmus=False: not
        downloaded, nfs uint8[n, 32]).  status: 0, or 1 asset identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 nk; such a note's
        outputs are zeros.  host.note_nullifiers is the same on the host."""
        from .host import note_nullifier_args
        args = note_nullifier_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, nks, positions)
        n = args[0].shape[0]
        status, nfs = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        cmus = np.zeros((n, 32), np.uint8) if want_cmus else None
        p = [_p(a) if n else None for a in args]
        self._check(self._L.masp_hip_sapling_note_nullifiers(self._h, n, *p, _p(status) if n else None, _p(cmus) if n else None,
                                                             _p(nfs) if n else None))
        return status, cmus, nfs

    def note_nullifiers_configure(self, lanes_per_note=0):
        """how many lanes add a note's table points: 1 or 8; 0 = by the number of notes (the default).  The bytes do not depend on it."""
        self._check(self._L.masp_hip_note_nullifiers_configure(self._h, int(lanes_per_note)))

    def note_nullifiers_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last note_nullifiers call of this context, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_note_nullifiers_last_timing, 3)

    # ---- a conversion tree's leaves on the GPU ----
    def allowed_conversions(self, term_offsets, identifiers, values, want_generators=True):
        """AllowedConversion::from and ::cmu for n_conv conversions on the GPU (masp_hip_sapling_allowed_conversions): conversion c owns the
        terms term_offsets[c] .. term_offsets[c + 1] - 1 of identifiers (n_terms x 32) and values (n_terms x 16 bytes, little-endian i128, or
        Python integers), summed as given -> (status uint8[n_conv], generators uint8[n_conv, 32] or None with want_generators=False: not
        downloaded, cmus uint8[n_conv, 32]).  status: 0, or 1 an identifier without a generator, else 2 a value that is i128::MIN; such a
        conversion's outputs are zeros.  host.allowed_conversions is the same on the host."""
        from .host import allowed_conversion_args
        off, ids, vals = allowed_conversion_args(term_offsets, identifiers, values)
        n = max(off.shape[0] - 1, 0)
        status, cmus = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
        gens = np.zeros((n, 32), np.uint8) if want_generators else None
        p = lambda a: _p(a) if a is not None and a.size else None
        self._check(self._L.masp_hip_sapling_allowed_conversions(self._h, n, p(off), ids.shape[0], p(ids), p(vals), p(status), p(gens), p(cmus)))
        return status, gens, cmus

    def allowed_conversions_configure(self, lanes_per_conversion=0, chunk_conversions=0, chunk_terms=0):
        """how many lanes add a conversion's points (1 or 8; 0 = by the number of conversions) and a chunk's limits (0 = the defaults,
        nothing above them).  For measurements and tests: the bytes do not depend on it."""
        self._check(self._L.masp_hip_allowed_conversions_configure(self._h, int(lanes_per_conversion), int(chunk_conversions), int(chunk_terms)))

    def allowed_conversions_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last allowed_conversions call of this context, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_allowed_conversions_last_timing, 3)

    # ---- output descriptions without their proofs on the GPU ----
    def build_outputs(self, asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, esks, rcvs, memos, ovks, ovk_flags=None,
                      out_randoms=None):
        """cv, cmu, epk, enc_ciphertext and out_ciphertext of n outputs on the GPU (masp_hip_sapling_build_outputs).  Arrays in, in the C
        ABI's order (n x 32 bytes each, diversifiers n x 11, values / lead bytes / ovk flags n, memos n x 512, out_randoms n x 96); esks (no
        lead byte is 1), memos (every memo empty, nothing uploaded), ovk_flags (every ovk present) and out_randoms (no flag is 0) may be None
        -> (status uint8[n], cvs, cmus, epks uint8[n, 32], encs uint8[n, 612], couts uint8[n, 80]).  status: 0, or 1 asset identifier,
        2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 esk, 6 rcv; such an output's outputs are zeros.  No randomness is drawn.
        host.build_outputs is the same on the host."""
        from .host import build_output_args, build_output_results
        args = build_output_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, esks, rcvs, memos, ovks, ovk_flags, out_randoms)
        n = args[0].shape[0]
        res = build_output_results(n)
        p = lambda a: _p(a) if a is not None and a.size else None
        self._check(self._L.masp_hip_sapling_build_outputs(self._h, n, *[p(a) for a in args], *[p(a) for a in res]))
        return res

    def build_outputs_configure(self, chunk_outputs=0):
        """outputs per chunk: 0 = the default, nothing above it.  For measurements and tests: the bytes do not depend on it."""
        self._check(self._L.masp_hip_build_outputs_configure(self._h, int(chunk_outputs)))

    def build_outputs_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last build_outputs call of this context, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_build_outputs_last_timing, 3)

    # ---- spend descriptions without their proofs, and RedJubjub signatures, on the GPU ----
    def redjubjub_sign_batch(self, sks, alphas, sighashes, kinds, randoms, want_vks=True):
        """n RedJubjub signatures on the GPU (masp_hip_redjubjub_sign_batch): rsk = sk + alpha, vk = [rsk] G_kind, sig = Rbar | S with the
        nonce from the item's 80 bytes of randoms.  sks, alphas (or None: no randomisation), sighashes n x 32, kinds n (0 spend
        authorisation, 1 binding), randoms n x 80 -> (status uint8[n], vks uint8[n, 32] or None with want_vks=False: not downloaded, sigs
        uint8[n, 64]).  status: 0, or 1 sk >= r_J, 2 alpha >= r_J; such an item's outputs are zeros.  No randomness is drawn; what the call
        uploaded and kept of the secrets is zeroed before it returns.  host.redjubjub_sign_batch is the same on the host."""
        from .host import sign_batch_args
        args = sign_batch_args(sks, alphas, sighashes, kinds, randoms)
        n = args[0].shape[0]
        status, sigs = np.zeros(n, np.uint8), np.zeros((n, 64), np.uint8)
        vks = np.zeros((n, 32), np.uint8) if want_vks else None
        p = lambda a: _p(a) if a is not None and a.size else None
        self._check(self._L.masp_hip_redjubjub_sign_batch(self._h, n, *[p(a) for a in args], p(status), p(vks), p(sigs)))
        return status, vks, sigs

    def redjubjub_sign_configure(self, chunk_items=0):
        """items per chunk: 0 = the default, nothing above it.  For measurements and tests: the bytes do not depend on it."""
        self._check(self._L.masp_hip_redjubjub_sign_configure(self._h, int(chunk_items)))

    def redjubjub_sign_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last redjubjub_sign_batch call of this context, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_redjubjub_sign_last_timing, 3)

    def build_spends(self, asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, positions,
                     want_cmus=True, want_nks=True):
        """cv, rk, nf, cmu and nk of n spends on the GPU (masp_hip_sapling_build_spends).  Arrays in, in the C ABI's order (n x 32 bytes each,
        diversifiers n x 11, values / lead bytes / positions n) -> (status uint8[n], cvs, rks, nfs uint8[n, 32], cmus, nks uint8[n, 32] or
        None where not wanted: not downloaded).  status: 0, or 1 asset identifier, 2 diversifier, 3 pk_d, 4 lead byte or rcm, 5 ak does not
        decode, 6 ak of small order, 7 nsk, 8 ar, 9 rcv; such a spend's outputs are zeros.  No randomness is drawn.  host.build_spends is
        the same on the host."""
        from .host import build_spend_args, build_spend_results
        args = build_spend_args(asset_identifiers, values, diversifiers, pk_ds, lead_bytes, rseeds, aks, nsks, ars, rcvs, positions)
        n = args[0].shape[0]
        res = build_spend_results(n, want_cmus, want_nks)
        p = lambda a: _p(a) if a is not None and a.size else None
        self._check(self._L.masp_hip_sapling_build_spends(self._h, n, *[p(a) for a in args], *[p(a) for a in res]))
        return res

    def build_spends_configure(self, chunk_spends=0):
        """spends per chunk: 0 = the default, nothing above it.  For measurements and tests: the bytes do not depend on it."""
        self._check(self._L.masp_hip_build_spends_configure(self._h, int(chunk_spends)))

    def build_spends_last_timing(self):
        """(upload ms, kernel ms, download ms) of the last build_spends call of this context, HIP events summed over its chunks"""
        return self._timing(self._L.masp_hip_build_spends_last_timing, 3)

    # ---- building blocks ----
    def msm_g1(self, bases, scalars):
        bases, scalars = _u8(bases, 96), _u8(scalars, 32)
        out = np.zeros(96, dtype=np.uint8)
        self._check(self._L.masp_hip_msm_g1(self._h, _p(bases), _p(scalars), scalars.shape[0], _p(out)))
        return out.tobytes()

    def msm_g2(self, bases, scalars):
        bases, scalars = _u8(bases, 192), _u8(scalars, 32)
        out = np.zeros(192, dtype=np.uint8)
        self._check(self._L.masp_hip_msm_g2(self._h, _p(bases), _p(scalars), scalars.shape[0], _p(out)))
        return out.tobytes()

    def msm_g1_multi(self, bases, scalars, window_bits=0):
        """bases u8[n,96]; scalars u8[np,n,32] -> list of np 96-byte results (one batched launch sequence)."""
        bases = _u8(bases, 96)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8)
        npf, n = scalars.shape[0], scalars.shape[1]
        assert scalars.shape == (npf, n, 32) and bases.shape[0] == n
        out = np.zeros((npf, 96), dtype=np.uint8)
        self._check(self._L.masp_hip_msm_g1_multi(self._h, _p(bases), n, _p(scalars), npf, int(window_bits), _p(out)))
        return [out[i].tobytes() for i in range(npf)]

    def msm_g2_multi(self, bases, scalars, window_bits=0):
        """bases u8[n,192]; scalars u8[np,n,32] -> list of np 192-byte results (one batched launch sequence)."""
        bases = _u8(bases, 192)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8)
        npf, n = scalars.shape[0], scalars.shape[1]
        assert scalars.shape == (npf, n, 32) and bases.shape[0] == n
        out = np.zeros((npf, 192), dtype=np.uint8)
        self._check(self._L.masp_hip_msm_g2_multi(self._h, _p(bases), n, _p(scalars), npf, int(window_bits), _p(out)))
        return [out[i].tobytes() for i in range(npf)]

    def _msm_multi_ex(self, fn, size, bases, scalars, window_bits, block_bits, sub_lo, sub_hi):
        bases = _u8(bases, size)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint8)
        npf, n = scalars.shape[0], scalars.shape[1]
        assert scalars.shape == (npf, n, 32) and bases.shape[0] == n
        out = np.zeros((npf, size), dtype=np.uint8)
        cnt = np.zeros(npf, dtype=np.uint32)
        self._check(fn(self._h, _p(bases), n, _p(scalars), npf, int(window_bits), int(block_bits), int(sub_lo), int(n if sub_hi is None else sub_hi),
                       _p(out), _p(cnt)))
        return [out[i].tobytes() for i in range(npf)], [int(c) for c in cnt]

    def msm_g1_multi_ex(self, bases, scalars, window_bits=0, block_bits=0, sub_lo=0, sub_hi=None):
        """msm_g1_multi with subset rows over the aligned blocks of 2^block_bits bases (0: none, 2, 3) inside [sub_lo, sub_hi) ->
        (results, entries of every proof's bucket 0 after the sort)."""
        return self._msm_multi_ex(self._L.masp_hip_msm_g1_multi_ex, 96, bases, scalars, window_bits, block_bits, sub_lo, sub_hi)

    def msm_g2_multi_ex(self, bases, scalars, window_bits=0, block_bits=0, sub_lo=0, sub_hi=None):
        """the same over G2"""
        return self._msm_multi_ex(self._L.masp_hip_msm_g2_multi_ex, 192, bases, scalars, window_bits, block_bits, sub_lo, sub_hi)

    def set_boolean_block_bits(self, bits):
        """Block width (log2) of the subset rows behind the tables of circuits loaded FROM NOW ON: 0 = the build's default, -1 = off, 2 or 3."""
        self._check(self._L.masp_hip_ctx_set_boolean_block_bits(self._h, int(bits)))

    @property
    def boolean_block_bits(self):
        """the resolved value: 0 = no subset rows, 2 or 3"""
        v = C.c_int32(0)
        self._check(self._L.masp_hip_ctx_get_boolean_block_bits(self._h, C.byref(v)))
        return int(v.value)

    def set_window_row_multiples(self, v):
        """Doubled window rows behind the batch tables of circuits loaded FROM NOW ON (two thirds as many buckets per MSM): 0 = the build's
        default, -1 = off, 1 = every table that batches use, 2 = the merged h + l tables only."""
        self._check(self._L.masp_hip_ctx_set_window_row_multiples(self._h, int(v)))

    @property
    def window_row_multiples(self):
        """the resolved value as a mask: bit 0 = the merged h + l tables, bit 1 = a, b_g1, b_g2"""
        v = C.c_int32(0)
        self._check(self._L.masp_hip_ctx_get_window_row_multiples(self._h, C.byref(v)))
        return int(v.value)

    def set_quotient_form(self, form):
        """How the batches of circuits loaded FROM NOW ON compute their quotient: QUOTIENT_EVALUATION (0, the default: four transforms per
        proof over bases derived when the circuit is loaded) or QUOTIENT_COEFFICIENT (1: six transforms over the h and l queries)."""
        self._check(self._L.masp_hip_ctx_set_quotient_form(self._h, int(form)))

    @property
    def quotient_form(self):
        v = C.c_int32(0)
        self._check(self._L.masp_hip_ctx_get_quotient_form(self._h, C.byref(v)))
        return int(v.value)

    def set_quotient_schedule(self, schedule):
        """How a batch in evaluation form runs its transforms FROM THE NEXT BATCH ON: QUOTIENT_FUSED (0, the default: three kernels per
        sub-batch, no permutation pass) or QUOTIENT_SEPARATE (1: seven launches, a bit-reversal pass in front of every transform)."""
        self._check(self._L.masp_hip_ctx_set_quotient_schedule(self._h, int(schedule)))

    @property
    def quotient_schedule(self):
        v = C.c_int32(0)
        self._check(self._L.masp_hip_ctx_get_quotient_schedule(self._h, C.byref(v)))
        return int(v.value)

    def circuit_quotient_form(self, slot):
        """the form the batches of the circuit in `slot` really use (coefficient form also where a derived base came out at infinity)"""
        v = C.c_int32(0)
        self._check(self._L.masp_hip_circuit_quotient_form(self._h, int(slot), C.byref(v)))
        return int(v.value)

    def circuit_window_row_multiples(self, slot):
        """the tables of the circuit in `slot` that really have doubled window rows: bit 0 h + l, bit 1 the evaluation form's merged table,
        bit 2 a, bit 3 b_g1, bit 4 b_g2 (a table with a point at infinity stays plain)"""
        v = C.c_int32(0)
        self._check(self._L.masp_hip_circuit_window_row_multiples(self._h, int(slot), C.byref(v)))
        return int(v.value)

    def circuit_eval_bases(self, slot):
        """masp_hip_circuit_eval_bases -> (u8[n, 96] uncompressed points: T' (m), L' (n_aux), one per used input; the used input columns)"""
        n, k = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.masp_hip_circuit_eval_bases(self._h, int(slot), None, 0, C.byref(n), None, 0, C.byref(k)))
        pts = np.zeros((n.value, 96), dtype=np.uint8)
        cols = np.zeros(max(k.value, 1), dtype=np.uint32)
        if n.value:
            self._check(self._L.masp_hip_circuit_eval_bases(self._h, int(slot), _p(pts), n.value, C.byref(n), _p(cols), cols.size, C.byref(k)))
        return pts, [int(c) for c in cols[:k.value]]

    def set_tree_entry_share(self, percent):
        """Of the witness scalars that the R1CS does not prove boolean, the share (1..100, 0 = the default) that the scratch of the bucket
        tree takes to be full width, for circuits loaded FROM NOW ON; a proof with more entries goes through the XYZZ accumulation."""
        self._check(self._L.masp_hip_ctx_set_tree_entry_share(self._h, int(percent)))

    @property
    def tree_entry_share(self):
        v = C.c_int32(0)
        self._check(self._L.masp_hip_ctx_get_tree_entry_share(self._h, C.byref(v)))
        return int(v.value)

    def circuit_tree_entry_bounds(self, slot):
        """-> {"hl" | "a" | "b_g1" | "b_g2": (entry bound of the batch MSM, its window width)} of the circuit in `slot`"""
        b, c = (C.c_uint64 * 4)(), (C.c_int32 * 4)()
        self._check(self._L.masp_hip_circuit_tree_entry_bounds(self._h, int(slot), b, c))
        return {k: (int(b[i]), int(c[i])) for i, k in enumerate(("hl", "a", "b_g1", "b_g2"))}

    def current_options(self):
        """masp_hip_ctx_get_options now: the options with what lack of tree scratch has changed since creation — the
        `bucket_tree_sub_batch` in use and `bucket_tree_fallback_proofs` (proofs that went through the XYZZ accumulation)."""
        got = OptionsStruct()
        got.struct_size = C.sizeof(OptionsStruct)
        self._check(self._L.masp_hip_ctx_get_options(self._h, C.byref(got)))
        d = {f: int(getattr(got, f)) for f in OPTION_FIELDS}
        d["bucket_tree_fallback_proofs"] = int(got.bucket_tree_fallback_proofs)
        d["hw_queues"] = int(got.hw_queues)
        return d

    @property
    def device_count(self):
        return self._L.masp_hip_ctx_device_count(self._h)

    def circuit_uses_endomorphism(self, slot):
        """masp_hip_circuit_flags bit 0: every CRS point behind A and B1 is in the prime-order subgroup"""
        f = C.c_uint32(0)
        self._check(self._L.masp_hip_circuit_flags(self._h, int(slot), C.byref(f)))
        return bool(f.value & 1)

    def lone_graph_launches(self):
        """small batches replayed from a captured launch graph so far (masp_hip_ctx_lone_graph_launches)"""
        v = C.c_uint64(0)
        self._check(self._L.masp_hip_ctx_lone_graph_launches(self._h, C.byref(v)))
        return int(v.value)

    def device_proofs(self):
        """proofs written so far by each device context of this prover (masp_hip_ctx_device_proofs)"""
        n = self.device_count
        counts = (C.c_uint64 * n)()
        self._check(self._L.masp_hip_ctx_device_proofs(self._h, counts, n))
        return list(counts)

    def stream_concurrency(self, mains_only=False):
        """masp_hip_ctx_stream_concurrency -> (streams of this context — or only the ones that carry batches —, how many of them ran a kernel at
        the same time)"""
        n, c = C.c_int(0), C.c_int(0)
        self._check(self._L.masp_hip_ctx_stream_concurrency(self._h, 1 if mains_only else 0, C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def device_status(self):
        """masp_hip_ctx_device_status -> ([0 or the error code that took device context d out], proofs put back on the queue so far)"""
        n = self.device_count
        st, rq = (C.c_int32 * n)(), C.c_uint64(0)
        self._check(self._L.masp_hip_ctx_device_status(self._h, st, n, C.byref(rq)))
        return list(st), int(rq.value)

    def inject_fault(self, device, nth):
        """TEST HOOK masp_hip_ctx_inject_fault: the nth prove_batch call device context `device` receives from now fails (0 disarms)"""
        self._check(self._L.masp_hip_ctx_inject_fault(self._h, int(device), int(nth)))

    def quotient_h(self, a, b, c, logm):
        a, b, c = _u8(a, 32), _u8(b, 32), _u8(c, 32)
        out = np.zeros(((1 << logm) - 1, 32), dtype=np.uint8)
        self._check(self._L.masp_hip_quotient_h(self._h, _p(a), _p(b), _p(c), a.shape[0], logm, _p(out)))
        return out

    def ntt(self, data, logm, inverse=False):
        d = _u8(data, 32).copy()
        self._check(self._L.masp_hip_ntt(self._h, _p(d), logm, 1 if inverse else 0))
        return d

    # ---- measurement hooks ----
    def batch_upload(self, jobs):
        jobs = list(jobs)
        arr = (JobStruct * len(jobs))()
        keep = []
        for i, job in enumerate(jobs):          # (slot, inputs, aux, r, s[, None[, aux_form]]): as marshal_jobs
            slot, inputs, aux, r, s = job[:5]
            arr[i], k = self._job(slot, inputs, aux, r, s, None, job[6] if len(job) > 6 else AUX_CANONICAL)
            keep.append(k)
        h = self._L.masp_hip_batch_upload(self._h, len(jobs), arr)
        if h < 0:
            raise MaspHipError(-h, self._L.masp_hip_last_error(self._h).decode(errors="replace"))
        return h, len(jobs)

    def batch_prove_resident(self, handle, n):
        out = np.zeros((n, 192), dtype=np.uint8)
        ms = C.c_float(0)
        self._check(self._L.masp_hip_batch_prove_resident(self._h, handle, _p(out), C.byref(ms)))
        return [out[i].tobytes() for i in range(n)], ms.value

    def batch_prove_resident_steps(self, handle, n, steps, rs=None):
        """Proves the n resident jobs `steps` times; rs: u8[steps, n, 64] (r | s per job and step) or None.
        -> (u8[steps, n, 192], HIP-event milliseconds)"""
        out = np.zeros((steps, n, 192), dtype=np.uint8)
        ms = C.c_float(0)
        if rs is not None:
            rs = np.ascontiguousarray(rs, dtype=np.uint8)
            assert rs.shape == (steps, n, 64)
        self._check(self._L.masp_hip_batch_prove_resident_steps(self._h, handle, steps, _p(rs), _p(out), C.byref(ms)))
        return out, ms.value

    def batch_free(self, handle):
        self._check(self._L.masp_hip_batch_free(self._h, handle))

    def profile_enable(self, on=True):
        self._check(self._L.masp_hip_profile_enable(self._h, 1 if on else 0))

    def profile_read_split(self):
        """-> summed ms of the profiled bucket stages by kernel group: plan / records / copies, pass 1, shared inversions, pass 2, XYZZ accumulation"""
        ms = (C.c_double * 8)()
        self._check(self._L.masp_hip_profile_read_split(self._h, ms))
        return dict(zip(("plan_records_copies", "k_tree_pass1", "k_binv", "k_tree_pass2", "k_msm_accumulate_pts"), [float(x) for x in ms[:5]]))

    LONE_MARKS = ("start", "msm_a", "s_A", "msm_b1", "r_B1", "msm_b2", "g_b", "quotient", "msm_h", "msm_l", "g_a_g_c", "complete")

    def profile_read_lone(self):
        """masp_hip_profile_read_lone: where the chains of the last lone proof ended (ms of GPU time, HIP events) -> dict by mark"""
        ms = (C.c_double * 12)()
        self._check(self._L.masp_hip_profile_read_lone(self._h, ms))
        return {k: round(float(v), 3) for k, v in zip(self.LONE_MARKS, ms)}

    def profile_read(self):
        """-> (summed k_msm_accumulate<G1> ms, launches, algorithmic bytes)"""
        t, l, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.masp_hip_profile_read(self._h, C.byref(t), C.byref(l), C.byref(b)))
        return t.value, l.value, b.value

    def sync(self):
        self._check(self._L.masp_hip_sync(self._h))

    def bench_msm(self, handle, job, which, iters):
        ms, nb = C.c_float(0), C.c_uint32(0)
        self._check(self._L.masp_hip_bench_msm(self._h, handle, job, which, iters, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value


class GpuVerifyingKey:
    """Groth16 batch verification with the Miller loops on the GPU (masp_hip_verify_batch): same interface as
    host.PreparedVerifyingKey.verify_batch = bellman `verify_proofs_batch` (sapling/verifier/batch.rs:24-31)."""

    def __init__(self, ctx, params):
        self._ctx = ctx
        buf = _u8(params)
        n_ic = int.from_bytes(buf[864:868].tobytes(), "big")
        self._buf = buf[:868 + 96 * n_ic].copy()
        self.n_public = n_ic - 1
        h = C.c_void_p()
        ctx._check(ctx._L.masp_hip_vk_prepare(ctx._h, _p(self._buf), self._buf.size, C.byref(h)))
        self._h = h

    def verify_batch(self, proofs, public_inputs, randomness=None):
        """proofs: list of 192-byte strings; public_inputs: one list of ints / 32-byte values per proof (excluding ONE).
        True iff all verify (up to 2^-127); False says at least one is invalid, not which."""
        import secrets
        n = len(proofs)
        if n == 0:
            return True
        if len(public_inputs) != n or any(len(pi) != self.n_public for pi in public_inputs):
            return False
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8)
        if pr.size != 192 * n:
            return False
        pi = np.frombuffer(b"".join(_scalar32(x) for row in public_inputs for x in row), dtype=np.uint8) if self.n_public else None
        z = randomness if randomness is not None else secrets.token_bytes(16 * n)
        assert len(z) == 16 * n
        zb = np.frombuffer(z, dtype=np.uint8)
        ok = C.c_int(0)
        rc = self._ctx._L.masp_hip_verify_batch(self._ctx._h, self._h, n, _p(pr), _p(pi), self.n_public, _p(zb), C.byref(ok))
        if rc == 8:        # MASP_HIP_E_SCALAR_RANGE: a public input >= r — "does not verify", as host.PreparedVerifyingKey.verify_batch says
            return False
        self._ctx._check(rc)
        return ok.value == 1

    def verify_each(self, proofs, public_inputs):
        """proofs and public_inputs as for verify_batch -> one verdict per proof (masp_hip_verify_each), what host.PreparedVerifyingKey's
        masp_host_vk_verify says of it alone: 1 valid, 0 the pairing equation fails, 2 `Proof::read` refuses the proof, 3 a public input
        >= r.  Deterministic.  Every proof is 192 bytes and has n_public inputs (ValueError otherwise: there is no verdict for those)."""
        n = len(proofs)
        if len(public_inputs) != n or any(len(pi) != self.n_public for pi in public_inputs) or any(len(bytes(p)) != 192 for p in proofs):
            raise ValueError("verify_each: every proof is 192 bytes and comes with n_public inputs")
        if n == 0:
            return []
        pr = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8)
        pi = np.frombuffer(b"".join(_scalar32(x) for row in public_inputs for x in row), dtype=np.uint8) if self.n_public else None
        out = C.create_string_buffer(n)
        self._ctx._check(self._ctx._L.masp_hip_verify_each(self._ctx._h, self._h, n, _p(pr), _p(pi), self.n_public, out))
        return list(out.raw[:n])

    def verify_each_last_timing(self):
        """HIP-event milliseconds of the last verify_each: decode (with the copies in), acc, miller, final_exp, copy out"""
        ms = self._ctx._timing(self._ctx._L.masp_hip_verify_each_last_timing, 5, self._h)
        return dict(zip(("decode", "acc", "miller", "final_exp", "copy_out"), ms))

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._L.masp_hip_vk_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def r1cs_boolean_variables(cs):
    """masp_hip_r1cs_boolean_variables -> u8[n_inputs + n_aux]: 1 where the R1CS proves the variable boolean (host only: no device)."""
    out = np.zeros(cs.n_inputs + cs.n_aux, dtype=np.uint8)
    rc = load_library().masp_hip_r1cs_boolean_variables(cs.ref, _p(out))
    if rc:
        raise MaspHipError(rc)
    return out


def tree_entry_bound(n, window_bits, n_witness, n_boolean, share_percent=0):
    """masp_hip_tree_entry_bound: the entries a witness can put into the digit list of an n-point MSM (host only: no device)."""
    return int(load_library().masp_hip_tree_entry_bound(int(n), int(window_bits), int(n_witness), int(n_boolean), int(share_percent)))
