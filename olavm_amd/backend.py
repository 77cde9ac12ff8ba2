"""ctypes binding of include/ola_gpu.h.  Plumbing only -- no arithmetic happens in Python."""
import ctypes as C
import os

import numpy as np

U64P = C.POINTER(C.c_uint64)
_HERE = os.path.dirname(os.path.abspath(__file__))

OLA_NTT_EVALUATE = 0
OLA_NTT_INTERPOLATE = 1
OLA_NTT_COSET_LDE = 2
OLA_NTT_COSET_INTERPOLATE = 3
OLA_NTT_COSET_LDE_LEAF_ORDER = 4


class OlaGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ola_gpu error {code}: {msg}")
        self.code = code


class OlaExecRecords(C.Structure):
    """include/ola_gpu.h OlaExecRecords: what the executor recorded, every pointer host or device memory"""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("cpu_log_n", C.c_uint32), ("prog_log_n", C.c_uint32), ("range_bits", C.c_uint32),
                ("limb_bits", C.c_uint32), ("steps", C.c_void_p), ("n_steps", C.c_uint64), ("prog_listing", C.c_void_p), ("mem_cells", C.c_void_p),
                ("n_mem_cells", C.c_uint64), ("cmp_ops", C.c_void_p), ("n_cmp_ops", C.c_uint64), ("cpu_rc", C.c_void_p), ("n_cpu_rc", C.c_uint64),
                ("bitwise_ops", C.c_void_p), ("n_bitwise_ops", C.c_uint64), ("accesses", C.c_void_p), ("n_access", C.c_uint64),
                ("siblings", C.c_void_p), ("psdn_inputs", C.c_void_p), ("psdn_filters", C.c_void_p), ("psdn_stride", C.c_uint64),
                ("psdn_rows", C.c_uint64), ("tape_cells", C.c_void_p), ("n_tape_cells", C.c_uint64), ("psdn_calls", C.c_void_p),
                ("n_psdn_calls", C.c_uint64), ("listing_words", C.c_void_p), ("n_listing_words", C.c_uint64), ("code_addr", C.c_uint64 * 4),
                ("bitwise_beta", C.c_uint64), ("program_beta", C.c_uint64)]


OLA_RECORDS_REFERENCE_QUIRKS, OLA_RECORDS_ZERO_FILLER, OLA_RECORDS_RESULT_LINE, OLA_RECORDS_EXPLICIT_BETAS = 1, 2, 4, 8
TABLE_WIDTHS = (94, 29, 59, 6, 12, 134, 53, 48, 6, 26, 18, 40)      # `enum Table` order


class ResidentTable:
    """One table of a TableSet: device memory of the library's pool, with the few attributes of a GPU tensor that prove_with_traces,
    check_constraints and check_lookup read."""

    def __init__(self, ptr, ncols, log_n):
        self.ptr, self.shape = int(ptr), (int(ncols), 1 << int(log_n))

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def numel(self):
        return self.shape[0] * self.shape[1]

    def to_host(self):
        import torch
        t = torch.as_tensor(_DeviceBytes(self.ptr, 8 * self.numel()), device="cuda")
        return t.cpu().numpy().view(np.uint64).reshape(self.shape)


class TableSet:
    """ola_tables_from_records' twelve resident tables with their challenges; free() returns them to the context's pool."""

    def __init__(self, backend, handle):
        self.backend, self.handle = backend, handle
        ptrs, logs, params, compress = (C.c_void_p * 12)(), (C.c_uint32 * 12)(), (C.c_uint64 * 2)(), (C.c_uint64 * 12)()
        backend._chk(backend.lib.ola_tables_get(handle, ptrs, logs, params, compress))
        self.tables = [ResidentTable(ptrs[t], TABLE_WIDTHS[t], logs[t]) for t in range(12)]
        self.log_n = [int(x) for x in logs]
        self.params, self.compress = [int(x) for x in params], [int(x) for x in compress]

    def free(self):
        if self.handle:
            self.backend._chk(self.backend.lib.ola_tables_free(self.handle))
            self.handle, self.tables = None, []


class OlaGpuConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("stream", C.c_void_p), ("rate_bits", C.c_uint32), ("cap_height", C.c_uint32),
                ("proof_of_work_bits", C.c_uint32), ("fri_arity_bits", C.c_uint32), ("fri_final_poly_bits", C.c_uint32),
                ("num_query_rounds", C.c_uint32), ("num_challenges", C.c_uint32), ("hasher", C.c_uint32)]


class OlaScopeTime(C.Structure):
    """include/ola_gpu.h OlaScopeTime: one `timed!` scope of the last proof with device times."""
    _fields_ = [("name", C.c_char * 64), ("depth", C.c_uint32), ("ref_depth", C.c_uint32), ("table", C.c_int32),
                ("is_reference_scope", C.c_uint32), ("start_ms", C.c_double), ("ms", C.c_double), ("sharded_ms", C.c_double)]


class OlaPassTime(C.Structure):
    """include/ola_gpu.h OlaPassTime: the launches of one transform-pass kernel instantiation, summed."""
    _fields_ = [("kernel", C.c_char * 48), ("launches", C.c_uint32), ("reserved", C.c_uint32), ("total_ms", C.c_double), ("elements", C.c_double)]


class OlaConstraintFailure(C.Structure):
    _fields_ = [("table", C.c_uint32), ("section", C.c_uint32), ("index", C.c_uint32), ("kind", C.c_uint32),
                ("first_row", C.c_uint64), ("rows_failing", C.c_uint64)]


OLA_LOOKUP_MAX_VALUES = 24


class OlaLookupMismatch(C.Structure):
    """include/ola_gpu.h OlaLookupMismatch: one tuple that the two sides of a cross-table lookup carry unequally often."""
    _fields_ = [("looking_count", C.c_uint64), ("looked_count", C.c_uint64), ("looking_entry", C.c_uint32), ("looking_table", C.c_uint32),
                ("looking_row", C.c_uint64), ("looked_row", C.c_uint64), ("values", C.c_uint64 * OLA_LOOKUP_MAX_VALUES)]


class OlaVerifyReport(C.Structure):
    """include/ola_gpu.h OlaVerifyReport: the verdict of ola_verify_all_proof / ola_verify_opening and where a refusal stops."""
    _fields_ = [("accepted", C.c_uint32), ("reason", C.c_uint32), ("table", C.c_int32), ("query", C.c_int32), ("oracle_or_layer", C.c_int32),
                ("merkle_jobs", C.c_uint32), ("query_jobs", C.c_uint32), ("kernel_launches", C.c_uint32), ("host_ms", C.c_double),
                ("device_ms", C.c_double), ("message", C.c_char * 96)]


# OLA_VERIFY_* (include/ola_gpu.h), by value
VERIFY_REASONS = ("OK", "MALFORMED", "EMPTY_FRI", "SHAPE_OPENING_WIDTH", "SHAPE_ZS_WIDTH", "SHAPE_CTL_ZS_LAST_WIDTH", "SHAPE_QUOTIENT_WIDTH",
                  "QUOTIENT_IDENTITY", "SHAPE_CAP_HEIGHT", "SHAPE_QUERY_ROUNDS", "SHAPE_INITIAL_PROOFS", "SHAPE_LEAF_LEN", "SHAPE_INITIAL_PATH_LEN",
                  "SHAPE_STEPS", "SHAPE_EVALS_LEN", "SHAPE_STEP_PATH_LEN", "SHAPE_FINAL_POLY_LEN", "POW", "MERKLE_INITIAL", "FRI_CONSISTENCY",
                  "MERKLE_COMMIT", "FINAL_POLY", "CTL")


class VerifyResult:
    """What a verification says: truthy when the proof is accepted; otherwise `reason` (a name of VERIFY_REASONS; `code` its OLA_VERIFY_*
    value), `table`, `query`, `oracle_or_layer` (None where they do not apply) and `message` say where the reference's verifier stops."""

    def __init__(self, rep):
        opt = lambda v: None if v < 0 else int(v)
        self.accepted, self.code = bool(rep.accepted), int(rep.reason)
        self.reason = VERIFY_REASONS[self.code] if self.code < len(VERIFY_REASONS) else str(self.code)
        self.table, self.query, self.oracle_or_layer = opt(rep.table), opt(rep.query), opt(rep.oracle_or_layer)
        self.merkle_jobs, self.query_jobs, self.kernel_launches = int(rep.merkle_jobs), int(rep.query_jobs), int(rep.kernel_launches)
        self.host_ms, self.device_ms = float(rep.host_ms), float(rep.device_ms)
        self.message = rep.message.decode()

    def __bool__(self):
        return self.accepted

    def __repr__(self):
        return "VerifyResult(%s)" % self.message


CHECK_SECTIONS = ("AIR", "PERMUTATION", "LOOKUP")
CONSTRAINT_KINDS = ("constraint", "constraint_transition", "constraint_first_row", "constraint_last_row")


class OlaChallenger(C.Structure):
    _fields_ = [("sponge_state", C.c_uint64 * 12), ("input_buffer", C.c_uint64 * 8), ("output_buffer", C.c_uint64 * 8),
                ("input_len", C.c_uint32), ("output_len", C.c_uint32), ("hasher", C.c_uint32), ("reserved", C.c_uint32)]


# GenericConfig::Hasher (plonk/config.rs:112-161): PoseidonGoldilocksConfig / Blake3GoldilocksConfig / Poseidon2GoldilocksConfig /
# Poseidon2GoldilocksConfig2 (Poseidon2 trees and transcript, Poseidon proof of work)
OLA_HASH_POSEIDON, OLA_HASH_BLAKE3, OLA_HASH_POSEIDON2, OLA_HASH_POSEIDON2_POW_POSEIDON = 0, 1, 2, 3
OLA_HASH_KECCAK = 5   # 4 is unassigned
HASHERS = {"poseidon": OLA_HASH_POSEIDON, "blake3": OLA_HASH_BLAKE3, "poseidon2": OLA_HASH_POSEIDON2,
           "poseidon2_pow_poseidon": OLA_HASH_POSEIDON2_POW_POSEIDON, OLA_HASH_POSEIDON: OLA_HASH_POSEIDON, OLA_HASH_BLAKE3: OLA_HASH_BLAKE3,
           OLA_HASH_POSEIDON2: OLA_HASH_POSEIDON2, OLA_HASH_POSEIDON2_POW_POSEIDON: OLA_HASH_POSEIDON2_POW_POSEIDON,
           "keccak": OLA_HASH_KECCAK, OLA_HASH_KECCAK: OLA_HASH_KECCAK}


def lib_path():
    return os.path.join(_HERE, "lib", "libola_gpu.so")


_lib = None


def load_library():
    """Load libola_gpu.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise OlaGpuError(-7, f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the backend has no CPU fallback)")
    # torch bundles its own libamdhip64.so.7 + HSA runtime; two HIP runtimes in one process fight over the device, so
    # let torch's load first (same SONAME -> the dynamic loader then binds our library to the already-loaded one).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(p)
    L.ola_gpu_last_error.restype = C.c_char_p
    L.ola_gpu_init.argtypes = [C.POINTER(OlaGpuConfig), C.POINTER(C.c_void_p)]
    L.ola_gpu_abi_version.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    a, b = C.c_size_t(), C.c_size_t()
    if L.ola_gpu_abi_version(C.byref(a), C.byref(b)) != 7 or a.value != C.sizeof(OlaChallenger) or b.value != C.sizeof(OlaGpuConfig):
        raise OlaGpuError(-7, "libola_gpu.so and olavm_amd/backend.py disagree on the ABI revision or struct sizes: rebuild the library")
    L.ola_gpu_init_multi.argtypes = [C.POINTER(OlaGpuConfig), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ola_gpu_device_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_gpu_collective.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    L.ola_gpu_all_gather_check.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.ola_gpu_proof_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.ola_gpu_phase_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
    L.ola_gpu_free.argtypes = [C.c_void_p]
    L.ola_gpu_sync.argtypes = [C.c_void_p]
    L.ola_ntt_batch.argtypes = [C.c_void_p, C.c_int32, U64P, U64P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    L.ola_ntt_batch_dev.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_uint64, C.c_uint32]
    L.ola_poseidon_permute.argtypes = [C.c_void_p, U64P, C.c_size_t]
    L.ola_poseidon2_permute.argtypes = [C.c_void_p, U64P, C.c_size_t]
    L.ola_hash_rows.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_size_t, U64P]
    L.ola_merkle_cap.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_size_t, C.c_uint32, U64P]
    L.ola_pow.argtypes = [C.c_void_p, U64P, C.c_uint32, U64P]
    for f in ("ola_commit_values", "ola_commit_coeffs"):
        getattr(L, f).argtypes = [C.c_void_p, C.POINTER(U64P), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), U64P]
    for f in ("ola_commit_values_dev", "ola_commit_coeffs_dev"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), U64P]
    L.ola_batch_free.argtypes = [C.c_void_p, C.c_void_p]
    L.ola_batch_shape.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ola_batch_get_coeffs.argtypes = [C.c_void_p, C.c_void_p, U64P]
    L.ola_batch_get_leaf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, U64P, U64P]
    L.ola_batch_get_lde_row.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, U64P]
    L.ola_challenger_init.argtypes = [C.POINTER(OlaChallenger)]
    L.ola_challenger_init_hasher.argtypes = [C.POINTER(OlaChallenger), C.c_uint32]
    L.ola_challenger_init_keccak.argtypes = [C.POINTER(OlaChallenger)]
    L.ola_challenger_observe_cap.argtypes = [C.POINTER(OlaChallenger), U64P, C.c_size_t]
    L.ola_blake3_hash_elements.argtypes = [U64P, C.c_size_t, U64P]
    L.ola_keccak_hash_elements.argtypes = [U64P, C.c_size_t, U64P]
    L.ola_challenger_observe.argtypes = [C.POINTER(OlaChallenger), U64P, C.c_size_t]
    L.ola_challenger_get.argtypes = [C.POINTER(OlaChallenger), U64P, C.c_size_t]
    L.ola_challenger_compact.argtypes = [C.POINTER(OlaChallenger)]
    L.ola_open_and_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(OlaChallenger),
                                     C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    # the opening proof one step per call (FriSteps)
    L.ola_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, U64P, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t),
                           C.POINTER(C.c_void_p)]
    L.ola_fri_plan.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ola_fri_commit_begin.argtypes = [C.c_void_p, U64P]
    L.ola_fri_commit_next_layer.argtypes = [C.c_void_p, U64P, U64P]
    L.ola_fri_commit_finish.argtypes = [C.c_void_p, U64P, U64P, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_fri_query.argtypes = [C.c_void_p, U64P, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_fri_free.argtypes = [C.c_void_p]
    for f in ("ola_open", "ola_fri_plan", "ola_fri_commit_begin", "ola_fri_commit_next_layer", "ola_fri_commit_finish", "ola_fri_query", "ola_fri_free"):
        getattr(L, f).restype = C.c_int32
    L.ola_prove_with_traces.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(U64P), C.POINTER(C.c_uint32), U64P, U64P,
                                        C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_prove_with_traces_cols.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(C.POINTER(U64P)), C.POINTER(C.c_uint32), U64P, U64P,
                                             C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_gpu_scope_times.argtypes = [C.c_void_p, C.c_int32, C.POINTER(OlaScopeTime), C.c_uint32, C.POINTER(C.c_uint32)]
    L.ola_gpu_upload_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.ola_gpu_warmup.argtypes = [C.c_int32, C.c_uint32, U64P, C.c_size_t]
    L.ola_gpu_warmup_wait.argtypes = [C.POINTER(C.c_double)]
    L.ola_gpu_ntt_pass_times.argtypes = [C.c_void_p, C.c_int32, C.POINTER(OlaPassTime), C.c_uint32, C.POINTER(C.c_uint32)]
    L.ola_commit_values_shard.argtypes = [C.c_void_p, C.POINTER(U64P), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_void_p), U64P]
    L.ola_commit_values_shard_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_void_p), U64P]
    L.ola_generate_poseidon_trace.argtypes = [C.c_void_p, U64P, U64P, C.c_size_t, U64P]
    L.ola_prove_single_table.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_uint32, C.POINTER(U64P), C.c_void_p, U64P, U64P, U64P,
                                         C.POINTER(OlaChallenger), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_take_pending_proof.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ola_permuted_cols.argtypes = [C.c_void_p, U64P, U64P, C.c_size_t, U64P, U64P]
    L.ola_permuted_cols_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ola_generate_rc_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_generate_bitwise_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_generate_prog_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.ola_generate_cpu_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.ola_generate_prog_trace_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                                C.POINTER(C.c_uint64)]
    L.ola_generate_memory_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                            C.POINTER(C.c_uint64)]
    L.ola_generate_cmp_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L.ola_generate_storage_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]
    L.ola_generate_poseidon_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_generate_tape_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_generate_poseidon_chunk_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ola_generate_prog_chunk_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.POINTER(C.c_uint32)]
    L.ola_tables_from_records.argtypes = [C.c_void_p, C.POINTER(OlaExecRecords), C.POINTER(C.c_void_p)]
    L.ola_tables_get.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ola_tables_free.argtypes = [C.c_void_p]
    L.ola_prove_from_records.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(OlaExecRecords), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    for f in ("ola_tables_from_records", "ola_tables_get", "ola_tables_free", "ola_prove_from_records"):
        getattr(L, f).restype = C.c_int32
    for f in ("ola_generate_rc_trace", "ola_generate_bitwise_trace", "ola_generate_prog_trace", "ola_generate_cpu_trace",
              "ola_generate_prog_trace_steps", "ola_generate_memory_trace", "ola_generate_cmp_trace", "ola_generate_storage_trace",
              "ola_generate_poseidon_table", "ola_generate_tape_trace", "ola_generate_poseidon_chunk_trace", "ola_generate_prog_chunk_trace"):
        getattr(L, f).restype = C.c_int32
    L.ola_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, ALL_GATHER_FN, C.c_void_p]
    L.ola_set_shard_options.argtypes = [C.c_void_p, C.c_uint32]
    L.ola_gpu_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.ola_table_shape.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]
    L.ola_perm_z.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(U64P), U64P, U64P]
    L.ola_ctl_z.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(U64P), U64P, U64P]
    L.ola_quotient.argtypes = [C.c_void_p, U64P, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, U64P, U64P, U64P, U64P, U64P]
    L.ola_gpu_memory_stats.argtypes = [C.c_void_p, U64P, C.c_int32]
    L.ola_gpu_selftest.argtypes = [C.c_void_p, C.c_uint64, U64P]
    L.ola_gpu_reserve.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(C.c_uint32)]
    L.ola_air_kernels_available.argtypes = [U64P, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ola_air_kernels_available_cfg.argtypes = [C.POINTER(OlaGpuConfig), U64P, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ola_air_kernels_available_cfg.restype = C.c_int32
    L.ola_check_constraints.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(C.POINTER(U64P)), C.POINTER(C.c_uint32), U64P, U64P, C.c_uint32,
                                        C.POINTER(OlaConstraintFailure), C.c_uint32, C.POINTER(C.c_uint32)]
    L.ola_check_constraints.restype = C.c_int32
    L.ola_check_lookup.argtypes = [C.c_void_p, U64P, C.c_size_t, C.POINTER(C.POINTER(U64P)), C.POINTER(C.c_uint32), C.c_uint32,
                                   C.POINTER(OlaLookupMismatch), C.c_uint32, C.POINTER(C.c_uint32), U64P, C.POINTER(C.c_uint32)]
    L.ola_check_lookup.restype = C.c_int32
    L.ola_verify_all_proof.argtypes = [C.c_void_p, U64P, C.c_size_t, U64P, C.c_char_p, C.c_size_t, C.POINTER(OlaVerifyReport)]
    L.ola_verify_all_proof.restype = C.c_int32
    L.ola_verify_opening.argtypes = [C.c_void_p, U64P, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t,
                                     C.POINTER(OlaChallenger), C.POINTER(OlaVerifyReport)]
    L.ola_verify_opening.restype = C.c_int32
    L.ola_gpu_set_fri_reduction.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
    L.ola_gpu_set_fri_reduction.restype = C.c_int32
    L.ola_fri_reduction_arity_bits.argtypes = [C.POINTER(OlaGpuConfig), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    L.ola_fri_reduction_arity_bits.restype = C.c_int32
    _lib = L
    return L


EXPORTS = [
    "ola_gpu_init", "ola_gpu_free", "ola_gpu_last_error", "ola_gpu_sync", "ola_ntt_batch", "ola_ntt_batch_dev",
    "ola_poseidon_permute", "ola_poseidon2_permute", "ola_hash_rows", "ola_merkle_cap", "ola_commit_values", "ola_commit_coeffs",
    "ola_commit_values_dev", "ola_commit_coeffs_dev", "ola_batch_free", "ola_batch_shape", "ola_batch_get_coeffs",
    "ola_batch_get_leaf", "ola_batch_get_lde_row", "ola_challenger_init", "ola_challenger_observe",
    "ola_challenger_get", "ola_challenger_compact", "ola_challenger_init_hasher", "ola_challenger_init_keccak", "ola_challenger_observe_cap", "ola_blake3_hash_elements", "ola_keccak_hash_elements", "ola_open_and_prove", "ola_pow", "ola_prove_with_traces",
    "ola_air_kernels_available", "ola_commit_values_shard", "ola_commit_values_shard_dev", "ola_set_shard", "ola_gpu_trim", "ola_generate_poseidon_trace",
    "ola_permuted_cols", "ola_permuted_cols_dev", "ola_prove_single_table", "ola_take_pending_proof", "ola_gpu_memory_stats", "ola_gpu_selftest", "ola_gpu_reserve",
    "ola_table_shape", "ola_perm_z", "ola_ctl_z", "ola_quotient", "ola_set_shard_options", "ola_gpu_get_stream",
    "ola_gpu_abi_version", "ola_gpu_init_multi", "ola_gpu_device_count", "ola_gpu_proof_stats", "ola_gpu_phase_stats",
    "ola_gpu_collective", "ola_gpu_all_gather_check", "ola_prove_with_traces_cols", "ola_gpu_scope_times", "ola_gpu_upload_stats",
    "ola_gpu_warmup", "ola_gpu_warmup_wait", "ola_gpu_ntt_pass_times",
    "ola_check_constraints", "ola_check_lookup", "ola_generate_rc_trace", "ola_generate_bitwise_trace", "ola_generate_prog_trace",
    "ola_generate_cpu_trace", "ola_generate_prog_trace_steps", "ola_generate_memory_trace", "ola_generate_cmp_trace",
    "ola_generate_storage_trace", "ola_generate_poseidon_table",
    "ola_generate_tape_trace", "ola_generate_poseidon_chunk_trace", "ola_generate_prog_chunk_trace",
    "ola_tables_from_records", "ola_tables_get", "ola_tables_free", "ola_prove_from_records",
    "ola_open", "ola_fri_plan", "ola_fri_commit_begin", "ola_fri_commit_next_layer", "ola_fri_commit_finish", "ola_fri_query", "ola_fri_free",
    "ola_verify_all_proof", "ola_verify_opening",
    "ola_gpu_set_fri_reduction", "ola_fri_reduction_arity_bits",
    "ola_air_kernels_available_cfg",
]

# FriReductionStrategy (include/ola_gpu.h OLA_FRI_*)
FRI_STRATEGIES = {"constant_arity_bits": 0, "fixed": 1, "min_size": 2}


def _fri_reduction_args(reduction):
    """("fixed", [4, 3, 3]) | ("min_size", None | k) | ("constant_arity_bits",) | None -> (strategy, c_uint32 array or None, n)"""
    if reduction is None:
        reduction = ("constant_arity_bits",)
    if isinstance(reduction, str):
        reduction = (reduction,)
    name, arg = reduction[0], (reduction[1] if len(reduction) > 1 else None)
    if name not in FRI_STRATEGIES:
        raise ValueError("unknown FRI reduction strategy %r (one of %s)" % (name, ", ".join(FRI_STRATEGIES)))
    if name == "fixed":
        vals = [int(a) for a in (arg if arg is not None else [])]
    elif name == "min_size":
        vals = [] if arg is None else [int(arg)]
    else:
        vals = []
    if any(v < 0 or v > 0xFFFFFFFF for v in vals):
        raise ValueError("FRI reduction arguments are 32-bit unsigned numbers")
    arr = (C.c_uint32 * len(vals))(*vals) if vals else None
    return FRI_STRATEGIES[name], arr, len(vals)


def fri_reduction_arity_bits(reduction, degree_bits, **cfg):
    """ola_fri_reduction_arity_bits: the arity bits of every FRI layer of a 2^degree_bits-row table under `reduction` (as for
    Backend(fri_reduction=...)) and the configuration's rate_bits, cap_height, num_query_rounds, fri_arity_bits and
    fri_final_poly_bits.  Host only: needs no device."""
    L = load_library()
    c = OlaGpuConfig(-1, None, cfg.get("rate_bits", 3), cfg.get("cap_height", 4), cfg.get("proof_of_work_bits", 16),
                     cfg.get("fri_arity_bits", 4), cfg.get("fri_final_poly_bits", 5), cfg.get("num_query_rounds", 28),
                     cfg.get("num_challenges", 2), HASHERS[cfg.get("hasher", "poseidon")])
    strategy, arr, n = _fri_reduction_args(reduction)
    out, n_out = (C.c_uint32 * 64)(), C.c_uint32()
    code = L.ola_fri_reduction_arity_bits(C.byref(c), strategy, arr, n, int(degree_bits), out, 64, C.byref(n_out))
    if code != 0:
        raise OlaGpuError(code, L.ola_gpu_last_error().decode())
    return [int(out[i]) for i in range(n_out.value)]


def air_kernels_available(airset_blob, ntables, **cfg):
    """ola_air_kernels_available_cfg: which tables of the AIR set have a generated quotient kernel for a context created with `cfg`
    (the configuration's num_challenges decides).  Host only: needs no device."""
    L = load_library()
    c = OlaGpuConfig(-1, None, cfg.get("rate_bits", 3), cfg.get("cap_height", 4), cfg.get("proof_of_work_bits", 16),
                     cfg.get("fri_arity_bits", 4), cfg.get("fri_final_poly_bits", 5), cfg.get("num_query_rounds", 28),
                     cfg.get("num_challenges", 2), HASHERS[cfg.get("hasher", "poseidon")])
    blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
    flags = (C.c_uint8 * ntables)()
    code = L.ola_air_kernels_available_cfg(C.byref(c), _p(blob), blob.size, flags, ntables)
    if code != 0:
        raise OlaGpuError(code, L.ola_gpu_last_error().decode())
    return [bool(x) for x in flags]


def describe_column(col):
    """a lookup's `Column` (olavm_amd.air.dsl.Col) as text: "c5", "c5 + 1", "2*c7 + c8", "0" """
    parts = [("c%d" % c) if f == 1 else "%d*c%d" % (f, c) for c, f in col.terms]
    if col.constant or not parts:
        parts.append(str(col.constant))
    return " + ".join(parts)


def format_lookup_report(rep, max_tuples=None):
    """The text of a Backend.check_lookup report, one line per tuple -- the same lines ola_host::check_lookup prints."""
    t = rep["totals"]
    lines = ["lookup %d: width %d, %d looking rows, %d looked rows, %d mismatching tuples, %d rows unmatched"
             % (rep["lookup"], rep["width"], t[0], t[1], t[2], t[3])]
    show = rep["mismatches"] if max_tuples is None else rep["mismatches"][:max_tuples]
    for m in show:
        lk = "-" if m["looking_entry"] is None else "entry %d table %d row %d" % (m["looking_entry"], m["looking_table"], m["looking_row"])
        ld = "-" if m["looked_row"] is None else "row %d" % m["looked_row"]
        lines.append("  (%s): looking %d (first: %s), looked %d (first: %s)"
                     % (", ".join(str(v) for v in m["values"]), m["looking_count"], lk, m["looked_count"], ld))
    if len(show) < t[2]:
        lines.append("  ... %d more" % (t[2] - len(show)))
    return "\n".join(lines)


OLA_WARMUP_PINNED_RING = 1
OLA_TABLEGEN_REFERENCE_QUIRKS = 1
OLA_TABLEGEN_ZERO_FILLER = 1
OLA_CPU_STEP_WORDS = 66
OLA_MEM_CELL_WORDS = 5
OLA_STORAGE_ACCESS_WORDS = 14
OLA_STORAGE_WRITE, OLA_STORAGE_FOR_PROG, OLA_STORAGE_SILENT = 1, 2, 4
OLA_TAPE_CELL_WORDS = 3
OLA_POSEIDON_CALL_WORDS = 5
OLA_PROG_CHUNK_RESULT_LINE = 1


def warmup(device=-1, pinned_ring=True, airset=None):
    """ola_gpu_warmup: start the HIP runtime, open the device, load the code objects and -- with an AIR-set blob -- prime a context
    with a throw-away proof, all on a helper thread; returns at once (the reference's early hook: OlaStark::default() ->
    init_gpu(), circuits/src/stark/ola_stark.rs:47)."""
    L = load_library()
    if airset is not None:
        a = np.ascontiguousarray(airset, dtype=np.uint64)
        rc = L.ola_gpu_warmup(int(device), OLA_WARMUP_PINNED_RING if pinned_ring else 0, _p(a), a.size)
    else:
        rc = L.ola_gpu_warmup(int(device), OLA_WARMUP_PINNED_RING if pinned_ring else 0, None, 0)
    if rc != 0:
        raise OlaGpuError(rc, (L.ola_gpu_last_error() or b"").decode())


def warmup_wait():
    """ola_gpu_warmup_wait -> milliseconds the warm-up thread ran."""
    L = load_library()
    ms = C.c_double()
    rc = L.ola_gpu_warmup_wait(C.byref(ms))
    if rc != 0:
        raise OlaGpuError(rc, (L.ola_gpu_last_error() or b"").decode())
    return ms.value


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


def _p(a):
    return a.ctypes.data_as(U64P)


def _words(a, rows=None):
    """An input of the table generators -> (address, keep-alive, shape): a numpy array (made contiguous uint64), a 64-bit torch
    tensor on the GPU, or an integer device address (its shape is then the caller's to give)."""
    if a is None:
        return None, None, None
    if isinstance(a, int):
        if rows is None:
            raise ValueError("a device address needs its size (n_rows / n_ops / log_n)")
        return C.c_void_p(a), None, rows
    if hasattr(a, "data_ptr"):
        if not (a.is_contiguous() and a.element_size() == 8):
            raise ValueError("device-resident inputs must be contiguous 64-bit tensors")
        return C.c_void_p(a.data_ptr()), a, tuple(int(x) for x in a.shape)
    h = np.ascontiguousarray(a, dtype=np.uint64)
    return C.c_void_p(h.ctypes.data), h, h.shape


def bitwise_beta(ops, limb_bits=8, reference_quirks=False):
    """The compress challenge of the bitwise table as generation/builtin.rs:120-131 derives it: a fresh Poseidon Challenger observes
    the twelve limb columns at full height (op0, op1, res limbs 0..3) and draws one challenge -- on the host, through the library's
    host challenger (a sequential sponge: it stays off the device).  ops: (5, n_ops) words -- filter, tag, op0, op1, res."""
    ops = np.ascontiguousarray(ops, dtype=np.uint64).reshape(5, -1)
    n_ops = ops.shape[1]
    size = 1 << limb_bits
    n = 2
    while n < max(size, 3 * size * size, n_ops):
        n *= 2
    p = np.uint64(0xFFFFFFFF00000001)
    ch = Challenger()
    col = np.zeros(n, dtype=np.uint64)
    for k in (2, 3, 4):
        v = np.where(ops[k] >= p, ops[k] - p, ops[k])
        for i in range(4):
            col[:n_ops] = 0 if (reference_quirks and i == 3) else (v >> np.uint64(limb_bits * i)) & np.uint64(size - 1)
            ch.observe(col)
    return ch.get()


class _DeviceBytes:
    """View of raw device memory for torch (CUDA array interface): lets torch.distributed operate on the library's buffers."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 3}


class Challenger:
    """Host-side Fiat-Shamir transcript (iop/challenger.rs:36-162), state lives in an OlaChallenger struct."""

    def __init__(self, lib=None, hasher="poseidon"):
        self.lib = lib or load_library()
        self.c = OlaChallenger()
        if HASHERS[hasher] == OLA_HASH_KECCAK:          # its own entry point: ola_challenger_init_hasher takes 0..3 only
            rc = self.lib.ola_challenger_init_keccak(C.byref(self.c))
        else:
            rc = self.lib.ola_challenger_init_hasher(C.byref(self.c), HASHERS[hasher])
        if rc != 0:
            raise OlaGpuError(rc, self.lib.ola_gpu_last_error().decode())

    def observe_cap(self, digests):
        """observe_cap: 4 elements per Poseidon digest, 5 (7 bytes each) per Blake3 digest, 4 (7, 7, 7 and 4 bytes) per Keccak digest."""
        d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 4)
        self.lib.ola_challenger_observe_cap(C.byref(self.c), _p(d), d.shape[0])

    def observe(self, elems):
        e = np.ascontiguousarray(elems, dtype=np.uint64).ravel()
        self.lib.ola_challenger_observe(C.byref(self.c), _p(e), e.size)

    def get(self, n=None):
        out = np.empty(1 if n is None else n, dtype=np.uint64)
        self.lib.ola_challenger_get(C.byref(self.c), _p(out), out.size)
        return int(out[0]) if n is None else out

    def compact(self):
        self.lib.ola_challenger_compact(C.byref(self.c))

    def state(self):
        return np.array(list(self.c.sponge_state), dtype=np.uint64)

    def clone(self):
        o = Challenger(self.lib, int(self.c.hasher))
        C.memmove(C.byref(o.c), C.byref(self.c), C.sizeof(OlaChallenger))
        return o


class FriSteps:
    """An OlaFri: the opening proof of one table, one step per call (ola_fri_*; include/ola_gpu.h "one step per call")."""

    def __init__(self, be, handle):
        self.be, self.h = be, handle
        n, fl = C.c_uint32(), C.c_uint32()
        ab = (C.c_uint32 * 64)()
        be._chk(be.lib.ola_fri_plan(self.h, ab, 64, C.byref(n), C.byref(fl)))
        self.arity_bits, self.final_poly_len = [int(ab[i]) for i in range(n.value)], fl.value

    def begin(self, alpha):
        a = np.ascontiguousarray(alpha, dtype=np.uint64)
        self.be._chk(self.be.lib.ola_fri_commit_begin(self.h, _p(a)))

    def next_layer(self, beta=None):
        """-> the layer's cap (2^cap_height x 4 words); beta = the PREVIOUS layer's challenge, None for the first layer"""
        cap = np.empty((1 << self.be.cap_height, 4), dtype=np.uint64)
        b = None if beta is None else np.ascontiguousarray(beta, dtype=np.uint64)
        self.be._chk(self.be.lib.ola_fri_commit_next_layer(self.h, None if b is None else _p(b), _p(cap)))
        return cap

    def finish(self, beta=None):
        """-> final polynomial as (len, 2) words"""
        out = np.empty((max(self.final_poly_len, 1), 2), dtype=np.uint64)
        n = C.c_size_t(0)
        b = None if beta is None else np.ascontiguousarray(beta, dtype=np.uint64)
        self.be._chk(self.be.lib.ola_fri_commit_finish(self.h, None if b is None else _p(b), _p(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def query(self, x_index):
        x = np.ascontiguousarray(x_index, dtype=np.uint64)
        need = C.c_size_t(0)
        cap = 1 << 18
        while True:
            buf = C.create_string_buffer(cap)
            rc = self.be.lib.ola_fri_query(self.h, _p(x), x.size, buf, cap, C.byref(need))
            if rc != 0 and need.value > cap:
                cap = need.value
                continue
            self.be._chk(rc)
            return bytes(buf.raw[:need.value])

    def free(self):
        if self.h:
            self.be.lib.ola_fri_free(self.h)
            self.h = None


class Batch:
    """A committed PolynomialBatch resident in HBM (fri/oracle.rs:31-39)."""

    def __init__(self, be, handle, cap, shard_log_world=0):
        self.be, self.h, self._cap, self.shard_log_world = be, handle, cap, shard_log_world
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        be._chk(be.lib.ola_batch_shape(handle, C.byref(a), C.byref(b), C.byref(c)))
        self.ncols, self.log_n, self.rate_bits = a.value, b.value, c.value

    def cap(self):
        return self._cap

    def coeffs(self):
        out = np.empty((self.ncols, 1 << self.log_n), dtype=np.uint64)
        self.be._chk(self.be.lib.ola_batch_get_coeffs(self.be.ctx, self.h, _p(out)))
        return out

    def leaf(self, index):
        depth = self.log_n + self.rate_bits + self.shard_log_world - self.be.cap_height   # rate_bits is the local one
        row = np.empty(self.ncols, dtype=np.uint64)
        sib = np.empty((max(depth, 0), 4), dtype=np.uint64)
        self.be._chk(self.be.lib.ola_batch_get_leaf(self.be.ctx, self.h, index, _p(row), _p(sib) if depth > 0 else None))
        return row, sib

    def lde_row(self, index, step=1):
        row = np.empty(self.ncols, dtype=np.uint64)
        self.be._chk(self.be.lib.ola_batch_get_lde_row(self.be.ctx, self.h, index, step, _p(row)))
        return row

    def free(self):
        if self.h:
            self.be.lib.ola_batch_free(self.be.ctx, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Backend:
    """One OlaCtx.  `stream` may be a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).
    devices=[d0, d1, ...] makes it ONE context spanning those GPUs (ola_gpu_init_multi): prove_with_traces then runs on the
    coset partition inside the library, one call, one process; entries may repeat (logical ranks sharing a GPU)."""

    def __init__(self, device=-1, stream=None, devices=None, **cfg):
        self.lib = load_library()
        c = OlaGpuConfig(device, stream, cfg.get("rate_bits", 3), cfg.get("cap_height", 4),
                         cfg.get("proof_of_work_bits", 16), cfg.get("fri_arity_bits", 4),
                         cfg.get("fri_final_poly_bits", 5), cfg.get("num_query_rounds", 28), cfg.get("num_challenges", 2),
                         HASHERS[cfg.get("hasher", "poseidon")])
        self.hasher = int(c.hasher)
        self.cap_height = c.cap_height
        self.rate_bits = c.rate_bits
        self.num_challenges = int(c.num_challenges)
        self._cfg = c
        self.ctx = C.c_void_p()
        if devices is not None:
            dv = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            # collective="rccl" | "peer": the library reads OLA_COLLECTIVE when the context is created (ola_gpu_collective tells what it got)
            want, old = cfg.get("collective"), os.environ.get("OLA_COLLECTIVE")
            if want is not None:
                os.environ["OLA_COLLECTIVE"] = want
            try:
                self._chk(self.lib.ola_gpu_init_multi(C.byref(c), dv, len(devices), C.byref(self.ctx)))
            finally:
                if want is not None:
                    if old is None:
                        del os.environ["OLA_COLLECTIVE"]
                    else:
                        os.environ["OLA_COLLECTIVE"] = old
        else:
            self._chk(self.lib.ola_gpu_init(C.byref(c), C.byref(self.ctx)))
        if cfg.get("fri_reduction") is not None:
            try:
                self.set_fri_reduction(cfg["fri_reduction"])
            except Exception:
                self.close()            # (the constructor fails: nobody else can free the context)
                raise

    def set_fri_reduction(self, reduction):
        """ola_gpu_set_fri_reduction: ("fixed", [4, 3, 3]) | ("min_size", None | k) | ("constant_arity_bits",) for every call that
        begins from now on (proving and verifying); a refused argument leaves the previous strategy in place."""
        strategy, arr, n = _fri_reduction_args(reduction)
        self._chk(self.lib.ola_gpu_set_fri_reduction(self.ctx, strategy, arr, n))

    PHASES = ("leaf_hash", "merkle_levels", "fri_fold", "lde", "intt", "quotient", "open_eval")

    def phase_stats(self):
        """ola_gpu_phase_stats of the last proof (accounting must be on): {phase: (ms, units0, units1)}."""
        n = len(self.PHASES)
        out = (C.c_double * (6 * n))()
        self._chk(self.lib.ola_gpu_phase_stats(self.ctx, out, 2 * n))
        st = {name: (out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i, name in enumerate(self.PHASES)}
        # rows n + p: the phase's dominant scope (most bytes): (ms, bytes)
        self.phase_top = {name: (out[3 * (n + i)], out[3 * (n + i) + 1]) for i, name in enumerate(self.PHASES)}
        return st

    def device_count(self):
        n = C.c_uint32()
        self._chk(self.lib.ola_gpu_device_count(self.ctx, C.byref(n)))
        return n.value

    def collective(self):
        """ola_gpu_collective: who carries this context's exchanges -> {"carrier": "none" | "peer" | "rccl", "ranks": n, "note": str}"""
        carrier, ranks = C.c_uint32(), C.c_uint32()
        note = C.create_string_buffer(512)
        self._chk(self.lib.ola_gpu_collective(self.ctx, C.byref(carrier), C.byref(ranks), note, 512))
        return {"carrier": ("none", "peer", "rccl")[carrier.value], "ranks": ranks.value, "note": note.value.decode()}

    def all_gather_check(self, carrier, bytes_per_rank, reps=10):
        """ola_gpu_all_gather_check through "peer" or "rccl": -> (ms per gather on the slowest rank, wrong bytes over all ranks)"""
        ms, bad = C.c_double(), C.c_uint64()
        self._chk(self.lib.ola_gpu_all_gather_check(self.ctx, {"peer": 1, "rccl": 2}[carrier], bytes_per_rank, reps, C.byref(ms), C.byref(bad)))
        return ms.value, bad.value

    def proof_stats(self, enable=None):
        """ola_gpu_proof_stats: switch the accounting (True / False / None = leave) and return the last proof's figures."""
        out = (C.c_double * 8)()
        self._chk(self.lib.ola_gpu_proof_stats(self.ctx, -1 if enable is None else int(bool(enable)), out))
        return {"wall_ms": out[0], "sharded_ms_upto2": out[1], "sharded_ms_upto4": out[2], "sharded_ms_upto8": out[3],
                "exchange_bytes": int(out[4]), "exchanges": int(out[5]), "peer_exchanges": int(out[6]), "peer_bytes_moved": int(out[7])}

    def scope_times(self, enable=None):
        """ola_gpu_scope_times: switch the recording (True / False / None = leave); -> the last proof's `timed!` scopes as dicts."""
        n = C.c_uint32()
        self._chk(self.lib.ola_gpu_scope_times(self.ctx, -1 if enable is None else int(bool(enable)), None, 0, C.byref(n)))
        if n.value == 0:
            return []
        out = (OlaScopeTime * n.value)()
        self._chk(self.lib.ola_gpu_scope_times(self.ctx, -1, out, n.value, C.byref(n)))
        return [{"name": o.name.decode(), "depth": o.depth, "ref_depth": o.ref_depth, "table": o.table, "reference": bool(o.is_reference_scope),
                 "start_ms": o.start_ms, "ms": o.ms, "sharded_ms": o.sharded_ms} for o in out]

    def ntt_pass_times(self, enable=None):
        """ola_gpu_ntt_pass_times: switch the per-launch events of the transform passes (True / False / None = leave); -> what was
        recorded since the last call as {kernel: {"launches", "total_ms", "avg_ms", "elements"}}."""
        n = C.c_uint32()
        out = (OlaPassTime * 64)()
        self._chk(self.lib.ola_gpu_ntt_pass_times(self.ctx, -1 if enable is None else int(bool(enable)), out, 64, C.byref(n)))
        return {o.kernel.decode(): {"launches": o.launches, "total_ms": o.total_ms, "avg_ms": o.total_ms / max(o.launches, 1), "elements": o.elements}
                for o in out[:n.value]}

    def upload_stats(self):
        """ola_gpu_upload_stats of the last whole proof."""
        out = (C.c_double * 8)()
        self._chk(self.lib.ola_gpu_upload_stats(self.ctx, out))
        return {"waited_ms": out[0], "total_ms": out[1], "first_group_ms": out[2], "bytes": int(out[3]),
                "mode": ("staged", "pageable")[int(out[4])], "threads": int(out[5]), "link_bytes": int(out[6])}

    def _chk(self, rc):
        if rc != 0:
            raise OlaGpuError(rc, (self.lib.ola_gpu_last_error() or b"").decode())

    def close(self):
        if self.ctx:
            self.lib.ola_gpu_free(self.ctx)
            self.ctx = None

    def sync(self):
        self._chk(self.lib.ola_gpu_sync(self.ctx))

    # ---- NTT (host arrays, shape (batch, n)) ----
    def ntt(self, op, data, shift=7, blowup_log=0):
        d = np.ascontiguousarray(data, dtype=np.uint64)
        if d.ndim == 1:
            d = d[None, :]
        batch, n = d.shape
        log_n = int(n).bit_length() - 1
        grows = op in (OLA_NTT_COSET_LDE, OLA_NTT_COSET_LDE_LEAF_ORDER)
        out = np.empty((batch, n << blowup_log if grows else n), dtype=np.uint64)
        self._chk(self.lib.ola_ntt_batch(self.ctx, op, _p(d), _p(out), log_n, batch, shift, blowup_log))
        return out

    def ntt_dev(self, op, in_ptr, out_ptr, log_n, batch, shift=7, blowup_log=0, scratch_ptr=None):
        self._chk(self.lib.ola_ntt_batch_dev(self.ctx, op, in_ptr, out_ptr, scratch_ptr, log_n, batch, shift, blowup_log))

    # ---- hashing ----
    def poseidon(self, states):
        s = np.array(states, dtype=np.uint64).reshape(-1, 12)
        self._chk(self.lib.ola_poseidon_permute(self.ctx, _p(s), s.shape[0]))
        return s

    def poseidon2(self, states):
        """Poseidon2::poseidon2 (hash/poseidon2.rs:50) of each 12-element state, on the device, under any hasher of the context"""
        s = np.array(states, dtype=np.uint64).reshape(-1, 12)
        self._chk(self.lib.ola_poseidon2_permute(self.ctx, _p(s), s.shape[0]))
        return s

    def hash_rows(self, rows):
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.empty((r.shape[0], 4), dtype=np.uint64)
        self._chk(self.lib.ola_hash_rows(self.ctx, _p(r), r.shape[0], r.shape[1], _p(out)))
        return out

    def merkle_cap(self, leaves, cap_height):
        lv = np.ascontiguousarray(leaves, dtype=np.uint64)
        out = np.empty((1 << cap_height, 4), dtype=np.uint64)
        self._chk(self.lib.ola_merkle_cap(self.ctx, _p(lv), lv.shape[0], lv.shape[1], cap_height, _p(out)))
        return out

    def pow(self, h4, bits=16):
        h = np.ascontiguousarray(h4, dtype=np.uint64)
        w = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.ola_pow(self.ctx, _p(h), bits, _p(w)))
        return int(w[0])

    # ---- commitments ----
    def commit(self, cols, from_coeffs=False):
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        ncols, n = cols.shape
        ptrs = (U64P * ncols)(*[cols[i].ctypes.data_as(U64P) for i in range(ncols)])
        h = C.c_void_p()
        cap = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        f = self.lib.ola_commit_coeffs if from_coeffs else self.lib.ola_commit_values
        self._chk(f(self.ctx, ptrs, ncols, int(n).bit_length() - 1, C.byref(h), _p(cap)))
        return Batch(self, h, cap)

    def commit_dev(self, dev_ptr, ncols, log_n, from_coeffs=False):
        h = C.c_void_p()
        cap = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        f = self.lib.ola_commit_coeffs_dev if from_coeffs else self.lib.ola_commit_values_dev
        self._chk(f(self.ctx, dev_ptr, ncols, log_n, C.byref(h), _p(cap)))
        return Batch(self, h, cap)

    def commit_shard(self, cols, rank, world, dev_ptr=None, ncols=None, log_n=None):
        """This GPU's share of a commitment under the coset partition (ola_commit_values_shard): -> Batch whose cap() is
        the slice [rank*16/world, (rank+1)*16/world) of the full Merkle cap.  Pass `cols` (host array) or dev_ptr/ncols/
        log_n (device-resident column-major values)."""
        lw = int(world).bit_length() - 1
        h = C.c_void_p()
        cap = np.empty(((1 << self.cap_height) >> lw, 4), dtype=np.uint64)
        if dev_ptr is not None:
            self._chk(self.lib.ola_commit_values_shard_dev(self.ctx, dev_ptr, ncols, log_n, rank, world, C.byref(h), _p(cap)))
        else:
            cols = np.ascontiguousarray(cols, dtype=np.uint64)
            ncols, n = cols.shape
            ptrs = (U64P * ncols)(*[cols[i].ctypes.data_as(U64P) for i in range(ncols)])
            self._chk(self.lib.ola_commit_values_shard(self.ctx, ptrs, ncols, int(n).bit_length() - 1, rank, world, C.byref(h), _p(cap)))
        return Batch(self, h, cap, shard_log_world=lw)

    def generate_poseidon_trace(self, inputs, filters=None):
        """Poseidon STARK table (134 x n) from permutation inputs (12 x n) and optional lookup filters (4 x n)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        assert inputs.shape[0] == 12
        n = inputs.shape[1]
        f = None if filters is None else np.ascontiguousarray(filters, dtype=np.uint64)
        out = np.empty((134, n), dtype=np.uint64)
        self._chk(self.lib.ola_generate_poseidon_trace(self.ctx, _p(inputs), None if f is None else _p(f), n, _p(out)))
        return out

    def permuted_cols(self, inputs, table):
        """lookup.rs permuted_cols on the device: -> (sorted canonical inputs, permuted table), both uint64 arrays."""
        a = np.ascontiguousarray(inputs, dtype=np.uint64)
        b = np.ascontiguousarray(table, dtype=np.uint64)
        assert a.ndim == 1 and a.shape == b.shape
        pi, pt = np.empty_like(a), np.empty_like(a)
        self._chk(self.lib.ola_permuted_cols(self.ctx, _p(a), _p(b), a.shape[0], _p(pi), _p(pt)))
        return pi, pt

    def permuted_cols_dev(self, in_ptr, table_ptr, n, out_in_ptr, out_table_ptr):
        self._chk(self.lib.ola_permuted_cols_dev(self.ctx, in_ptr, table_ptr, n, out_in_ptr, out_table_ptr))

    # ---- whole derived tables from their primary columns (ola_generate_*_trace) ----
    # Inputs: numpy arrays, 64-bit torch tensors on this GPU, or integer device addresses.  out: None -> a new numpy array is
    # returned; a torch tensor on this GPU or an integer device address -> written in place (the table never crosses the link) and
    # log_n is returned.  Device buffers must be complete when the call is made (torch.cuda.synchronize() after copies and fills
    # on torch's stream): the library works on the context's stream.
    def _table_out(self, out, ncols, log_n):
        if out is None:
            t = np.empty((ncols, 1 << log_n), dtype=np.uint64)
            return C.c_void_p(t.ctypes.data), t
        if isinstance(out, int):
            return C.c_void_p(out), log_n
        if hasattr(out, "data_ptr"):
            if not (out.is_contiguous() and out.element_size() == 8 and out.numel() >= ncols << log_n):
                raise ValueError("out must be a contiguous 64-bit tensor of at least ncols * 2^log_n words")
            return C.c_void_p(out.data_ptr()), log_n
        t = np.ascontiguousarray(out)
        if t is not out or t.dtype != np.uint64 or t.size < ncols << log_n:
            raise ValueError("out must be a contiguous uint64 array of at least ncols * 2^log_n words")
        return C.c_void_p(t.ctypes.data), log_n

    def rc_trace_log_n(self, n_rows, range_bits=16):
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_rc_trace(self.ctx, None, None, n_rows, range_bits, None, C.byref(log_n)))
        return log_n.value

    def bitwise_trace_log_n(self, n_ops, limb_bits=8):
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_bitwise_trace(self.ctx, None, n_ops, limb_bits, 0, 0, None, C.byref(log_n)))
        return log_n.value

    def generate_rc_trace(self, vals, filters=None, range_bits=16, out=None, n_rows=None):
        """ola_generate_rc_trace: the range-check table (12 x n) from vals (n_rows) and filters (4 x n_rows, or None for zeros).
        n_rows must be given when vals is a device address."""
        pv, kv, shape = _words(vals, None if n_rows is None else (n_rows,))
        n_rows = int(np.prod(shape)) if shape is not None else 0
        pf, kf, fshape = _words(filters, (4, n_rows))
        if fshape is not None and int(np.prod(fshape)) != 4 * n_rows:
            raise ValueError("filters must be 4 x n_rows")
        log_n = self.rc_trace_log_n(n_rows, range_bits)
        po, ret = self._table_out(out, 12, log_n)
        got = C.c_uint32()
        self._chk(self.lib.ola_generate_rc_trace(self.ctx, pv if n_rows else None, pf, n_rows, range_bits, po, C.byref(got)))
        return ret

    def generate_bitwise_trace(self, ops, beta, limb_bits=8, reference_quirks=False, out=None, n_ops=None):
        """ola_generate_bitwise_trace: the bitwise table (59 x n) from ops (5 x n_ops: filter, tag, op0, op1, res) and the compress
        challenge beta (bitwise_beta derives the reference's).  n_ops must be given when ops is a device address."""
        po_, ko, shape = _words(ops, None if n_ops is None else (5, n_ops))
        if shape is None:
            n_ops = 0
        else:
            if int(np.prod(shape)) % 5:
                raise ValueError("ops must be 5 x n_ops")
            n_ops = int(np.prod(shape)) // 5
        log_n = self.bitwise_trace_log_n(n_ops, limb_bits)
        po, ret = self._table_out(out, 59, log_n)
        got = C.c_uint32()
        self._chk(self.lib.ola_generate_bitwise_trace(self.ctx, po_ if n_ops else None, n_ops, limb_bits, int(beta) % (1 << 64),
                                                      OLA_TABLEGEN_REFERENCE_QUIRKS if reference_quirks else 0, po, C.byref(got)))
        return ret

    def generate_prog_trace(self, exec_side, prog_side, beta, out=None, log_n=None):
        """ola_generate_prog_trace: the program table (18 x n) from the executed side and the listing side, each 7 x n (four
        code-address words, pc, inst, filter) at full height.  log_n must be given when the sides are device addresses."""
        pe, ke, es = _words(exec_side, None if log_n is None else (7, 1 << log_n))
        pp, kp, ps = _words(prog_side, None if log_n is None else (7, 1 << log_n))
        if es is None or ps is None or tuple(es) != tuple(ps) or len(es) != 2 or es[0] != 7 or es[1] & (es[1] - 1) or es[1] < 2:
            raise ValueError("exec_side and prog_side must both be 7 x 2^log_n")
        log_n = int(es[1]).bit_length() - 1
        po, ret = self._table_out(out, 18, log_n)
        self._chk(self.lib.ola_generate_prog_trace(self.ctx, pe, pp, log_n, int(beta) % (1 << 64), po))
        return ret

    def _steps(self, steps, n_steps):
        ps, ks, shape = _words(steps, None if n_steps is None else (OLA_CPU_STEP_WORDS, n_steps))
        if shape is None:
            return None, None, 0
        if len(shape) != 2 or shape[0] != OLA_CPU_STEP_WORDS:
            raise ValueError("steps must be OLA_CPU_STEP_WORDS x n_steps")
        return (ps if shape[1] else None), ks, int(shape[1])

    def generate_cpu_trace(self, steps, log_n, out=None, n_steps=None):
        """ola_generate_cpu_trace: the CPU table (94 x 2^log_n) from step records (OLA_CPU_STEP_WORDS x n_steps, column-major; None
        or zero columns for a table of padding rows).  n_steps must be given when steps is a device address."""
        ps, ks, n_steps = self._steps(steps, n_steps)
        po, ret = self._table_out(out, 94, log_n)
        self._chk(self.lib.ola_generate_cpu_trace(self.ctx, ps, n_steps, log_n, po))
        return ret

    def generate_prog_trace_steps(self, steps, prog_side, beta, zero_filler=False, out=None, n_steps=None, log_n=None):
        """ola_generate_prog_trace_steps: the program table (18 x 2^log_n) from step records and the listing side (7 x 2^log_n).
        -> (table or log_n, executed rows).  More executed rows than 2^log_n: OlaGpuError with the count in its `exec_rows`."""
        ps, ks, n_steps = self._steps(steps, n_steps)
        pp, kp, shape = _words(prog_side, None if log_n is None else (7, 1 << log_n))
        if shape is None or len(shape) != 2 or shape[0] != 7 or shape[1] & (shape[1] - 1) or shape[1] < 2:
            raise ValueError("prog_side must be 7 x 2^log_n")
        log_n = int(shape[1]).bit_length() - 1
        po, ret = self._table_out(out, 18, log_n)
        rows = C.c_uint64()
        rc = self.lib.ola_generate_prog_trace_steps(self.ctx, ps, n_steps, pp, log_n, int(beta) % (1 << 64),
                                                    OLA_TABLEGEN_ZERO_FILLER if zero_filler else 0, po, C.byref(rows))
        try:
            self._chk(rc)
        except OlaGpuError as e:
            e.exec_rows = rows.value
            raise
        return ret, rows.value

    def _list_out(self, dst, words):
        """A value list the memory / comparison generators fill -> (address or None, what the caller gets back): None = a new numpy array,
        False = not wanted (NULL), else a numpy array, a 64-bit torch tensor on the GPU or a device address with room for `words` words."""
        if dst is False:
            return None, None
        if dst is None:
            h = np.empty(words, dtype=np.uint64)
            return C.c_void_p(h.ctypes.data), h
        if isinstance(dst, int):
            return C.c_void_p(dst), dst
        if hasattr(dst, "data_ptr"):
            if not (dst.is_contiguous() and dst.element_size() == 8 and dst.numel() >= words):
                raise ValueError("a value list must be a contiguous 64-bit tensor with room for every value")
            return C.c_void_p(dst.data_ptr()), dst
        h = np.ascontiguousarray(dst)
        if h is not dst or h.dtype != np.uint64 or h.size < words:
            raise ValueError("a value list must be a contiguous uint64 array with room for every value")
        return C.c_void_p(h.ctypes.data), h

    def memory_trace_log_n(self, n_cells):
        log_n, counts = C.c_uint32(), (C.c_uint64 * 2)()
        self._chk(self.lib.ola_generate_memory_trace(self.ctx, None, n_cells, 0, None, C.byref(log_n), None, counts))
        return log_n.value

    def cmp_trace_log_n(self, n_ops):
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_cmp_trace(self.ctx, None, n_ops, None, C.byref(log_n), None))
        return log_n.value

    def generate_memory_trace(self, cells, reference_quirks=False, out=None, rc_out=None, n_cells=None):
        """ola_generate_memory_trace: the memory table (29 x n) from raw cells (OLA_MEM_CELL_WORDS x n_cells column-major, any order:
        address, clock, the op's one-hot word, value, is_write; None or zero columns for a table of padding rows), sorted on the device.
        -> (table or log_n, value list, (sort values, region values)).  rc_out: None = the range-checked sort values followed by the
        region values come back as a numpy array; False = they are not wanted; an array, GPU tensor or device address with room for
        2 n_cells words = they are written to its head and it is returned.  n_cells must be given when cells is a device address."""
        pc, kc, shape = _words(cells, None if n_cells is None else (OLA_MEM_CELL_WORDS, n_cells))
        if shape is not None and (len(shape) != 2 or shape[0] != OLA_MEM_CELL_WORDS):
            raise ValueError("cells must be OLA_MEM_CELL_WORDS x n_cells")
        n_cells = int(shape[1]) if shape is not None else 0
        log_n = self.memory_trace_log_n(n_cells)
        po, ret = self._table_out(out, 29, log_n)
        pr, rc = self._list_out(rc_out, 2 * n_cells)
        got, counts = C.c_uint32(), (C.c_uint64 * 2)()
        self._chk(self.lib.ola_generate_memory_trace(self.ctx, pc if n_cells else None, n_cells,
                                                     OLA_TABLEGEN_REFERENCE_QUIRKS if reference_quirks else 0, po, C.byref(got), pr, counts))
        if rc_out is None:
            rc = rc[:counts[0] + counts[1]]
        return ret, rc, (int(counts[0]), int(counts[1]))

    def generate_cmp_trace(self, ops, out=None, abs_diff_out=None, n_ops=None):
        """ola_generate_cmp_trace: the comparison table (6 x n) from operand pairs (2 x n_ops column-major: op0, op1; None or zero
        columns for a table of padding rows).  -> (table or log_n, ABS_DIFF of the live rows); abs_diff_out as rc_out of
        generate_memory_trace, with room for n_ops words.  n_ops must be given when ops is a device address."""
        pp, kp, shape = _words(ops, None if n_ops is None else (2, n_ops))
        if shape is not None and (len(shape) != 2 or shape[0] != 2):
            raise ValueError("ops must be 2 x n_ops")
        n_ops = int(shape[1]) if shape is not None else 0
        log_n = self.cmp_trace_log_n(n_ops)
        po, ret = self._table_out(out, 6, log_n)
        pd, diff = self._list_out(abs_diff_out, n_ops)
        got = C.c_uint32()
        self._chk(self.lib.ola_generate_cmp_trace(self.ctx, pp if n_ops else None, n_ops, po, C.byref(got), pd))
        return ret, diff

    def storage_trace_log_n(self, accesses, n_access=None):
        """log2 of the storage table's height for these records (a sizing call: the silent ones have no rows)"""
        pa, ka, shape = _words(accesses, None if n_access is None else (OLA_STORAGE_ACCESS_WORDS, n_access))
        n_access = int(shape[1]) if shape is not None else 0
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_storage_trace(self.ctx, pa if n_access else None, n_access, None, None, C.byref(log_n), None, None, 0, None))
        return log_n.value

    def generate_storage_trace(self, accesses, siblings=None, out=None, psdn_inputs=None, psdn_filters=None, roots_out=None, n_access=None):
        """ola_generate_storage_trace: the account-storage tree hashed on the device and the storage table (48 x n) from access records
        (OLA_STORAGE_ACCESS_WORDS x n_access column-major: key[4], value[4], pre_value[4], flags, psdn_row; None or zero columns for a
        table of padding rows).  siblings: None = the self-contained batch on an empty tree, else 1024 x n_access from the caller's tree.
        psdn_inputs / psdn_filters: None, or the (12, stride) / (4, stride) input buffers of generate_poseidon_table -- numpy arrays, GPU
        tensors or device addresses (then `psdn_stride` words per column is taken from the arrays' shape; for addresses pass a tuple
        (address, stride)) -- whose storage rows the call fills in place.  roots_out: None = the two roots come back as a numpy array
        of 8 words, False = not wanted, else as rc_out of generate_memory_trace.  -> (table or log_n, roots).  n_access must be given
        when accesses is a device address."""
        pa, ka, shape = _words(accesses, None if n_access is None else (OLA_STORAGE_ACCESS_WORDS, n_access))
        if shape is not None and (len(shape) != 2 or shape[0] != OLA_STORAGE_ACCESS_WORDS):
            raise ValueError("accesses must be OLA_STORAGE_ACCESS_WORDS x n_access")
        n_access = int(shape[1]) if shape is not None else 0
        ps, ks, sshape = _words(siblings, (1024, n_access))
        if sshape is not None and int(np.prod(sshape)) != 1024 * n_access:
            raise ValueError("siblings must be 1024 x n_access")
        if (psdn_inputs is None) != (psdn_filters is None):
            raise ValueError("psdn_inputs and psdn_filters go together")
        pi = pf = None
        stride = 0
        if psdn_inputs is not None:
            if isinstance(psdn_inputs, tuple):
                (ai, stride), (af, fstride) = psdn_inputs, psdn_filters
                pi, pf, ishape, fshape = C.c_void_p(ai), C.c_void_p(af), (12, stride), (4, fstride)
            else:
                for b in (psdn_inputs, psdn_filters):      # written in place: no silent copy
                    if not hasattr(b, "data_ptr") and not (isinstance(b, np.ndarray) and b.dtype == np.uint64 and b.flags.c_contiguous):
                        raise ValueError("psdn_inputs / psdn_filters must be contiguous uint64 arrays or GPU tensors")
                pi, ki, ishape = _words(psdn_inputs)
                pf, kf, fshape = _words(psdn_filters)
            if len(ishape) != 2 or ishape[0] != 12 or tuple(fshape) != (4, ishape[1]):
                raise ValueError("psdn_inputs must be 12 x stride and psdn_filters 4 x stride")
            stride = int(ishape[1])
        log_n = self.storage_trace_log_n(accesses, n_access)
        po, ret = self._table_out(out, 48, log_n)
        pr, roots = self._list_out(roots_out, 8)
        got = C.c_uint32()
        self._chk(self.lib.ola_generate_storage_trace(self.ctx, pa if n_access else None, n_access, ps if n_access else None, po, C.byref(got),
                                                      pi, pf, stride, pr))
        return ret, roots

    def poseidon_table_log_n(self, n_rows):
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_poseidon_table(self.ctx, None, None, n_rows, n_rows, None, C.byref(log_n)))
        return log_n.value

    def generate_poseidon_table(self, inputs, filters=None, n_rows=None, out=None, stride=None):
        """ola_generate_poseidon_table: the Poseidon table (134 x n, n = next_pow2(max(n_rows, 8))) from permutation inputs (12 x stride)
        and optional lookup filters (4 x stride); rows n_rows .. n are rows of all-zero inputs.  n_rows defaults to the stride;
        stride must be given when inputs is a device address."""
        pi, ki, shape = _words(inputs, None if stride is None else (12, stride))
        if shape is None or len(shape) != 2 or shape[0] != 12:
            raise ValueError("inputs must be 12 x stride")
        stride = int(shape[1])
        pf, kf, fshape = _words(filters, (4, stride))
        if fshape is not None and tuple(fshape) != (4, stride):
            raise ValueError("filters must be 4 x stride")
        n_rows = stride if n_rows is None else int(n_rows)
        if n_rows > stride:
            raise ValueError("n_rows is larger than the stride")
        log_n = self.poseidon_table_log_n(n_rows)
        po, ret = self._table_out(out, 134, log_n)
        got = C.c_uint32()
        self._chk(self.lib.ola_generate_poseidon_table(self.ctx, pi if stride else None, pf if stride else None, n_rows, stride, po, C.byref(got)))
        return ret

    def _poseidon_table(self, poseidon_table, psdn_log_n):
        """the resident (or host) Poseidon table of the two chunk generators -> (address, keep-alive, log2 of its height)"""
        pt, kt, shape = _words(poseidon_table, None if psdn_log_n is None else (134, 1 << psdn_log_n))
        if shape is None or len(shape) != 2 or shape[0] != 134 or shape[1] & (shape[1] - 1) or shape[1] < 8:
            raise ValueError("poseidon_table must be 134 x 2^psdn_log_n")
        return pt, kt, int(shape[1]).bit_length() - 1

    def generate_tape_trace(self, cells, out=None, n_cells=None):
        """ola_generate_tape_trace: the tape table (6 x n, n = next_pow2(max(n_cells, 8))) from cells in execution order
        (OLA_TAPE_CELL_WORDS x n_cells column-major: tape address, the opcode's one-hot word, value; None or zero columns for the
        padding table), sorted by address on the device.  n_cells must be given when cells is a device address."""
        pc, kc, shape = _words(cells, None if n_cells is None else (OLA_TAPE_CELL_WORDS, n_cells))
        if shape is not None and (len(shape) != 2 or shape[0] != OLA_TAPE_CELL_WORDS):
            raise ValueError("cells must be OLA_TAPE_CELL_WORDS x n_cells")
        n_cells = int(shape[1]) if shape is not None else 0
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_tape_trace(self.ctx, None, n_cells, None, C.byref(log_n)))
        po, ret = self._table_out(out, 6, log_n.value)
        self._chk(self.lib.ola_generate_tape_trace(self.ctx, pc if n_cells else None, n_cells, po, C.byref(log_n)))
        return ret

    def generate_poseidon_chunk_trace(self, calls, poseidon_table, out=None, n_calls=None, psdn_log_n=None):
        """ola_generate_poseidon_chunk_trace: the Poseidon-chunk table (53 x n) from POSEIDON call records (OLA_POSEIDON_CALL_WORDS x
        n_calls column-major: clk, src, len, dst, psdn_row; None or zero columns for the padding table) and the Poseidon table
        (134 x 2^psdn_log_n) whose rows psdn_row .. psdn_row + len / 8 hashed each call's blocks.  n_calls / psdn_log_n must be given
        for device addresses."""
        pc, kc, shape = _words(calls, None if n_calls is None else (OLA_POSEIDON_CALL_WORDS, n_calls))
        if shape is not None and (len(shape) != 2 or shape[0] != OLA_POSEIDON_CALL_WORDS):
            raise ValueError("calls must be OLA_POSEIDON_CALL_WORDS x n_calls")
        n_calls = int(shape[1]) if shape is not None else 0
        pt, kt, psdn_log_n = self._poseidon_table(poseidon_table, psdn_log_n)
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_poseidon_chunk_trace(self.ctx, pc if n_calls else None, n_calls, pt, psdn_log_n, None, C.byref(log_n)))
        po, ret = self._table_out(out, 53, log_n.value)
        self._chk(self.lib.ola_generate_poseidon_chunk_trace(self.ctx, pc if n_calls else None, n_calls, pt, psdn_log_n, po, C.byref(log_n)))
        return ret

    def generate_prog_chunk_trace(self, words, code_addr, poseidon_table, result_line=False, out=None, n_words=None, psdn_log_n=None):
        """ola_generate_prog_chunk_trace: the program-chunk table (40 x n, n = next_pow2(max(n_words / 8, 8))) from the zero-padded
        listing, the four code-address words and the Poseidon table whose row i hashed listing words 8 i .. 8 i + 7.  n_words /
        psdn_log_n must be given for device addresses."""
        pw, kw, shape = _words(words, None if n_words is None else (n_words,))
        n_words = int(np.prod(shape)) if shape is not None else 0
        pa, ka, ashape = _words(code_addr, (4,))
        if ashape is None or int(np.prod(ashape)) != 4:
            raise ValueError("code_addr must be 4 words")
        pt, kt, psdn_log_n = self._poseidon_table(poseidon_table, psdn_log_n)
        flags = OLA_PROG_CHUNK_RESULT_LINE if result_line else 0
        log_n = C.c_uint32()
        self._chk(self.lib.ola_generate_prog_chunk_trace(self.ctx, None, n_words, None, flags, None, psdn_log_n, None, C.byref(log_n)))
        po, ret = self._table_out(out, 40, log_n.value)
        self._chk(self.lib.ola_generate_prog_chunk_trace(self.ctx, pw if n_words else None, n_words, pa, flags, pt, psdn_log_n, po, C.byref(log_n)))
        return ret

    def exec_records(self, rec, range_bits=16, limb_bits=8, reference_quirks=False, zero_filler=False, result_line=False, bitwise_beta=None,
                     program_beta=None, siblings=None):
        """The OlaExecRecords struct for the records of fastexec.instance(records_only=True) (numpy arrays, GPU tensors, or a mix).
        -> (struct, keep-alive list)"""
        assert (bitwise_beta is None) == (program_beta is None), "give both compress challenges or neither"
        keep = []

        def arr(key, rows):
            p, k, shape = _words(rec[key])
            keep.append(k)
            if rows is not None and (len(shape) != 2 or shape[0] != rows):
                raise ValueError("%s must be %d x n" % (key, rows))
            return (p.value if int(np.prod(shape)) else None), (int(shape[-1]) if len(shape) else 0)
        r = OlaExecRecords()
        r.size = C.sizeof(OlaExecRecords)
        r.flags = ((OLA_RECORDS_REFERENCE_QUIRKS if reference_quirks else 0) | (OLA_RECORDS_ZERO_FILLER if zero_filler else 0) |
                   (OLA_RECORDS_RESULT_LINE if result_line else 0) | (OLA_RECORDS_EXPLICIT_BETAS if bitwise_beta is not None else 0))
        r.cpu_log_n, r.prog_log_n, r.range_bits, r.limb_bits = rec["cpu_log_n"], rec["prog_log_n"], range_bits, limb_bits
        r.steps, r.n_steps = arr("steps", OLA_CPU_STEP_WORDS)
        r.prog_listing, n = arr("listing", 7)
        if n != 1 << rec["prog_log_n"]:
            raise ValueError("listing must be 7 x 2^prog_log_n")
        r.mem_cells, r.n_mem_cells = arr("cells", OLA_MEM_CELL_WORDS)
        r.cmp_ops, r.n_cmp_ops = arr("cmp_ops", 2)
        r.cpu_rc, r.n_cpu_rc = arr("cpu_rc", None)
        r.bitwise_ops, r.n_bitwise_ops = arr("bitwise_ops", 5)
        r.accesses, r.n_access = arr("accesses", OLA_STORAGE_ACCESS_WORDS)
        if siblings is not None:
            p, k, shape = _words(siblings)
            keep.append(k)
            r.siblings = p.value
        r.psdn_inputs, r.psdn_stride = arr("psdn_inputs", 12)
        r.psdn_filters, n = arr("psdn_filters", 4)
        if n != r.psdn_stride:
            raise ValueError("psdn_inputs and psdn_filters differ in stride")
        r.psdn_rows = rec.get("psdn_rows", r.psdn_stride)
        r.tape_cells, r.n_tape_cells = arr("tape_cells", OLA_TAPE_CELL_WORDS)
        r.psdn_calls, r.n_psdn_calls = arr("psdn_calls", OLA_POSEIDON_CALL_WORDS)
        r.listing_words, r.n_listing_words = arr("words", None)
        r.code_addr = (C.c_uint64 * 4)(*[int(x) for x in rec["code_addr"]])
        r.bitwise_beta, r.program_beta = (int(bitwise_beta) % (1 << 64), int(program_beta) % (1 << 64)) if bitwise_beta is not None else (0, 0)
        return r, keep

    def tables_from_records(self, rec, **kw):
        """ola_tables_from_records: all twelve tables resident, from the executor's records (exec_records' arguments).  -> TableSet"""
        r, keep = self.exec_records(rec, **kw)
        handle = C.c_void_p()
        self._chk(self.lib.ola_tables_from_records(self.ctx, C.byref(r), C.byref(handle)))
        return TableSet(self, handle)

    def prove_from_records(self, airset_blob, rec, cap=8 << 20, **kw):
        """ola_prove_from_records: AllProof bytes from the executor's records; no table crosses the link."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        r, keep = self.exec_records(rec, **kw)
        need = C.c_size_t(0)
        buf = C.create_string_buffer(cap)
        rc = self.lib.ola_prove_from_records(self.ctx, _p(blob), blob.size, C.byref(r), buf, cap, C.byref(need))
        if rc != 0 and need.value > cap:            # the proof is kept in the context: fetch it, do not prove again
            buf = C.create_string_buffer(need.value)
            rc = self.lib.ola_take_pending_proof(self.ctx, buf, need.value, C.byref(need))
        self._chk(rc)
        return bytes(buf.raw[:need.value])

    def trim(self):
        """Return the context's cached device buffers to the driver (ola_gpu_trim)."""
        self._chk(self.lib.ola_gpu_trim(self.ctx))

    # ---- per-phase entry points (one `timed!` scope of prove_single_table at a time) ----
    def table_shape(self, airset_blob, table):
        """-> dict(ncols, n_params, perm_zs, ctl_zs, quotient_degree_factor, permutation_batch_size)."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        out = (C.c_uint32 * 6)()
        self._chk(self.lib.ola_table_shape(self.ctx, _p(blob), blob.size, table, out))
        return dict(zip(("ncols", "n_params", "perm_zs", "ctl_zs", "quotient_degree_factor", "permutation_batch_size"), (int(x) for x in out)))

    def _zs_phase(self, fn, airset_blob, table, trace, challenges, count):
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        tr = np.ascontiguousarray(trace, dtype=np.uint64)
        ptrs = (U64P * tr.shape[0])(*[_p(tr[c]) for c in range(tr.shape[0])])
        cc = np.ascontiguousarray(np.array(challenges, dtype=np.uint64).reshape(-1))
        out = np.zeros((count, tr.shape[1]), dtype=np.uint64)
        self._chk(fn(self.ctx, _p(blob), blob.size, table, int(tr.shape[1]).bit_length() - 1, ptrs, _p(cc), _p(out) if count else _p(np.zeros(1, dtype=np.uint64))))
        return out

    def perm_z(self, airset_blob, table, trace, perm_challenges):
        """Permutation Z columns (values): perm_challenges = [batch_size][num_challenges] pairs (beta, gamma)."""
        return self._zs_phase(self.lib.ola_perm_z, airset_blob, table, trace, perm_challenges, self.table_shape(airset_blob, table)["perm_zs"])

    def ctl_z(self, airset_blob, table, trace, ctl_challenges):
        """CTL Z columns (values): ctl_challenges = [num_challenges] pairs (beta, gamma)."""
        return self._zs_phase(self.lib.ola_ctl_z, airset_blob, table, trace, ctl_challenges, self.table_shape(airset_blob, table)["ctl_zs"])

    def quotient(self, airset_blob, table, trace_batch, zs_batch, perm_challenges, ctl_challenges, alphas, params, n):
        """Coefficients of the num_challenges * quotient_degree_factor quotient chunk polynomials, [chunks][n]."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        q = self.table_shape(airset_blob, table)["quotient_degree_factor"]
        pc = None if perm_challenges is None else np.ascontiguousarray(np.array(perm_challenges, dtype=np.uint64).reshape(-1))
        cc = np.ascontiguousarray(np.array(ctl_challenges, dtype=np.uint64).reshape(-1))
        al = np.ascontiguousarray(alphas, dtype=np.uint64)
        pr = None if params is None or len(params) == 0 else np.ascontiguousarray(params, dtype=np.uint64)
        out = np.zeros((self.num_challenges * q, n), dtype=np.uint64)
        self._chk(self.lib.ola_quotient(self.ctx, _p(blob), blob.size, table, trace_batch.h, zs_batch.h, None if pc is None else _p(pc), _p(cc), _p(al),
                                        None if pr is None else _p(pr), _p(out)))
        return out

    def reserve(self, airset_blob, log_ns):
        """Start allocating the buffers of a coming proof in the background (ola_gpu_reserve); returns at once."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        logs = (C.c_uint32 * len(log_ns))(*[int(x) for x in log_ns])
        self._chk(self.lib.ola_gpu_reserve(self.ctx, _p(blob), blob.size, logs))

    def selftest(self, pairs=1 << 28):
        """Device field-arithmetic self-test (carry-flag reduction against the C++ form): number of mismatches."""
        out = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.ola_gpu_selftest(self.ctx, int(pairs), _p(out)))
        return int(out[0])

    def memory_stats(self, reset=False):
        """Device memory of the context's pool in bytes: dict(live, live_peak, reserved, reserved_peak)."""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.ola_gpu_memory_stats(self.ctx, _p(out), 1 if reset else 0))
        return dict(zip(("live", "live_peak", "reserved", "reserved_peak"), (int(x) for x in out)))

    def set_shard(self, rank, world, group=None):
        """Coset-partitioned proving (ola_set_shard): this context is rank `rank` of `world` GPUs.  The all-gather the
        library asks for runs through torch.distributed on `group` -- RCCL when the process group is "nccl" (device
        buffers are handed over as they are), host staging for "gloo" (tests).  world = 1 switches back."""
        if world == 1:
            self._chk(self.lib.ola_set_shard(self.ctx, 0, 1, ALL_GATHER_FN(0), None))
            self._shard_cb = None
            return
        import torch
        import torch.distributed as dist
        on_device = dist.get_backend(group) == "nccl"

        self.shard_calls = 0          # exchanges performed so far (observability / tests)

        # RCCL path: the collective is launched on the context's own stream (torch ExternalStream), so it is ordered with the
        # library's kernels by the stream itself -- no host synchronisation per exchange (OLA_SHARD_STREAM_ORDERED).
        ext = None
        if on_device:
            sp = C.c_void_p()
            self._chk(self.lib.ola_gpu_get_stream(self.ctx, C.byref(sp)))
            ext = torch.cuda.ExternalStream(sp.value)

        def all_gather(_user, send, recv, nbytes):
            self.shard_calls += 1
            try:
                src = torch.as_tensor(_DeviceBytes(send, nbytes), device="cuda")
                dst = torch.as_tensor(_DeviceBytes(recv, nbytes * world), device="cuda")
                if on_device:
                    with torch.cuda.stream(ext):
                        dist.all_gather_into_tensor(dst, src, group=group)
                else:
                    parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
                    dist.all_gather(parts, src.cpu(), group=group)
                    dst.copy_(torch.cat(parts))
                    torch.cuda.synchronize()
                return 0
            except Exception as e:          # noqa: BLE001 -- must not unwind through the C frame
                import sys
                print("ola all_gather callback failed:", repr(e), file=sys.stderr)
                return 1

        self._shard_cb = ALL_GATHER_FN(all_gather)      # keep the trampoline alive as long as the context uses it
        self._chk(self.lib.ola_set_shard(self.ctx, rank, world, self._shard_cb, None))
        self._chk(self.lib.ola_set_shard_options(self.ctx, 1 if on_device else 0))

    def prove_with_traces(self, airset_blob, traces, params=None, compress=None, cap=8 << 20):
        """AllProof bytes for the multi-table STARK described by `airset_blob` (olavm_amd.air.AirSet.blob()).

        A table is a 2-d numpy array (host, one column-major block), a contiguous 64-bit torch tensor resident on this GPU, or a
        LIST of 1-d uint64 arrays -- every column its own allocation, the reference's Vec<PolynomialValues<F>> (prover.rs:79-83).
        As soon as one table is a list the call goes through ola_prove_with_traces_cols (blocks become their column pointers)."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        pr = None if params is None else np.ascontiguousarray(params, dtype=np.uint64)
        cc = None if compress is None else np.ascontiguousarray(compress, dtype=np.uint64)
        need = C.c_size_t(0)
        buf = C.create_string_buffer(cap)
        if any(isinstance(t, (list, tuple)) for t in traces):
            keep, tabs, logs = [], [], []
            for t in traces:
                if isinstance(t, (list, tuple)):
                    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in t]
                    n = cols[0].size
                    if any(c.size != n for c in cols):
                        raise ValueError("columns of one table differ in length")
                    addrs = [c.ctypes.data for c in cols]
                elif hasattr(t, "data_ptr"):
                    if not (t.is_contiguous() and t.element_size() == 8):
                        raise ValueError("device-resident tables must be contiguous 64-bit tensors")
                    cols, n = t, int(t.shape[1])
                    addrs = [t.data_ptr() + 8 * n * c for c in range(int(t.shape[0]))]
                else:
                    cols = np.ascontiguousarray(t, dtype=np.uint64)
                    n = cols.shape[1]
                    addrs = [cols.ctypes.data + 8 * n * c for c in range(cols.shape[0])]
                arr = (U64P * len(addrs))(*[C.cast(C.c_void_p(a), U64P) for a in addrs])
                keep.append((cols, arr))
                tabs.append(arr)
                logs.append(n.bit_length() - 1)
            ptrs = (C.POINTER(U64P) * len(tabs))(*[C.cast(a, C.POINTER(U64P)) for a in tabs])
            logs = (C.c_uint32 * len(logs))(*logs)
            rc = self.lib.ola_prove_with_traces_cols(self.ctx, _p(blob), blob.size, ptrs, logs, None if pr is None else _p(pr),
                                                     None if cc is None else _p(cc), buf, cap, C.byref(need))
        else:
            tr = [t if hasattr(t, "data_ptr") else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
            for t in tr:
                if hasattr(t, "data_ptr") and not (t.is_contiguous() and t.element_size() == 8):
                    raise ValueError("device-resident tables must be contiguous 64-bit tensors")
            ptrs = (U64P * len(tr))(*[C.cast(C.c_void_p(t.data_ptr()), U64P) if hasattr(t, "data_ptr") else _p(t) for t in tr])
            logs = (C.c_uint32 * len(tr))(*[int(t.shape[1]).bit_length() - 1 for t in tr])
            rc = self.lib.ola_prove_with_traces(self.ctx, _p(blob), blob.size, ptrs, logs, None if pr is None else _p(pr),
                                                None if cc is None else _p(cc), buf, cap, C.byref(need))
        if rc != 0 and need.value > cap:            # the proof is kept in the context: fetch it, do not prove again
            buf = C.create_string_buffer(need.value)
            rc = self.lib.ola_take_pending_proof(self.ctx, buf, need.value, C.byref(need))
        self._chk(rc)
        return bytes(buf.raw[:need.value])

    @staticmethod
    def _column_pointers(traces, mask):
        """per-column pointers of the tables of `mask` (numpy tables, contiguous device tensors or lists of columns), NULL for the
        others -> (what must stay alive, cols, log_n) as ola_check_constraints / ola_check_lookup take them"""
        nt = len(traces)
        keep, tabs, logs = [], [], []
        for i, t in enumerate(traces):
            if t is None or not (mask >> i & 1):
                tabs.append(None)
                logs.append(0)
                continue
            if isinstance(t, (list, tuple)):
                cols = [c if hasattr(c, "data_ptr") else np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in t]
                n = int(cols[0].numel()) if hasattr(cols[0], "data_ptr") else cols[0].size
                addrs = [c.data_ptr() if hasattr(c, "data_ptr") else c.ctypes.data for c in cols]
            elif hasattr(t, "data_ptr"):
                if not (t.is_contiguous() and t.element_size() == 8):
                    raise ValueError("device-resident tables must be contiguous 64-bit tensors")
                cols, n = t, int(t.shape[1])
                addrs = [t.data_ptr() + 8 * n * c for c in range(int(t.shape[0]))]
            else:
                cols = np.ascontiguousarray(t, dtype=np.uint64)
                n = cols.shape[1]
                addrs = [cols.ctypes.data + 8 * n * c for c in range(cols.shape[0])]
            arr = (U64P * len(addrs))(*[C.cast(C.c_void_p(a), U64P) for a in addrs])
            keep.append((cols, arr))
            tabs.append(arr)
            logs.append(n.bit_length() - 1)
        ptrs = (C.POINTER(U64P) * nt)(*[C.cast(a, C.POINTER(U64P)) if a is not None else C.POINTER(U64P)() for a in tabs])
        logs = (C.c_uint32 * nt)(*logs)
        return keep, ptrs, logs

    def check_constraints_raw(self, airset_blob, traces, params=None, tables=None, ctl_challenges=None, cap=256):
        """ola_check_constraints as it is: -> (the first min(cap, total) entries as OlaConstraintFailure tuples
        (table, section, index, kind, first_row, rows_failing), total number of entries)."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        nt = len(traces)
        mask = 0
        for t in (range(nt) if tables is None else tables):
            if int(t) < 0:
                raise ValueError("negative table index")
            mask |= 1 << int(t)
        if mask >> 32:
            raise OlaGpuError(-1, "invalid argument: table_mask names a table beyond the AIR set")
        pr = None if params is None or len(params) == 0 else np.ascontiguousarray(params, dtype=np.uint64)
        cc = None if ctl_challenges is None else np.ascontiguousarray(np.array(ctl_challenges, dtype=np.uint64).reshape(-1))
        keep, ptrs, logs = self._column_pointers(traces, mask)
        n_out = C.c_uint32(0)
        out = (OlaConstraintFailure * max(1, cap))()
        self._chk(self.lib.ola_check_constraints(self.ctx, _p(blob), blob.size, ptrs, logs, None if pr is None else _p(pr),
                                                 None if cc is None else _p(cc), mask, out, cap, C.byref(n_out)))
        got = [(int(f.table), int(f.section), int(f.index), int(f.kind), int(f.first_row), int(f.rows_failing)) for f in out[:min(cap, n_out.value)]]
        return got, int(n_out.value)

    def check_constraints(self, airset, traces, params=None, tables=None, ctl_challenges=None):
        """Why a trace does not prove (ola_check_constraints): the constraint programs, permutation arguments and cross-table
        lookups of `tables` (indices; default all) evaluated on the trace domain.  airset: an olavm_amd.air.AirSet (its table
        names go into the report) or a blob; traces: as for prove_with_traces, a table may also be a list of 1-d device tensors
        (entries outside `tables` may be None).
        -> list of dicts {table, table_name, section, index, kind, first_row, rows_failing}, sorted by (table, section, index):
        section "AIR" (index = ordinal of the emit in AirTable.emits, kind = its ConstraintConsumer method), "PERMUTATION"
        (index = batch) or "LOOKUP" (index = the lookup, kind = the challenge index, and first_row / rows_failing are also given
        as looking_rows / looked_rows).  Empty for a trace that satisfies everything."""
        names = [t.name for t in airset.tables] if hasattr(airset, "tables") else None
        blob = airset.blob() if hasattr(airset, "blob") else airset
        got, total = self.check_constraints_raw(blob, traces, params, tables, ctl_challenges)
        if total > len(got):
            got, total = self.check_constraints_raw(blob, traces, params, tables, ctl_challenges, cap=total)
        report = []
        for table, sec, index, kind, first_row, rows_failing in got:
            section = CHECK_SECTIONS[sec]
            d = {"table": table, "table_name": names[table] if names else None, "section": section, "index": index,
                 "kind": CONSTRAINT_KINDS[kind] if section == "AIR" else kind, "first_row": first_row, "rows_failing": rows_failing}
            if section == "LOOKUP":
                d["looking_rows"], d["looked_rows"] = first_row, rows_failing
            report.append(d)
        return report

    def check_lookup_raw(self, airset_blob, traces, lookup, cap=256, tables=None):
        """ola_check_lookup as it is -> (the first min(cap, total) entries as tuples (looking_count, looked_count, looking_entry,
        looking_table, looking_row, looked_row, values[:width]) with None where the C struct says "none", total number of
        mismatching tuples, totals[4], width).  tables: the tables to pass pointers for (default: every table that is not None)."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        mask = 0
        for t in (range(len(traces)) if tables is None else tables):
            mask |= 1 << int(t)
        keep, ptrs, logs = self._column_pointers(traces, mask)
        n_out, width = C.c_uint32(0), C.c_uint32(0)
        totals = (C.c_uint64 * 4)()
        out = (OlaLookupMismatch * max(1, cap))()
        self._chk(self.lib.ola_check_lookup(self.ctx, _p(blob), blob.size, ptrs, logs, int(lookup), out if cap else None, cap, C.byref(n_out),
                                            totals, C.byref(width)))
        none32, none64 = (1 << 32) - 1, (1 << 64) - 1
        opt = lambda v, none: None if int(v) == none else int(v)
        got = [(int(m.looking_count), int(m.looked_count), opt(m.looking_entry, none32), opt(m.looking_table, none32), opt(m.looking_row, none64),
                opt(m.looked_row, none64), tuple(int(v) for v in m.values[:width.value])) for m in out[:min(cap, n_out.value)]]
        return got, int(n_out.value), [int(x) for x in totals], int(width.value)

    def check_lookup(self, airset, traces, lookup, max_tuples=None):
        """Which tuples a cross-table lookup is missing (ola_check_lookup): the exact multiset difference of the filter-selected,
        column-projected rows of its looking side and its looked side.  airset: an olavm_amd.air.AirSet (its names go into the
        report) or a blob; traces: as for check_constraints, tables the lookup does not name may be None; lookup: the `index`
        of a "LOOKUP" entry of check_constraints.  max_tuples: report at most that many (default: all).
        -> {"lookup", "width", "totals": [selected looking rows, selected looked rows, mismatching tuples, unmatched rows], "looked_table", "looked_table_name", "columns",
            "mismatches": [{values, looking_count, looked_count, looking_entry, looking_table, looking_table_name, looking_row,
            looked_row}, ...]} sorted by `values`; "columns" describes the looked side's data columns where the AIR set is given."""
        names = [t.name for t in airset.tables] if hasattr(airset, "tables") else None
        blob = airset.blob() if hasattr(airset, "blob") else airset
        cap = 256 if max_tuples is None else int(max_tuples)
        got, total, totals, width = self.check_lookup_raw(blob, traces, lookup, cap=cap)
        if max_tuples is None and total > len(got):
            got, total, totals, width = self.check_lookup_raw(blob, traces, lookup, cap=total)
        rep = {"lookup": int(lookup), "width": width,
               "totals": totals,
               "looked_table": None, "looked_table_name": None, "columns": None, "mismatches": []}
        if hasattr(airset, "ctls"):
            looked = airset.ctls[lookup].looked_table
            rep["looked_table"], rep["looked_table_name"] = looked.table, names[looked.table]
            rep["columns"] = [describe_column(c) for c in looked.columns]
        for lk, ld, entry, table, lrow, drow, values in got:
            rep["mismatches"].append({"values": values, "looking_count": lk, "looked_count": ld, "looking_entry": entry, "looking_table": table,
                                      "looking_table_name": names[table] if names and table is not None else None, "looking_row": lrow,
                                      "looked_row": drow})
        return rep

    def verify_all_proof(self, airset_blob, proof, params=None):
        """ola_verify_all_proof: the reference's `verify_proof` of AllProof bytes under this context's configuration -> VerifyResult.
        params: the per-table constraint parameters as for prove_with_traces; None takes them from the proof's compress challenges,
        as the reference's verifier does.  A rejected proof is a result, not an error."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        pr = None if params is None or len(params) == 0 else np.ascontiguousarray(params, dtype=np.uint64)
        proof = bytes(proof)
        rep = OlaVerifyReport()
        self._chk(self.lib.ola_verify_all_proof(self.ctx, _p(blob), blob.size, None if pr is None else _p(pr), proof, len(proof), C.byref(rep)))
        return VerifyResult(rep)

    def verify_opening(self, caps, num_polys, degree_bits, num_permutation_zs, proof, challenger):
        """ola_verify_opening, the counterpart of open_and_prove: caps = the three commitments' caps (3 x 2^cap_height x 4), num_polys
        their widths, proof = opening-set bytes + FRI-proof bytes, challenger = the transcript where the prover's stood before
        open_and_prove (a Challenger; advanced to where the prover's stands afterwards when the proof is accepted) -> VerifyResult"""
        cp = np.ascontiguousarray(caps, dtype=np.uint64).reshape(-1)
        if cp.size != 3 * 4 << self.cap_height:
            raise OlaGpuError(-1, "invalid argument: caps must be 3 x 2^cap_height digests")
        proof = bytes(proof)
        rep = OlaVerifyReport()
        self._chk(self.lib.ola_verify_opening(self.ctx, _p(cp), (C.c_uint32 * 3)(*[int(x) for x in num_polys]), int(degree_bits),
                                              int(num_permutation_zs), proof, len(proof), C.byref(challenger.c), C.byref(rep)))
        return VerifyResult(rep)

    def prove_single_table(self, airset_blob, table, trace, batch, ctl_challenges, params, challenger):
        """StarkProof bytes of one table (ola_prove_single_table): `batch` is the table's trace commitment, `challenger` the
        shared transcript (a Challenger, advanced in place), ctl_challenges = [(beta, gamma)] * num_challenges."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        tr = np.ascontiguousarray(trace, dtype=np.uint64)
        ptrs = (U64P * tr.shape[0])(*[_p(tr[c]) for c in range(tr.shape[0])])
        cc = np.ascontiguousarray(np.array(ctl_challenges, dtype=np.uint64).reshape(-1))
        cap_words = np.ascontiguousarray(batch.cap(), dtype=np.uint64).reshape(-1)
        pr = None if params is None or len(params) == 0 else np.ascontiguousarray(params, dtype=np.uint64)
        need = C.c_size_t(0)
        cap = 8 << 20          # larger than any proof of the supported sizes: a too-small buffer costs a second full proof
        while True:
            buf = C.create_string_buffer(cap)
            rc = self.lib.ola_prove_single_table(self.ctx, _p(blob), blob.size, table, ptrs, batch.h, _p(cap_words), _p(cc),
                                                 None if pr is None else _p(pr), C.byref(challenger.c), buf, cap, C.byref(need))
            if rc != 0 and need.value > cap:
                cap = need.value
                continue
            self._chk(rc)
            return bytes(buf.raw[:need.value])

    def air_kernels_available(self, airset_blob, ntables):
        """-> list of bool: which tables of the AIR set have a specialised quotient kernel in this build, at this context's
        num_challenges (ola_air_kernels_available_cfg)."""
        blob = np.ascontiguousarray(airset_blob, dtype=np.uint64)
        flags = (C.c_uint8 * ntables)()
        self._chk(self.lib.ola_air_kernels_available_cfg(C.byref(self._cfg), _p(blob), blob.size, flags, ntables))
        return [bool(x) for x in flags]

    def open(self, trace, zs, quot, num_permutation_zs, zeta):
        """ola_open: StarkOpeningSet::new at `zeta` = (a, b) -> (opening-set bytes in wire format, FriSteps for the rest of the opening proof)"""
        z = np.ascontiguousarray(zeta, dtype=np.uint64)
        need, h = C.c_size_t(0), C.c_void_p()
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            rc = self.lib.ola_open(self.ctx, trace.h, zs.h, quot.h, num_permutation_zs, _p(z), buf, cap, C.byref(need), C.byref(h))
            if rc != 0 and need.value > cap:
                cap = need.value
                continue
            self._chk(rc)
            return bytes(buf.raw[:need.value]), FriSteps(self, h)

    def open_and_prove(self, trace, zs, quot, num_permutation_zs, challenger):
        need, olen = C.c_size_t(0), C.c_size_t(0)
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            rc = self.lib.ola_open_and_prove(self.ctx, trace.h, zs.h, quot.h, num_permutation_zs, C.byref(challenger.c), buf, cap,
                                             C.byref(need), C.byref(olen))
            if rc != 0 and need.value > cap:
                cap = need.value
                continue
            self._chk(rc)
            return bytes(buf.raw[:olen.value]), bytes(buf.raw[olen.value:need.value])
