//! Raw bindings of `libola_gpu.so` (`include/ola_gpu.h`, ABI revision 6) for the reference's `circuits` crate.
//!
//! Drop into `circuits/src/stark/ola_gpu_sys.rs` (integration/patches/0001-feature-hip.patch adds the `mod` line and the
//! feature).  Replaces the reference's dead CUDA FFI -- `gpu_init` / `gpu_method` / `gpu_free`,
//! `plonky2/field/src/cfft/ntt/mod.rs:21-45` -- with the wider boundary: one call per proof, per table or per `timed!` scope.
//! `GoldilocksField` is `#[repr(transparent)] u64` (`plonky2/field/src/goldilocks_field.rs:24-26`) and `HashOut` is `[F; 4]`
//! (`hash/hash_types.rs:19-21`), so `Vec<F>` / `MerkleCap` cross as plain `*const u64`.
//!
//! This file is checked mechanically against the header (tests/test_rust_shim.py: every export, its arity and the width /
//! constness of every argument); no Rust toolchain exists in the build image, so it has not been compiled there.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_void};

pub const OLA_GPU_ABI_VERSION: i32 = 7;
pub const OLA_MAX_CHALLENGES: u32 = 8;
pub const OLA_OK: i32 = 0;
pub const OLA_E_INVALID_ARG: i32 = -1;
pub const OLA_E_NO_DEVICE: i32 = -2;
pub const OLA_E_OOM: i32 = -3;
/// prover.rs:469-473 "vanishing polynomial is not divisible by Z_H"
pub const OLA_E_QUOTIENT_DEGREE: i32 = -4;
pub const OLA_E_HIP: i32 = -5;
/// prover.rs:508-511
pub const OLA_E_ZETA_IN_SUBGROUP: i32 = -6;
pub const OLA_E_INTERNAL: i32 = -7;
/// PoseidonGoldilocksConfig (plonk/config.rs:112-121)
pub const OLA_HASH_POSEIDON: u32 = 0;
/// Blake3GoldilocksConfig (plonk/config.rs:153-161)
pub const OLA_HASH_BLAKE3: u32 = 1;
/// Poseidon2GoldilocksConfig (plonk/config.rs:123-131): Poseidon2 trees, transcript and proof of work
pub const OLA_HASH_POSEIDON2: u32 = 2;
/// Poseidon2GoldilocksConfig2 (plonk/config.rs:133-141): Poseidon2 trees and transcript, Poseidon proof of work
pub const OLA_HASH_POSEIDON2_POW_POSEIDON: u32 = 3;
/// KeccakGoldilocksConfig (plonk/config.rs:145-151): Keccak-256 trees and transcript (25-byte digests), Poseidon proof of work; 4 is unassigned
pub const OLA_HASH_KECCAK: u32 = 5;
/// FriReductionStrategy::ConstantArityBits (fri/reduction_strategies.rs:18): the numbers of OlaGpuConfig, the default
pub const OLA_FRI_CONSTANT_ARITY_BITS: u32 = 0;
/// FriReductionStrategy::Fixed (fri/reduction_strategies.rs:9): the layers' arity bits
pub const OLA_FRI_FIXED: u32 = 1;
/// FriReductionStrategy::MinSize (fri/reduction_strategies.rs:24): no argument = None, one = Some(max_arity_bits)
pub const OLA_FRI_MIN_SIZE: u32 = 2;
pub const OLA_NTT_EVALUATE: i32 = 0;
pub const OLA_NTT_INTERPOLATE: i32 = 1;
pub const OLA_NTT_COSET_LDE: i32 = 2;
pub const OLA_NTT_COSET_INTERPOLATE: i32 = 3;
pub const OLA_NTT_COSET_LDE_LEAF_ORDER: i32 = 4;
pub const OLA_SHARD_STREAM_ORDERED: u32 = 1;
/// ola_gpu_collective: who carries a multi-device context's exchanges
pub const OLA_COLLECTIVE_NONE: u32 = 0;
pub const OLA_COLLECTIVE_PEER: u32 = 1;
pub const OLA_COLLECTIVE_RCCL: u32 = 2;
pub const OLA_PHASE_COUNT: u32 = 7;
/// ola_gpu_warmup: also pin the trace upload's staging ring
pub const OLA_WARMUP_PINNED_RING: u32 = 1;
/// `flags` of `ola_generate_bitwise_trace`: leave the three limb-3 columns zero, as the reference's generator does.
pub const OLA_TABLEGEN_REFERENCE_QUIRKS: u32 = 1;
/// Words of one step record of `ola_generate_cpu_trace` / `ola_generate_prog_trace_steps` (CPU columns 1 .. 65, filter_tape_looking).
pub const OLA_CPU_STEP_WORDS: usize = 66;
/// Words of one memory cell of `ola_generate_memory_trace` (address, clock, the op's one-hot word, value, is_write).
pub const OLA_MEM_CELL_WORDS: usize = 5;
/// Words of one access record of `ola_generate_storage_trace` (key[4], value[4], pre_value[4], flags, psdn_row) and its flag bits.
pub const OLA_STORAGE_ACCESS_WORDS: usize = 14;
pub const OLA_STORAGE_WRITE: u64 = 1;
pub const OLA_STORAGE_FOR_PROG: u64 = 2;
pub const OLA_STORAGE_SILENT: u64 = 4;
/// Words of one tape cell of `ola_generate_tape_trace` (tape address, the opcode's one-hot word, value) and of one POSEIDON call record
/// of `ola_generate_poseidon_chunk_trace` (clk, src, len, dst, psdn_row); `flags` of `ola_generate_prog_chunk_trace`.
pub const OLA_TAPE_CELL_WORDS: usize = 3;
pub const OLA_POSEIDON_CALL_WORDS: usize = 5;
pub const OLA_PROG_CHUNK_RESULT_LINE: u32 = 1;
/// `OlaExecRecords::flags`
pub const OLA_RECORDS_REFERENCE_QUIRKS: u32 = 1;
pub const OLA_RECORDS_ZERO_FILLER: u32 = 2;
pub const OLA_RECORDS_RESULT_LINE: u32 = 4;
pub const OLA_RECORDS_EXPLICIT_BETAS: u32 = 8;
/// `flags` of `ola_generate_prog_trace_steps`: zero rows beyond the executed ones, as the reference's generator leaves them.
pub const OLA_TABLEGEN_ZERO_FILLER: u32 = 1;
/// ola_check_constraints: `OlaConstraintFailure::section`
pub const OLA_CHECK_AIR: u32 = 0;
pub const OLA_CHECK_PERMUTATION: u32 = 1;
pub const OLA_CHECK_LOOKUP: u32 = 2;
/// ... and `kind` of an AIR entry: the ConstraintConsumer method of the emit
pub const OLA_CONSTRAINT_ALL: u32 = 0;
pub const OLA_CONSTRAINT_TRANSITION: u32 = 1;
pub const OLA_CONSTRAINT_FIRST_ROW: u32 = 2;
pub const OLA_CONSTRAINT_LAST_ROW: u32 = 3;

#[repr(C)]
pub struct OlaCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct OlaTableSet {
    _p: [u8; 0],
}
/// What the executor recorded (`ola_tables_from_records`, `ola_prove_from_records`): every pointer host or device memory, NULL where
/// its count is 0; `size` = `size_of::<OlaExecRecords>()`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct OlaExecRecords {
    pub size: u32,
    pub flags: u32,
    pub cpu_log_n: u32,
    pub prog_log_n: u32,
    pub range_bits: u32,
    pub limb_bits: u32,
    pub steps: *const u64,
    pub n_steps: u64,
    pub prog_listing: *const u64,
    pub mem_cells: *const u64,
    pub n_mem_cells: u64,
    pub cmp_ops: *const u64,
    pub n_cmp_ops: u64,
    pub cpu_rc: *const u64,
    pub n_cpu_rc: u64,
    pub bitwise_ops: *const u64,
    pub n_bitwise_ops: u64,
    pub accesses: *const u64,
    pub n_access: u64,
    pub siblings: *const u64,
    pub psdn_inputs: *const u64,
    pub psdn_filters: *const u64,
    pub psdn_stride: u64,
    pub psdn_rows: u64,
    pub tape_cells: *const u64,
    pub n_tape_cells: u64,
    pub psdn_calls: *const u64,
    pub n_psdn_calls: u64,
    pub listing_words: *const u64,
    pub n_listing_words: u64,
    pub code_addr: [u64; 4],
    pub bitwise_beta: u64,
    pub program_beta: u64,
}
#[repr(C)]
pub struct OlaBatch {
    _p: [u8; 0],
}
/// one table's opening proof between the steps of `ola_open` / `ola_fri_*`
#[repr(C)]
pub struct OlaFri {
    _p: [u8; 0],
}
/// `StarkConfig::standard_fast_config()` (circuits/src/stark/config.rs:18-30) + device selection + the hash configuration.
/// Zero-initialise, then fill: `hasher` sits where the struct's tail padding used to be.
#[repr(C)]
pub struct OlaGpuConfig {
    pub device: i32,
    pub stream: *mut c_void,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub proof_of_work_bits: u32,
    pub fri_arity_bits: u32,
    pub fri_final_poly_bits: u32,
    pub num_query_rounds: u32,
    pub num_challenges: u32,
    pub hasher: u32,
}
/// The fields of `plonky2::iop::challenger::Challenger` (iop/challenger.rs:19-24), lengths <= SPONGE_RATE = 8.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct OlaChallenger {
    pub sponge_state: [u64; 12],
    pub input_buffer: [u64; 8],
    pub output_buffer: [u64; 8],
    pub input_len: u32,
    pub output_len: u32,
    pub hasher: u32,
    pub reserved: u32,
}
/// One `timed!` scope of the last proof with device times (`ola_gpu_scope_times`), for the caller's `TimingTree`
/// (plonky2/plonky2/src/util/timing.rs:7-194).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct OlaScopeTime {
    pub name: [c_char; 64],
    pub depth: u32,
    pub ref_depth: u32,
    pub table: i32,
    pub is_reference_scope: u32,
    pub start_ms: f64,
    pub ms: f64,
    pub sharded_ms: f64,
}
/// The launches of one transform-pass kernel instantiation, summed (`ola_gpu_ntt_pass_times`).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct OlaPassTime {
    pub kernel: [c_char; 48],
    pub launches: u32,
    pub reserved: u32,
    pub total_ms: f64,
    pub elements: f64,
}
/// One failing constraint, permutation batch or cross-table lookup (`ola_check_constraints`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct OlaConstraintFailure {
    pub table: u32,
    pub section: u32,
    pub index: u32,
    pub kind: u32,
    pub first_row: u64,
    pub rows_failing: u64,
}
/// `ola_check_lookup`: the widest lookup of the 12-table OlaStark (`OLA_LOOKUP_MAX_VALUES` of ola_gpu.h)
pub const OLA_LOOKUP_MAX_VALUES: usize = 24;
/// One tuple that the two sides of a cross-table lookup carry unequally often (`ola_check_lookup`); `u32::MAX` / `u64::MAX` = none.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct OlaLookupMismatch {
    pub looking_count: u64,
    pub looked_count: u64,
    pub looking_entry: u32,
    pub looking_table: u32,
    pub looking_row: u64,
    pub looked_row: u64,
    pub values: [u64; OLA_LOOKUP_MAX_VALUES],
}
/// `OlaVerifyReport.reason` (`OLA_VERIFY_*` of ola_gpu.h): where the reference's `verify_proof` stops
pub const OLA_VERIFY_OK: u32 = 0;
pub const OLA_VERIFY_MALFORMED: u32 = 1;
pub const OLA_VERIFY_EMPTY_FRI: u32 = 2;
pub const OLA_VERIFY_SHAPE_OPENING_WIDTH: u32 = 3;
pub const OLA_VERIFY_SHAPE_ZS_WIDTH: u32 = 4;
pub const OLA_VERIFY_SHAPE_CTL_ZS_LAST_WIDTH: u32 = 5;
pub const OLA_VERIFY_SHAPE_QUOTIENT_WIDTH: u32 = 6;
pub const OLA_VERIFY_QUOTIENT_IDENTITY: u32 = 7;
pub const OLA_VERIFY_SHAPE_CAP_HEIGHT: u32 = 8;
pub const OLA_VERIFY_SHAPE_QUERY_ROUNDS: u32 = 9;
pub const OLA_VERIFY_SHAPE_INITIAL_PROOFS: u32 = 10;
pub const OLA_VERIFY_SHAPE_LEAF_LEN: u32 = 11;
pub const OLA_VERIFY_SHAPE_INITIAL_PATH_LEN: u32 = 12;
pub const OLA_VERIFY_SHAPE_STEPS: u32 = 13;
pub const OLA_VERIFY_SHAPE_EVALS_LEN: u32 = 14;
pub const OLA_VERIFY_SHAPE_STEP_PATH_LEN: u32 = 15;
pub const OLA_VERIFY_SHAPE_FINAL_POLY_LEN: u32 = 16;
pub const OLA_VERIFY_POW: u32 = 17;
pub const OLA_VERIFY_MERKLE_INITIAL: u32 = 18;
pub const OLA_VERIFY_FRI_CONSISTENCY: u32 = 19;
pub const OLA_VERIFY_MERKLE_COMMIT: u32 = 20;
pub const OLA_VERIFY_FINAL_POLY: u32 = 21;
pub const OLA_VERIFY_CTL: u32 = 22;
/// The verdict of `ola_verify_all_proof` / `ola_verify_opening`: `accepted`, and for a refusal the reason and the table, query and
/// oracle-or-layer (-1 where they do not apply) at which the reference's verifier stops; `message` starts with the reason in words.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct OlaVerifyReport {
    pub accepted: u32,
    pub reason: u32,
    pub table: i32,
    pub query: i32,
    pub oracle_or_layer: i32,
    pub merkle_jobs: u32,
    pub query_jobs: u32,
    pub kernel_launches: u32,
    pub host_ms: f64,
    pub device_ms: f64,
    pub message: [c_char; 96],
}
/// `ola_all_gather_fn`: gather `bytes` bytes of device memory from every rank into `recv_dev` (rank order), 0 = done
pub type OlaAllGatherFn = Option<unsafe extern "C" fn(user: *mut c_void, send_dev: *const c_void, recv_dev: *mut c_void, bytes: usize) -> i32>;

#[link(name = "ola_gpu")]
extern "C" {
    pub fn ola_gpu_init(cfg: *const OlaGpuConfig, out_ctx: *mut *mut OlaCtx) -> i32;
    pub fn ola_gpu_abi_version(challenger_size: *mut usize, config_size: *mut usize) -> i32;
    pub fn ola_gpu_init_multi(cfg: *const OlaGpuConfig, devices: *const i32, n_devices: u32, out_ctx: *mut *mut OlaCtx) -> i32;
    pub fn ola_gpu_device_count(ctx: *mut OlaCtx, n_devices: *mut u32) -> i32;
    pub fn ola_gpu_collective(ctx: *mut OlaCtx, carrier: *mut u32, ranks: *mut u32, note: *mut c_char, note_cap: usize) -> i32;
    pub fn ola_gpu_all_gather_check(ctx: *mut OlaCtx, carrier: u32, bytes_per_rank: usize, reps: u32, ms_per_gather: *mut f64,
        mismatches: *mut u64) -> i32;
    pub fn ola_gpu_free(ctx: *mut OlaCtx) -> i32;
    pub fn ola_gpu_warmup(device: i32, flags: u32, airset: *const u64, airset_words: usize) -> i32;
    pub fn ola_gpu_warmup_wait(ms_out: *mut f64) -> i32;
    pub fn ola_gpu_last_error() -> *const c_char;
    pub fn ola_gpu_sync(ctx: *mut OlaCtx) -> i32;
    pub fn ola_gpu_trim(ctx: *mut OlaCtx) -> i32;
    pub fn ola_gpu_memory_stats(ctx: *mut OlaCtx, out: *mut u64, reset: i32) -> i32;
    pub fn ola_gpu_proof_stats(ctx: *mut OlaCtx, enable: i32, out: *mut f64) -> i32;
    pub fn ola_gpu_phase_stats(ctx: *mut OlaCtx, out: *mut f64, n_phases: u32) -> i32;
    pub fn ola_gpu_scope_times(ctx: *mut OlaCtx, enable: i32, out: *mut OlaScopeTime, cap: u32, n_out: *mut u32) -> i32;
    pub fn ola_gpu_upload_stats(ctx: *mut OlaCtx, out: *mut f64) -> i32;
    pub fn ola_gpu_ntt_pass_times(ctx: *mut OlaCtx, enable: i32, out: *mut OlaPassTime, cap: u32, n_out: *mut u32) -> i32;
    pub fn ola_gpu_selftest(ctx: *mut OlaCtx, pairs: u64, mismatches: *mut u64) -> i32;
    pub fn ola_gpu_reserve(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, log_n: *const u32) -> i32;
    pub fn ola_table_shape(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, table: u32, out: *mut u32) -> i32;
    pub fn ola_perm_z(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, table: u32, log_n: u32,
        trace_cols: *const *const u64, perm_challenges: *const u64, z_out: *mut u64) -> i32;
    pub fn ola_ctl_z(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, table: u32, log_n: u32,
        trace_cols: *const *const u64, ctl_challenges: *const u64, z_out: *mut u64) -> i32;
    pub fn ola_quotient(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, table: u32, trace: *const OlaBatch,
        zs: *const OlaBatch, perm_challenges: *const u64, ctl_challenges: *const u64, alphas: *const u64,
        params: *const u64, chunks_out: *mut u64) -> i32;
    pub fn ola_ntt_batch(ctx: *mut OlaCtx, op: i32, input: *const u64, out: *mut u64, log_n: u32, batch: u32, shift: u64,
        blowup_log: u32) -> i32;
    pub fn ola_ntt_batch_dev(ctx: *mut OlaCtx, op: i32, in_dev: *const u64, out_dev: *mut u64, scratch_dev: *mut u64,
        log_n: u32, batch: u32, shift: u64, blowup_log: u32) -> i32;
    pub fn ola_poseidon_permute(ctx: *mut OlaCtx, states: *mut u64, n: usize) -> i32;
    pub fn ola_poseidon2_permute(ctx: *mut OlaCtx, states: *mut u64, n: usize) -> i32;
    pub fn ola_hash_rows(ctx: *mut OlaCtx, rows: *const u64, num_rows: usize, row_len: usize, digests: *mut u64) -> i32;
    pub fn ola_merkle_cap(ctx: *mut OlaCtx, leaves: *const u64, num_leaves: usize, leaf_len: usize, cap_height: u32,
        cap_out: *mut u64) -> i32;
    pub fn ola_commit_values(ctx: *mut OlaCtx, cols: *const *const u64, ncols: u32, log_n: u32,
        out_batch: *mut *mut OlaBatch, cap_out: *mut u64) -> i32;
    pub fn ola_commit_coeffs(ctx: *mut OlaCtx, cols: *const *const u64, ncols: u32, log_n: u32,
        out_batch: *mut *mut OlaBatch, cap_out: *mut u64) -> i32;
    pub fn ola_commit_values_dev(ctx: *mut OlaCtx, cols_dev: *const u64, ncols: u32, log_n: u32,
        out_batch: *mut *mut OlaBatch, cap_out: *mut u64) -> i32;
    pub fn ola_commit_coeffs_dev(ctx: *mut OlaCtx, cols_dev: *const u64, ncols: u32, log_n: u32,
        out_batch: *mut *mut OlaBatch, cap_out: *mut u64) -> i32;
    pub fn ola_commit_values_shard(ctx: *mut OlaCtx, cols: *const *const u64, ncols: u32, log_n: u32, rank: u32,
        world: u32, out_batch: *mut *mut OlaBatch, cap_slice_out: *mut u64) -> i32;
    pub fn ola_commit_values_shard_dev(ctx: *mut OlaCtx, cols_dev: *const u64, ncols: u32, log_n: u32, rank: u32,
        world: u32, out_batch: *mut *mut OlaBatch, cap_slice_out: *mut u64) -> i32;
    pub fn ola_batch_free(ctx: *mut OlaCtx, batch: *mut OlaBatch) -> i32;
    pub fn ola_batch_shape(batch: *const OlaBatch, ncols: *mut u32, log_n: *mut u32, rate_bits: *mut u32) -> i32;
    pub fn ola_batch_get_coeffs(ctx: *mut OlaCtx, batch: *const OlaBatch, out: *mut u64) -> i32;
    pub fn ola_batch_get_leaf(ctx: *mut OlaCtx, batch: *const OlaBatch, leaf_index: usize, row_out: *mut u64,
        siblings_out: *mut u64) -> i32;
    pub fn ola_batch_get_lde_row(ctx: *mut OlaCtx, batch: *const OlaBatch, index: usize, step: usize, row_out: *mut u64) -> i32;
    pub fn ola_challenger_init(ch: *mut OlaChallenger) -> i32;
    pub fn ola_challenger_init_hasher(ch: *mut OlaChallenger, hasher: u32) -> i32;
    pub fn ola_challenger_init_keccak(ch: *mut OlaChallenger) -> i32;
    pub fn ola_challenger_observe_cap(ch: *mut OlaChallenger, digests: *const u64, n: usize) -> i32;
    pub fn ola_blake3_hash_elements(elems: *const u64, n: usize, out: *mut u64) -> i32;
    pub fn ola_keccak_hash_elements(elems: *const u64, n: usize, out: *mut u64) -> i32;
    pub fn ola_challenger_observe(ch: *mut OlaChallenger, elems: *const u64, n: usize) -> i32;
    pub fn ola_challenger_get(ch: *mut OlaChallenger, out: *mut u64, n: usize) -> i32;
    pub fn ola_challenger_compact(ch: *mut OlaChallenger) -> i32;
    pub fn ola_open_and_prove(ctx: *mut OlaCtx, trace: *const OlaBatch, zs: *const OlaBatch, quotient: *const OlaBatch,
        num_permutation_zs: u32, challenger: *mut OlaChallenger, out: *mut u8, cap: usize, out_len: *mut usize,
        openings_len: *mut usize) -> i32;
    pub fn ola_pow(ctx: *mut OlaCtx, h: *const u64, bits: u32, witness: *mut u64) -> i32;
    pub fn ola_open(ctx: *mut OlaCtx, trace: *const OlaBatch, zs: *const OlaBatch, quotient: *const OlaBatch, num_permutation_zs: u32,
        zeta: *const u64, out: *mut u8, cap: usize, out_len: *mut usize, fri_out: *mut *mut OlaFri) -> i32;
    pub fn ola_gpu_set_fri_reduction(ctx: *mut OlaCtx, strategy: u32, args: *const u32, n: u32) -> i32;
    pub fn ola_fri_reduction_arity_bits(cfg: *const OlaGpuConfig, strategy: u32, args: *const u32, n: u32, degree_bits: u32, out: *mut u32, cap: u32, n_out: *mut u32) -> i32;
    pub fn ola_fri_plan(fri: *const OlaFri, arity_bits: *mut u32, cap: u32, n_layers: *mut u32, final_poly_len: *mut u32) -> i32;
    pub fn ola_fri_commit_begin(fri: *mut OlaFri, alpha: *const u64) -> i32;
    pub fn ola_fri_commit_next_layer(fri: *mut OlaFri, beta: *const u64, cap_out: *mut u64) -> i32;
    pub fn ola_fri_commit_finish(fri: *mut OlaFri, beta: *const u64, final_poly_out: *mut u64, cap_elems: usize, n_out: *mut usize) -> i32;
    pub fn ola_fri_query(fri: *mut OlaFri, x_index: *const u64, n: u32, out: *mut u8, cap: usize, out_len: *mut usize) -> i32;
    pub fn ola_fri_free(fri: *mut OlaFri) -> i32;
    pub fn ola_prove_with_traces(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, traces: *const *const u64,
        log_n: *const u32, params: *const u64, compress_challenges: *const u64, out: *mut u8, cap: usize,
        out_len: *mut usize) -> i32;
    pub fn ola_prove_with_traces_cols(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, cols: *const *const *const u64,
        log_n: *const u32, params: *const u64, compress_challenges: *const u64, out: *mut u8, cap: usize,
        out_len: *mut usize) -> i32;
    pub fn ola_check_constraints(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, cols: *const *const *const u64,
        log_n: *const u32, params: *const u64, ctl_challenges: *const u64, table_mask: u32, out: *mut OlaConstraintFailure,
        cap: u32, n_out: *mut u32) -> i32;
    pub fn ola_check_lookup(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, cols: *const *const *const u64,
        log_n: *const u32, lookup: u32, out: *mut OlaLookupMismatch, cap: u32, n_out: *mut u32, totals: *mut u64,
        width: *mut u32) -> i32;
    pub fn ola_verify_all_proof(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, params: *const u64, proof: *const u8,
        proof_len: usize, report: *mut OlaVerifyReport) -> i32;
    pub fn ola_verify_opening(ctx: *mut OlaCtx, caps: *const u64, num_polys: *const u32, degree_bits: u32, num_permutation_zs: u32,
        proof: *const u8, proof_len: usize, challenger: *mut OlaChallenger, report: *mut OlaVerifyReport) -> i32;
    pub fn ola_take_pending_proof(ctx: *mut OlaCtx, out: *mut u8, cap: usize, out_len: *mut usize) -> i32;
    pub fn ola_prove_single_table(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, table: u32,
        trace_cols: *const *const u64, trace_commitment: *const OlaBatch, trace_cap: *const u64,
        ctl_challenges: *const u64, params: *const u64, challenger: *mut OlaChallenger, out: *mut u8, cap: usize,
        out_len: *mut usize) -> i32;
    pub fn ola_generate_poseidon_trace(ctx: *mut OlaCtx, inputs: *const u64, filters: *const u64, n: usize, out: *mut u64) -> i32;
    pub fn ola_permuted_cols(ctx: *mut OlaCtx, inputs: *const u64, table: *const u64, n: usize, permuted_inputs: *mut u64,
        permuted_table: *mut u64) -> i32;
    pub fn ola_permuted_cols_dev(ctx: *mut OlaCtx, inputs_dev: *const u64, table_dev: *const u64, n: usize,
        permuted_inputs_dev: *mut u64, permuted_table_dev: *mut u64) -> i32;
    pub fn ola_generate_rc_trace(ctx: *mut OlaCtx, vals: *const u64, filters: *const u64, n_rows: usize, range_bits: u32,
        out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_generate_bitwise_trace(ctx: *mut OlaCtx, ops: *const u64, n_ops: usize, limb_bits: u32, beta: u64, flags: u32,
        out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_generate_prog_trace(ctx: *mut OlaCtx, exec: *const u64, prog: *const u64, log_n: u32, beta: u64, out: *mut u64) -> i32;
    pub fn ola_generate_cpu_trace(ctx: *mut OlaCtx, steps: *const u64, n_steps: usize, log_n: u32, out: *mut u64) -> i32;
    pub fn ola_generate_prog_trace_steps(ctx: *mut OlaCtx, steps: *const u64, n_steps: usize, prog: *const u64, log_n: u32,
        beta: u64, flags: u32, out: *mut u64, exec_rows_out: *mut u64) -> i32;
    pub fn ola_generate_memory_trace(ctx: *mut OlaCtx, cells: *const u64, n_cells: usize, flags: u32, out: *mut u64,
        log_n_out: *mut u32, rc_out: *mut u64, rc_counts: *mut u64) -> i32;
    pub fn ola_generate_cmp_trace(ctx: *mut OlaCtx, ops: *const u64, n_ops: usize, out: *mut u64, log_n_out: *mut u32,
        abs_diff_out: *mut u64) -> i32;
    pub fn ola_generate_storage_trace(ctx: *mut OlaCtx, accesses: *const u64, n_access: usize, siblings: *const u64, out: *mut u64,
        log_n_out: *mut u32, psdn_inputs: *mut u64, psdn_filters: *mut u64, psdn_stride: usize, roots_out: *mut u64) -> i32;
    pub fn ola_generate_poseidon_table(ctx: *mut OlaCtx, inputs: *const u64, filters: *const u64, n_rows: usize, stride: usize,
        out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_generate_tape_trace(ctx: *mut OlaCtx, cells: *const u64, n_cells: usize, out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_generate_poseidon_chunk_trace(ctx: *mut OlaCtx, calls: *const u64, n_calls: usize, poseidon_table: *const u64,
        psdn_log_n: u32, out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_generate_prog_chunk_trace(ctx: *mut OlaCtx, words: *const u64, n_words: usize, code_addr: *const u64, flags: u32,
        poseidon_table: *const u64, psdn_log_n: u32, out: *mut u64, log_n_out: *mut u32) -> i32;
    pub fn ola_tables_from_records(ctx: *mut OlaCtx, rec: *const OlaExecRecords, out: *mut *mut OlaTableSet) -> i32;
    pub fn ola_tables_get(set: *const OlaTableSet, ptrs: *mut *const u64, log_n: *mut u32, params: *mut u64, compress: *mut u64) -> i32;
    pub fn ola_tables_free(set: *mut OlaTableSet) -> i32;
    pub fn ola_prove_from_records(ctx: *mut OlaCtx, airset: *const u64, airset_words: usize, rec: *const OlaExecRecords, out: *mut u8,
        cap: usize, out_len: *mut usize) -> i32;
    pub fn ola_set_shard(ctx: *mut OlaCtx, rank: u32, world: u32, all_gather: OlaAllGatherFn, user: *mut c_void) -> i32;
    pub fn ola_set_shard_options(ctx: *mut OlaCtx, flags: u32) -> i32;
    pub fn ola_gpu_get_stream(ctx: *mut OlaCtx, stream_out: *mut *mut c_void) -> i32;
    pub fn ola_air_kernels_available(airset: *const u64, airset_words: usize, has_kernel: *mut u8, ntables: usize) -> i32;
    pub fn ola_air_kernels_available_cfg(cfg: *const OlaGpuConfig, airset: *const u64, airset_words: usize, has_kernel: *mut u8,
        ntables: usize) -> i32;
}

/// Non-zero status -> `anyhow::Error` carrying the library's message (the reference's `Result` / `ensure!` sites).
pub fn check(rc: i32) -> anyhow::Result<()> {
    if rc == OLA_OK {
        return Ok(());
    }
    let msg = unsafe { std::ffi::CStr::from_ptr(ola_gpu_last_error()) }.to_string_lossy().into_owned();
    Err(anyhow::anyhow!("ola_gpu error {rc}: {msg}"))
}

/// Refuse a library whose ABI revision or struct sizes differ from this file's (call once at start-up).
pub fn check_abi() -> anyhow::Result<()> {
    let (mut chal, mut cfg) = (0usize, 0usize);
    let rev = unsafe { ola_gpu_abi_version(&mut chal, &mut cfg) };
    anyhow::ensure!(
        rev == OLA_GPU_ABI_VERSION && chal == std::mem::size_of::<OlaChallenger>() && cfg == std::mem::size_of::<OlaGpuConfig>(),
        "libola_gpu.so is ABI revision {rev} (OlaChallenger {chal} bytes, OlaGpuConfig {cfg} bytes); this binding is revision {OLA_GPU_ABI_VERSION}"
    );
    Ok(())
}
