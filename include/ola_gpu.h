/* ola_gpu.h -- C ABI of the MI355X-native Goldilocks STARK proving backend for OlaVM.
 *
 * This is the drop-in boundary behind circuits::stark::prover::prove_with_traces (reference
 * circuits/src/stark/prover.rs:79).  It widens the reference's existing GPU FFI precedent
 *     extern "C" { gpu_init; gpu_method; gpu_free }      plonky2/field/src/cfft/ntt/mod.rs:21-45
 * (one column per call, host<->device round trip per column, global mutex) to whole-phase granularity:
 * a PolynomialBatch is committed in one call and stays resident in HBM.  INTEGRATION.md shows the Rust-side
 * bindings (`extern "C"` block + build.rs link lines) a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int32_t: 0 = OLA_OK, negative = error; ola_gpu_last_error() gives the message of
 *     the last failure on the calling thread.  No exceptions, no abort() cross this boundary
 *     (the reference panics / returns anyhow::Error: prover.rs:352-355,471-473,508-511).
 *   - field elements are uint64_t Goldilocks values (p = 2^64 - 2^32 + 1), GoldilocksField is
 *     #[repr(transparent)] u64 (plonky2/field/src/goldilocks_field.rs:24-26).  Inputs may be non-canonical
 *     (>= p); ALL outputs are canonical (< p), i.e. exactly what the reference serialises
 *     (circuits/src/stark/serialization.rs:50-52).
 *   - "host" pointers are ordinary process memory owned by the caller and are not retained after return.
 *     "_dev" entry points take device (HBM) pointers valid on the context's device; work is enqueued on the
 *     context's stream and the call returns after the stream has been synchronised unless stated otherwise.
 *   - column-major: a table of `ncols` columns of n = 2^log_n rows is ncols contiguous runs of n elements
 *     (the reference's Vec<PolynomialValues<F>>, plonky2/field/src/polynomial/mod.rs:24-26).
 *   - thread-compatible per OlaCtx: one orchestrating thread per context (prove_with_traces is sequential
 *     across tables, prover.rs:160-287).
 */
#ifndef OLA_GPU_H
#define OLA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  3: OlaChallenger carries `hasher` + `reserved` (sizeof 240, was 232 in revision 1) and
 * OlaGpuConfig.hasher occupies what was tail padding (sizeof unchanged, but the field must be set: zero-initialise the struct);
 * multi-device contexts and the accounting entry points were added.  A host built against an older header must be rebuilt:
 * ola_gpu_abi_version() lets it check at start-up that library and header agree (also on sizeof(OlaChallenger)).
 * 5: ola_prove_with_traces_cols (one pointer per column: the reference's [Vec<PolynomialValues<F>>; NUM_TABLES] as it is),
 * ola_gpu_scope_times (the `timed!` scopes with device times, for the caller's TimingTree), ola_gpu_upload_stats; no struct of
 * revision 4 changed.
 * 6: ola_gpu_warmup / ola_gpu_warmup_wait (start-up work ahead of the first context, where the reference calls init_gpu()),
 * ola_gpu_ntt_pass_times (the transform passes one by one, for the dominant kernel's roofline); no struct changed.
 * 7 (number unchanged by the later additions, which change no struct and no existing behaviour): the hashers OLA_HASH_POSEIDON2 and
 * OLA_HASH_POSEIDON2_POW_POSEIDON and the entry point ola_poseidon2_permute were added to revision 7; so were OlaConstraintFailure
 * and the entry point ola_check_constraints (which constraint of which table fails at which row); so were ola_generate_rc_trace,
 * ola_generate_bitwise_trace and ola_generate_prog_trace (the range-check, bitwise and program tables completed in HBM); so were
 * OlaLookupMismatch and the entry point ola_check_lookup (the tuples a failing cross-table lookup is missing); so were
 * ola_generate_cpu_trace and ola_generate_prog_trace_steps (the CPU table and the program table from the executor's step records); so
 * were ola_generate_memory_trace and ola_generate_cmp_trace (the memory table from raw cells, sorted on the device, and the comparison
 * table from operand pairs, both with their range-checked value lists); so were ola_generate_storage_trace and
 * ola_generate_poseidon_table (the account-storage tree hashed on the device with the storage-access table and the Poseidon table's
 * inputs, and the Poseidon table at its padded height, resident); so were ola_generate_tape_trace, ola_generate_poseidon_chunk_trace
 * and ola_generate_prog_chunk_trace (the tape table sorted on the device, and the two chunk tables gathered from the resident Poseidon
 * table); so were OlaExecRecords, ola_tables_from_records, ola_tables_get, ola_tables_free and ola_prove_from_records (the twelve
 * generators composed in one call, from the executor's records to resident tables and to proof bytes); so were OlaVerifyReport, the
 * OLA_VERIFY_* reasons and the entry points ola_verify_all_proof and ola_verify_opening (proof bytes to a verdict with the place and
 * the reason of a refusal); so were the hasher OLA_HASH_KECCAK (KeccakGoldilocksConfig: Keccak-256 trees and challenger, 25-byte
 * digests) and the host entry points ola_keccak_hash_elements and ola_challenger_init_keccak; so were the OLA_FRI_* strategies and
 * the entry points ola_gpu_set_fri_reduction and ola_fri_reduction_arity_bits (FriReductionStrategy::Fixed and MinSize: an arity
 * per FRI layer, in the prover and in the verifier); so were OlaGpuConfig.num_challenges 1..OLA_MAX_CHALLENGES (it had to be 2) and
 * the host entry point ola_air_kernels_available_cfg (the generated kernels of a configuration's challenge count). */
#define OLA_GPU_ABI_VERSION 7
#define OLA_MAX_CHALLENGES 8 /* OlaGpuConfig.num_challenges: 1..8, the range the verifier reads */
#define OLA_OK 0
#define OLA_E_INVALID_ARG (-1)
#define OLA_E_NO_DEVICE (-2)
#define OLA_E_OOM (-3)
#define OLA_E_QUOTIENT_DEGREE (-4) /* prover.rs:469-473 "vanishing polynomial is not divisible by Z_H" */
#define OLA_E_HIP (-5)
#define OLA_E_ZETA_IN_SUBGROUP (-6) /* prover.rs:508-511 */
#define OLA_E_INTERNAL (-7)

typedef struct OlaCtx OlaCtx;     /* device context: streams, twiddle tables, Poseidon constants            */
typedef struct OlaBatch OlaBatch; /* a committed PolynomialBatch resident in HBM (fri/oracle.rs:31-39)      */

/* StarkConfig::standard_fast_config (circuits/src/stark/config.rs:18-30) is the default when NULL is passed. */
typedef struct OlaGpuConfig {
    int32_t device;             /* HIP device ordinal; -1 = current device                                   */
    void* stream;               /* hipStream_t to run on, NULL = the library creates its own                 */
    uint32_t rate_bits;         /* 3                                                                         */
    uint32_t cap_height;        /* 4                                                                         */
    uint32_t proof_of_work_bits;/* 16                                                                        */
    uint32_t fri_arity_bits;    /* ConstantArityBits(4, 5).  1..8 for proving (arities 2 to 256); the verifier supports FRI
                                 * arities of 2 to 16: under 5..8 ola_verify_all_proof and ola_verify_opening return
                                 * OLA_E_INVALID_ARG ("the verifier supports FRI arities of 2 to 16") and the context goes on
                                 * proving.                                                                   */
    uint32_t fri_final_poly_bits;
    uint32_t num_query_rounds;  /* 28                                                                        */
    uint32_t num_challenges;    /* 2.  1..OLA_MAX_CHALLENGES (0 and 9 up: OLA_E_INVALID_ARG): the number of grand-product
                                 * challenge sets, of CTL challenges and of alphas (prover.rs:360-367,425,
                                 * cross_table_lookup.rs:182-188, permutation.rs:265-280), hence of Z columns per lookup side
                                 * and of quotient polynomials.  Every entry point runs at the context's value; 2 and 3 have
                                 * generated quotient kernels for the default table sets, the other counts run the
                                 * interpreter kernel (ola_air_kernels_available_cfg).                          */
    uint32_t hasher;            /* GenericConfig::Hasher of the Merkle trees and the challenger (plonk/config.rs:112-161):
                                 * OLA_HASH_POSEIDON = PoseidonGoldilocksConfig (0, the default),
                                 * OLA_HASH_BLAKE3 = Blake3GoldilocksConfig.  InnerHasher (proof of work) is Poseidon in both.
                                 * OLA_HASH_POSEIDON2 = Poseidon2GoldilocksConfig (plonk/config.rs:125): Merkle trees, challenger
                                 * and proof of work all Poseidon2 (hash/poseidon2.rs:50); OLA_HASH_POSEIDON2_POW_POSEIDON =
                                 * Poseidon2GoldilocksConfig2 (plonk/config.rs:135): Poseidon2 trees and challenger, Poseidon
                                 * proof of work.
                                 * OLA_HASH_KECCAK = KeccakGoldilocksConfig (plonk/config.rs:145): Merkle trees and challenger on
                                 * Keccak-256 truncated to 25 bytes (hash/keccak.rs, KeccakHash<25>), Poseidon proof of work.  A
                                 * digest keeps 4 words in memory (word 3 = byte 24, upper 56 bits zero) and is 25 bytes in a proof.
                                 * The value 4 is unassigned and refused.
                                 * The field takes the place of the struct's tail padding: sizeof is unchanged.             */
} OlaGpuConfig;
#define OLA_HASH_POSEIDON 0u
#define OLA_HASH_BLAKE3 1u
#define OLA_HASH_POSEIDON2 2u
#define OLA_HASH_POSEIDON2_POW_POSEIDON 3u
#define OLA_HASH_KECCAK 5u /* 4 is not a hasher */

/* ---- lifetime (replaces gpu_init / gpu_free, cfft/ntt/mod.rs:89-121 and core/src/storage/db.rs:248) ---- */
/* The configuration is validated before a device is looked for: OLA_E_INVALID_ARG for a value out of range (an unassigned hasher
 * among them) with or without a device, OLA_E_NO_DEVICE for a valid configuration on a machine without one. */
int32_t ola_gpu_init(const OlaGpuConfig* cfg, OlaCtx** out_ctx);
/* OLA_GPU_ABI_VERSION of the library that was loaded; *challenger_size / *config_size (may be NULL) receive its sizeof(OlaChallenger)
 * and sizeof(OlaGpuConfig). */
int32_t ola_gpu_abi_version(size_t* challenger_size, size_t* config_size);

/* ---- FriReductionStrategy (plonky2/plonky2/src/fri/reduction_strategies.rs:7-25): the arity of every FRI layer ----
 * A context starts with ConstantArityBits(cfg.fri_arity_bits, cfg.fri_final_poly_bits).  ola_gpu_set_fri_reduction replaces the
 * strategy for every call that BEGINS after it: ola_prove_with_traces*, ola_prove_single_table, ola_prove_from_records,
 * ola_open_and_prove, ola_open / ola_fri_* (an OlaFri keeps the plan it was opened with), ola_verify_all_proof and
 * ola_verify_opening.  Like the reference, one strategy serves all tables of a proof; the transcript does not see the plan.
 *   OLA_FRI_FIXED      args[0..n) are the layers' arity bits, each in 1..4 (the verifier keeps one coset of a layer in registers),
 *                      n = 0..32; n = 0 is no reduction at all.  A plan whose total exceeds degree_bits + rate_bits - cap_height of
 *                      a table, or its degree_bits, fails the call that proves or verifies that table with OLA_E_INVALID_ARG
 *                      ("FRI total reduction arity is too large.", plonk/circuit_builder.rs:922-925); the context goes on working.
 *   OLA_FRI_MIN_SIZE   n = 0: MinSize(None), n = 1: MinSize(Some(args[0])), args[0] in 1..4: the search of
 *                      fri/reduction_strategies.rs:60-164 for the smallest estimated proof.  Final polynomials grow to 2^9
 *                      coefficients at the default rate and query count.
 * A bad argument is OLA_E_INVALID_ARG and leaves the previous strategy in place.  Multi-device contexts (ola_gpu_init_multi with more
 * than one device) are refused with OLA_E_INVALID_ARG: the coset partition's first layer is measured and tested for arity 16 only.
 * ctx == NULL: OLA_E_NO_DEVICE on a machine without a HIP device, OLA_E_INVALID_ARG otherwise; the other arguments are validated first.
 *
 * ola_fri_reduction_arity_bits is the plan itself, host only (no device, no context): strategy.reduction_arity_bits(degree_bits,
 * cfg.rate_bits, cfg.cap_height, cfg.num_query_rounds) with cfg == NULL meaning the defaults.  out receives min(*n_out, cap) entries,
 * *n_out the plan's length; OLA_E_INVALID_ARG when cap is too small (*n_out is set), for a bad strategy or degree_bits > 32. */
#define OLA_FRI_CONSTANT_ARITY_BITS 0u  /* cfg.fri_arity_bits / cfg.fri_final_poly_bits: the default                          */
#define OLA_FRI_FIXED 1u                /* args[0..n): the layers' arity bits, n = 0 .. 32; n = 0: no reduction               */
#define OLA_FRI_MIN_SIZE 2u             /* n = 0: MinSize(None); n = 1: MinSize(Some(args[0]))                                 */
int32_t ola_gpu_set_fri_reduction(OlaCtx* ctx, uint32_t strategy, const uint32_t* args, uint32_t n);
int32_t ola_fri_reduction_arity_bits(const OlaGpuConfig* cfg, uint32_t strategy, const uint32_t* args, uint32_t n,
                                     uint32_t degree_bits, uint32_t* out, uint32_t cap, uint32_t* n_out);
/* One context that spans n_devices GPUs of the node (1, 2, 4 or 8; devices = HIP ordinals, NULL = 0..n-1): the caller stays the
 * single process the reference's prover is (client/src/main.rs:174-214, one `prove` per process; the reference's own GPU state is
 * process-wide, cfft/ntt/mod.rs:14-17,48-50) and calls ola_prove_with_traces ONCE; inside, rank r is a worker thread on
 * devices[r] with its own stream and buffer pool, the proof runs on the coset partition described under ola_set_shard below, and
 * the exchanges are the library's own all-gather over xGMI (peer-to-peer pulls ordered by events on the ranks' streams, no host
 * synchronisation; olavm_amd/csrc/peer_group.h).  Every other entry point of such a context works on devices[0] as on a
 * single-device context.  Entries of devices[] may repeat (logical ranks sharing a GPU: how the one-GPU test box exercises the
 * path).  cfg->device is ignored, cfg->stream must be NULL when n_devices > 1.  Needs peer access between the devices
 * (OLA_E_HIP otherwise). */
int32_t ola_gpu_init_multi(const OlaGpuConfig* cfg, const int32_t* devices, uint32_t n_devices, OlaCtx** out_ctx);
int32_t ola_gpu_device_count(OlaCtx* ctx, uint32_t* n_devices);
/* Who carries the exchanges of a multi-device context (SURVEY 8(b),(e): "RCCL-over-xGMI all-gather of Merkle caps and FRI
 * commitments").  OLA_COLLECTIVE = peer (default) | rccl, read by ola_gpu_init_multi: with rccl the library dlopen()s librccl.so,
 * creates one communicator per device (ncclCommInitAll over the context's devices) and every exchange is an ncclAllGather on the
 * rank's stream; with peer it is the library's own event-ordered pulls (hipMemcpyPeerAsync).  RCCL is never a link dependency.
 * When RCCL cannot carry the context -- library absent, or logical ranks aliased onto one physical GPU -- the context keeps the
 * peer carrier and `note` says why.  *carrier: OLA_COLLECTIVE_*, *ranks: ranks the carrier spans; note (may be NULL) receives a
 * NUL-terminated explanation (RCCL version when active, the refusal otherwise). */
#define OLA_COLLECTIVE_NONE 0u /* single-device context: no exchanges */
#define OLA_COLLECTIVE_PEER 1u
#define OLA_COLLECTIVE_RCCL 2u
int32_t ola_gpu_collective(OlaCtx* ctx, uint32_t* carrier, uint32_t* ranks, char* note, size_t note_cap);
/* The context's all-gather by itself (what bench.py times for the 512-byte cap exchange and the trace exchange, and what the
 * tests check): every rank contributes bytes_per_rank bytes of its own pattern, `reps` gathers run back to back on the ranks'
 * streams through `carrier` (OLA_COLLECTIVE_PEER / _RCCL; the latter needs a context created under OLA_COLLECTIVE=rccl, also a
 * single-device one: a 1-rank communicator).  *ms_per_gather: slowest rank's mean; *mismatches: wrong bytes over all ranks (0). */
int32_t ola_gpu_all_gather_check(OlaCtx* ctx, uint32_t carrier, size_t bytes_per_rank, uint32_t reps, double* ms_per_gather, uint64_t* mismatches);
int32_t ola_gpu_free(OlaCtx* ctx);
/* Start-up ahead of the first context: replaces the reference's early hook -- OlaStark::default() calls
 * plonky2::field::cfft::ntt::init_gpu() (circuits/src/stark/ola_stark.rs:47, plonky2/field/src/cfft/ntt/mod.rs:53-99) before
 * prove() generates the traces (client/src/main.rs:193-195).  Returns at once; a helper thread starts the HIP runtime, opens
 * `device` (-1: the current one), loads the library's code objects (the main one and one per generated quotient kernel) and, with
 * OLA_WARMUP_PINNED_RING, pins the 128 MB staging ring of the trace upload.  With an AIR set (may be NULL; copied) it also creates
 * a context with the default configuration and PRIMES it: one throw-away proof per hash configuration of an all-zero instance with
 * small tables (divisibility check off, bytes discarded), so that every kernel of the proof path has been launched once, the
 * transform tables exist and the upload path has carried data -- what otherwise makes the first proof of a process 1.2 - 1.4 x a
 * warm one.  None of this depends on the StarkConfig or the hasher, which the caller does not know yet at that point:
 * ola_gpu_init / ola_gpu_init_multi wait for a warm-up that is under way and, when cfg->stream is NULL and the device is the
 * warmed one, take the primed context over (configuration and hasher are set then); otherwise they find at least the runtime up
 * (5 ms instead of 160 ms: the split is printed under OLA_TIMING=1).  Calling it again is a no-op; a failure inside the thread
 * (no device) is reported by the ola_gpu_init that follows, as it would have been without the warm-up. */
#define OLA_WARMUP_PINNED_RING 1u
int32_t ola_gpu_warmup(int32_t device, uint32_t flags, const uint64_t* airset, size_t airset_words);
/* Waits for the warm-up thread; *ms_out (may be NULL) = how long it ran.  OLA_E_INVALID_ARG when ola_gpu_warmup was never called,
 * OLA_E_HIP when the thread failed (message in ola_gpu_last_error). */
int32_t ola_gpu_warmup_wait(double* ms_out);
const char* ola_gpu_last_error(void);
int32_t ola_gpu_sync(OlaCtx* ctx);
/* Scratch and commitment buffers are recycled through a per-context cache (tens of GB after a 2^22-row proof); this returns
 * the cached blocks to the driver.  Live OlaBatch objects are not affected.
 * Single-device contexts of one process that sit on the same GPU hand cached blocks to each other: a context that needs a
 * block takes a fitting one from a sibling that is idle (no call running on it, its stream drained) before it asks the
 * driver -- a host that keeps a Poseidon and a Blake3 context pays for one pool, and the second context's first proof does
 * not wait for the driver to scrub recycled VRAM.  OLA_POOL_SHARE=0 (read at ola_gpu_init) keeps a context out of it. */
int32_t ola_gpu_trim(OlaCtx* ctx);
/* Device memory of the context's buffer pool, in bytes: out[0] handed out now, out[1] the most ever handed out at once,
 * out[2] handed out + cached now, out[3] the most ever held (the high-water mark of a proof; reset = 1 restarts the marks).
 * On a multi-device context every rank has its own pool: each figure is the largest over the ranks (what one GPU must hold). */
int32_t ola_gpu_memory_stats(OlaCtx* ctx, uint64_t out[4], int32_t reset);
/* Where the device time of a proof goes with respect to the coset partition.  enable: 1 / 0 switches the accounting on / off for
 * the proofs that follow (a few hundred event records per proof, no synchronisation), -1 leaves it as it is.  out (may be NULL)
 * describes the LAST ola_prove_with_traces of this context:
 *   out[0]  wall-clock milliseconds of the call
 *   out[1..3]  milliseconds of kernel time in work that the partition divides among the ranks, by the largest world that still
 *           divides it: [1] at most 2 ranks, [2] at most 4, [3] 8 (commitment LDEs, leaf hashing, Merkle sub-trees, quotient
 *           evaluation on 2^qdb cosets, opening evaluations, the first FRI layer).  On a multi-rank run this is rank 0's SHARE.
 *   out[4], out[5]  bytes gathered by the partition's exchanges (all ranks' payload together; a rank receives (G-1)/G of it)
 *           and their number -- counted on a single-GPU run as well, which is what makes a projection from one GPU possible:
 *           T(G) ~ out[0] - sum_k out[k] * (1 - 1/min(G, 2^k)) + out[4] * (G-1)/G / (xGMI rate) + out[5] * latency
 *   out[6], out[7]  multi-device context only: exchanges performed by the library's own all-gather and the bytes they moved between
 *           the ranks, both SINCE THE CONTEXT WAS CREATED (divide by the number of proofs). */
int32_t ola_gpu_proof_stats(OlaCtx* ctx, int32_t enable, double out[8]);
/* With the accounting on, the kernel families of the last proof one by one (Merkle leaves/s,
 * permutations/s, FRI-fold bytes/s of a REAL proof): out[3*i .. 3*i+2] = device milliseconds and two unit counters of phase i.
 *   OLA_PHASE_LEAF_HASH      hash invocations (sponge permutations / Blake3 compressions), bytes read + written
 *   OLA_PHASE_MERKLE_LEVELS  inner nodes hashed (one permutation each under Poseidon), bytes read + written
 *   OLA_PHASE_FRI_FOLD       bytes read + written, extension elements folded (fri/prover.rs:98-112)
 *   OLA_PHASE_LDE            bytes read + written by the coset LDEs (8*n*(1 + cosets) per column), column-cosets
 *   OLA_PHASE_INTT           bytes (16*n per column), columns
 *   OLA_PHASE_QUOTIENT       LDE points evaluated, bytes a point streams (local + next row of the trace and Z batches, 16 written)
 *   OLA_PHASE_OPEN_EVAL      coefficient x point products, bytes read
 * (hash/merkle_tree/mod.rs:180-266, fri/prover.rs:72-121, fri/oracle.rs:66-99).  On a multi-device context: rank 0's share. */
#define OLA_PHASE_LEAF_HASH 0
#define OLA_PHASE_MERKLE_LEVELS 1
#define OLA_PHASE_FRI_FOLD 2
#define OLA_PHASE_LDE 3
#define OLA_PHASE_INTT 4
#define OLA_PHASE_QUOTIENT 5
#define OLA_PHASE_OPEN_EVAL 6
#define OLA_PHASE_COUNT 7
/* Asked for 2 * OLA_PHASE_COUNT rows, rows OLA_PHASE_COUNT + p hold phase p's DOMINANT scope -- the one launch (or group of launches) that
 * moved the most bytes: {device ms, its bytes, 0}.  A phase's totals hide it behind the launch-bound small ones (a proof has about thirty
 * FRI folds, two of them large). */
int32_t ola_gpu_phase_stats(OlaCtx* ctx, double* out /* 3 * n_phases */, uint32_t n_phases);
/* The reference's `timed!` scopes of the LAST whole proof with device times, for the caller's TimingTree (prover.rs:84
 * `timing: &mut TimingTree`; plonky2/plonky2/src/util/timing.rs:7-194; scope names prover.rs:111-553, fri/oracle.rs:56-90,221-225,
 * fri/prover.rs:41-58).  enable: 1 / 0 switches the recording on / off for the proofs that follow (two event records per scope on
 * the context's stream, no synchronisation inside the proof), -1 leaves it.  out (may be NULL; cap entries): the scopes in the
 * order they were entered; *n_out (may be NULL) their number (returns OLA_E_INVALID_ARG when cap is too small; *n_out is set).
 *   name                the reference's scope name ("compute Zs commitment", "IFFT", "perform final FFT 33554432", ...) or one of
 *                       this library's grouping scopes ("table 3 prove_single_table", "prove_with_traces total")
 *   is_reference_scope  1 when the reference has a `timed!` of that name at that place
 *   depth / ref_depth   open scopes around it: all of them / only the reference's (the reference's tree is flat across tables)
 *   table               index of the table being proven, -1 outside
 *   start_ms, ms        when the GPU entered the scope (since the proof's first enqueue) and how long it stayed
 *   sharded_ms          part of `ms` that the coset partition divides among ranks (needs ola_gpu_proof_stats switched on)
 * "transpose LDEs" (fri/oracle.rs:84) never appears: the LDE is produced in leaf order, there is no transpose. */
typedef struct OlaScopeTime {
    char name[64];
    uint32_t depth;
    uint32_t ref_depth;
    int32_t table;
    uint32_t is_reference_scope;
    double start_ms;
    double ms;
    double sharded_ms;
} OlaScopeTime;
int32_t ola_gpu_scope_times(OlaCtx* ctx, int32_t enable, OlaScopeTime* out, uint32_t cap, uint32_t* n_out);
/* The trace upload of the last whole proof: out[0] milliseconds the proving thread was blocked waiting for column groups,
 * out[1] milliseconds from the first byte asked for to the last byte on the device, out[2] until the first column group was
 * complete, out[3] bytes, out[4] path (0 pinned staging ring, 1 pageable hipMemcpyAsync: env OLA_UPLOAD),
 * out[5] copier threads, out[6] bytes that crossed the link (columns whose words are all below 2^32 travel as 32-bit words and are
 * widened on the device: OLA_UPLOAD_PACK=0 switches that off), out[7] reserved.  On a multi-device context: rank 0's share. */
int32_t ola_gpu_upload_stats(OlaCtx* ctx, double out[8]);
/* The transform passes one by one (the roofline of the DOMINANT kernel needs that kernel's own launch duration, not
 * the mean over a transform's passes).  enable: 1 / 0 switches on / off, for the transforms that follow, two event records around
 * every launch of ntt2t_pass_kernel on the context's stream (log_n >= 14; no synchronisation inside a transform), -1 leaves it.
 * The call drains the stream and returns what was recorded since the last call, summed per kernel instantiation
 * (template arguments as rocprofv3 prints them: <R, MODE, INV, CB, LM>), and forgets it.  out may be NULL; *n_out = entries. */
typedef struct OlaPassTime {
    char kernel[48];
    uint32_t launches;
    uint32_t reserved;
    double total_ms;
    double elements;            /* field elements the launches transformed (each read once and written once) */
} OlaPassTime;
int32_t ola_gpu_ntt_pass_times(OlaCtx* ctx, int32_t enable, OlaPassTime* out, uint32_t cap, uint32_t* n_out);
/* Self-test of the device field arithmetic: the kernels' modular reduction is written with explicit carry chains in inline
 * assembly (olavm_amd/csrc/gl.cuh); this compares it with the plain C++ reduction on a table of edge values and on `pairs`
 * pseudo-random operand pairs and returns the number of disagreements (0 expected; about 10^9 pairs per 50 ms).  It also runs
 * the limb arithmetic of the transform passes (olavm_amd/csrc/ntt2t.cuh: fold to u64 with its carry fixes, carry step, product
 * cut into limbs, table multiplication, the sixteen shifts of a radix-16 block) against canonical arithmetic on pairs / 16 limb
 * vectors that sit on the magnitude bounds.  Meant to be run once after ola_gpu_init on a new driver or compiler. */
int32_t ola_gpu_selftest(OlaCtx* ctx, uint64_t pairs, uint64_t* mismatches);
/* Start allocating, on a helper thread, the large device buffers that ola_prove_with_traces will need for this AIR set and these
 * table heights (log2 rows per table); returns at once.  The driver scrubs previously used VRAM inside hipMalloc (about 30 ms per
 * GB here), which is what makes the first proof of a process slow; called right after ola_gpu_init -- before the host reads or
 * generates the traces -- it moves that cost off the proof.  Optional: proving without it is correct, only colder. */
int32_t ola_gpu_reserve(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint32_t* log_n);

/* ---- per-phase entry points: one `timed!` scope of prove_single_table at a time ---------------------------------------
 * The Rust host keeps its transcript and draws the challenges exactly where the reference does; each call replaces the body of
 * one scope (circuits/src/stark/prover.rs:374-480) and hands host arrays back, so a port can move to the GPU one scope at a
 * time and compare with the CPU prover after every step.  ola_prove_single_table is the same sequence in one call. */
/* out[6] = columns, public-parameter words, permutation Z columns, CTL Z columns, quotient_degree_factor,
 * permutation_batch_size of table `table` of the AIR set (for config.num_challenges of the context). */
int32_t ola_table_shape(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, uint32_t table, uint32_t out[6]);
/* compute_permutation_z_polys (permutation.rs:103-187).  trace_cols: host columns of 2^log_n rows; perm_challenges:
 * [permutation_batch_size][num_challenges][2] = (beta, gamma) in get_n_grand_product_challenge_sets order (prover.rs:360-367);
 * z_out: [permutation Z columns][n], column-major values (the head of the reference's `z_polys`).
 * A row at which the product of the right-hand sides gamma + sum beta^k rhs_k of a batch is zero has no quotient: the reference
 * panics "Tried to invert zero" there (permutation.rs:143, plonky2/field/src/types.rs:99-101).  Here that is OLA_E_INVALID_ARG with
 * the message "Tried to invert zero: table T, permutation batch B ..." (the first such batch), from this call, from
 * ola_prove_single_table and from ola_prove_with_traces alike; the context stays usable.  ola_ctl_z does not report it: it has no
 * permutation challenges and returns no permutation column.  A table without permutation arguments has no Z column here:
 * nothing is written, the call succeeds.  Filters are ola_ctl_z's business: this call does not look at them. */
int32_t ola_perm_z(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, uint32_t table, uint32_t log_n,
                   const uint64_t* const* trace_cols, const uint64_t* perm_challenges, uint64_t* z_out);
/* The table's columns of cross_table_lookup_data (cross_table_lookup.rs:224-311), looking sides before looked sides, lookups in
 * declaration order, challenge-minor.  ctl_challenges: [num_challenges][2] = (beta, gamma).  z_out: [CTL Z columns][n].
 * "Non-binary filter?" is reported as OLA_E_INVALID_ARG. */
int32_t ola_ctl_z(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, uint32_t table, uint32_t log_n,
                  const uint64_t* const* trace_cols, const uint64_t* ctl_challenges, uint64_t* z_out);
/* compute_quotient_polys and the split into chunks (prover.rs:441-480, 571-705).  trace / zs: the table's trace and Z commitments
 * (ola_commit_values of the trace columns and of perm Z columns followed by CTL Z columns); alphas: [num_challenges];
 * chunks_out: [num_challenges * quotient_degree_factor][n] coefficients, the input of from_coeffs (ola_commit_coeffs).
 * OLA_E_QUOTIENT_DEGREE when the trace does not satisfy the constraints. */
int32_t ola_quotient(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, uint32_t table, const OlaBatch* trace,
                     const OlaBatch* zs, const uint64_t* perm_challenges, const uint64_t* ctl_challenges, const uint64_t* alphas,
                     const uint64_t* params, uint64_t* chunks_out);

/* ---- NTT family: replaces gpu_method and the cfft CPU paths --------------------------------------------
 * op selects the reference function (plonky2/field/src/cfft/mod.rs):
 *   OLA_NTT_EVALUATE              evaluate_poly               :22   coeffs -> values on <w>, natural order
 *   OLA_NTT_INTERPOLATE           interpolate_poly            :128  values -> coeffs (x n^-1), natural order
 *   OLA_NTT_COSET_LDE             evaluate_poly_with_offset   :65   n coeffs -> n*2^blowup_log values at
 *                                                                   shift*g^m, m natural (shift = `shift`)
 *   OLA_NTT_COSET_INTERPOLATE     interpolate_poly_with_offset:180  values on shift*<w> -> coeffs
 *   OLA_NTT_COSET_LDE_LEAF_ORDER  the same LDE (shift must be 7) but rows in commitment-leaf order, i.e.
 *                                 bit-reversed (what PolynomialBatch::from_coeffs feeds the Merkle tree,
 *                                 fri/oracle.rs:84-85) -- the order the device keeps internally.
 * `in`/`out` are column-major batches; out may equal in when the op preserves length.
 */
#define OLA_NTT_EVALUATE 0
#define OLA_NTT_INTERPOLATE 1
#define OLA_NTT_COSET_LDE 2
#define OLA_NTT_COSET_INTERPOLATE 3
#define OLA_NTT_COSET_LDE_LEAF_ORDER 4

int32_t ola_ntt_batch(OlaCtx* ctx, int32_t op, const uint64_t* in, uint64_t* out, uint32_t log_n, uint32_t batch,
                      uint64_t shift, uint32_t blowup_log);
/* same, operands resident in HBM; `scratch_dev` must hold batch * 2^log_n elements when log_n > 13 and the op
 * produces natural order (NULL lets the library allocate and free it). */
int32_t ola_ntt_batch_dev(OlaCtx* ctx, int32_t op, const uint64_t* in_dev, uint64_t* out_dev, uint64_t* scratch_dev,
                          uint32_t log_n, uint32_t batch, uint64_t shift, uint32_t blowup_log);

/* ---- Poseidon / Merkle: replaces hash/poseidon.rs:593-603, hashing.rs:84-111, merkle_tree/mod.rs:180-337 --
 * ola_hash_rows, ola_merkle_cap and every commitment hash with the context's Hasher: the Poseidon sponge, the Poseidon2 sponge
 * under OLA_HASH_POSEIDON2 / OLA_HASH_POSEIDON2_POW_POSEIDON (the same sponge and tree, hash/poseidon2.rs:500-512), or under
 * OLA_HASH_KECCAK KeccakHash<25> (hash/keccak.rs; word 3 of a digest is byte 24 alone), or under
 * OLA_HASH_BLAKE3 Blake3_256 (hash/blake3.rs:203-233) of the canonical little-endian words; a digest is 4 words (32 bytes)
 * either way, and a Blake3 digest is bytes -- its words may be >= p and are never reduced. */
/* n states of 12 elements each, permuted in place (host memory). */
int32_t ola_poseidon_permute(OlaCtx* ctx, uint64_t* states, size_t n);
/* The same with the Poseidon2 permutation, `poseidon2` (hash/poseidon2.rs:50-82), under any hasher of the context. */
int32_t ola_poseidon2_permute(OlaCtx* ctx, uint64_t* states, size_t n);
/* hash_no_pad over each row of a row-major num_rows x row_len host matrix -> digests (num_rows x 4). */
int32_t ola_hash_rows(OlaCtx* ctx, const uint64_t* rows, size_t num_rows, size_t row_len, uint64_t* digests);
/* MerkleTree::new_v2 over row-major host leaves: writes the cap (2^cap_height x 4). */
int32_t ola_merkle_cap(OlaCtx* ctx, const uint64_t* leaves, size_t num_leaves, size_t leaf_len, uint32_t cap_height,
                       uint64_t* cap_out);

/* ---- PolynomialBatch commitment: replaces PolynomialBatch::from_values / from_coeffs (fri/oracle.rs:45,66) ---
 * iNTT -> coset LDE (shift 7, blowup 2^rate_bits) -> Poseidon leaf hashes -> Merkle cap, all on the device.
 * cols: ncols host pointers (ola_commit_*) or one device buffer, column-major (ola_commit_*_dev).
 * cap_out: 2^cap_height x 4 canonical elements (host).  *out_batch stays resident until ola_batch_free. */
int32_t ola_commit_values(OlaCtx* ctx, const uint64_t* const* cols, uint32_t ncols, uint32_t log_n,
                          OlaBatch** out_batch, uint64_t* cap_out);
int32_t ola_commit_coeffs(OlaCtx* ctx, const uint64_t* const* cols, uint32_t ncols, uint32_t log_n,
                          OlaBatch** out_batch, uint64_t* cap_out);
int32_t ola_commit_values_dev(OlaCtx* ctx, const uint64_t* cols_dev, uint32_t ncols, uint32_t log_n,
                              OlaBatch** out_batch, uint64_t* cap_out);
int32_t ola_commit_coeffs_dev(OlaCtx* ctx, const uint64_t* cols_dev, uint32_t ncols, uint32_t log_n,
                              OlaBatch** out_batch, uint64_t* cap_out);
/* One GPU's share of PolynomialBatch::from_values under the coset partition: with rate_bits = 3 the LDE is 8
 * independent cosets that are also contiguous blocks of n commitment leaves.  Shard `rank` of `world`
 * (1, 2, 4 or 8) interpolates all columns (replicated), extends them onto cosets [rank*8/world, (rank+1)*8/world), hashes
 * those leaves and builds their sub-trees; cap_slice_out receives entries [rank*16/world, (rank+1)*16/world) of the
 * commitment's Merkle cap (2^cap_height/world digests).  Concatenating the slices of all ranks in rank order -- one
 * all-gather of 512/world bytes -- gives exactly the cap ola_commit_values returns.  The batch answers
 * ola_batch_get_leaf for local leaf indices (global index - rank*N/world) with paths up to its own cap slice. */
int32_t ola_commit_values_shard(OlaCtx* ctx, const uint64_t* const* cols, uint32_t ncols, uint32_t log_n, uint32_t rank,
                                uint32_t world, OlaBatch** out_batch, uint64_t* cap_slice_out);
int32_t ola_commit_values_shard_dev(OlaCtx* ctx, const uint64_t* cols_dev, uint32_t ncols, uint32_t log_n, uint32_t rank,
                                    uint32_t world, OlaBatch** out_batch, uint64_t* cap_slice_out);
int32_t ola_batch_free(OlaCtx* ctx, OlaBatch* batch);
/* accessors (PolynomialBatch.polynomials, MerkleTree::get / prove, merkle_tree/mod.rs:268-308) */
int32_t ola_batch_shape(const OlaBatch* batch, uint32_t* ncols, uint32_t* log_n, uint32_t* rate_bits);
int32_t ola_batch_get_coeffs(OlaCtx* ctx, const OlaBatch* batch, uint64_t* out /* ncols x n, column-major */);
int32_t ola_batch_get_leaf(OlaCtx* ctx, const OlaBatch* batch, size_t leaf_index, uint64_t* row_out /* ncols */,
                           uint64_t* siblings_out /* (log_n+rate_bits-cap_height) x 4 */);
/* fri/oracle.rs:131-137 get_lde_values(index, step): natural-order LDE row index*step */
int32_t ola_batch_get_lde_row(OlaCtx* ctx, const OlaBatch* batch, size_t index, size_t step, uint64_t* row_out);

/* ---- openings + FRI: replaces StarkOpeningSet::new (circuits/src/stark/proof.rs:198-233),
 * PolynomialBatch::prove_openings (fri/oracle.rs:167-241) and fri_proof (fri/prover.rs:20-204).
 * The Fiat-Shamir transcript stays on the host: the caller passes the 12-element challenger state and the
 * buffered inputs, and receives them back (iop/challenger.rs:36-162); see OlaChallenger. */
typedef struct OlaChallenger {
    uint64_t sponge_state[12];
    uint64_t input_buffer[8];
    uint64_t output_buffer[8];
    uint32_t input_len;
    uint32_t output_len;
    uint32_t hasher;            /* OLA_HASH_*: the permutation (Poseidon, Poseidon2, Blake3Permutation or KeccakPermutation) and       */
    uint32_t reserved;          /* how a digest is observed; set by the init calls, do not change afterwards                 */
} OlaChallenger;

int32_t ola_challenger_init(OlaChallenger* ch);                          /* Challenger::<F, PoseidonHash>::new()          */
int32_t ola_challenger_init_hasher(OlaChallenger* ch, uint32_t hasher);  /* Challenger::<F, C::Hasher>::new(), hashers 0..3 */
/* Challenger::<F, KeccakHash<25>>::new(): the transcript of OLA_HASH_KECCAK.  Its own entry point: ola_challenger_init_hasher keeps
 * the range of values it was published with (0..3) and refuses every other, 5 included. */
int32_t ola_challenger_init_keccak(OlaChallenger* ch);
/* observe_cap (iop/challenger.rs:75-84) of n digests of 4 words: a Poseidon digest is 4 elements, a Blake3 digest is observed
 * as the 5 elements BytesHash::to_vec cuts it into (7 bytes each, hash/hash_types.rs:142-152), a Keccak digest (25 bytes: words
 * 0..2 and the low byte of word 3) as 4 elements of 7, 7, 7 and 4 bytes. */
int32_t ola_challenger_observe_cap(OlaChallenger* ch, const uint64_t* digests, size_t n);
/* Blake3_256::hash_no_pad of n field elements as this backend computes it on the device (canonical little-endian words,
 * hash/blake3.rs:203-213), on the host: for digests the integrator needs outside a proof, and the CPU-side test of the kernel code. */
int32_t ola_blake3_hash_elements(const uint64_t* elems, size_t n, uint64_t out[4]);
/* KeccakHash<25>::hash_no_pad of n field elements (1..4096) the same way (hash/keccak.rs: the first 25 bytes of Keccak-256 -- original
 * padding, not SHA3-256 -- of the canonical little-endian words), on the host: out[0..2] are bytes 0..23, out[3] is byte 24. */
int32_t ola_keccak_hash_elements(const uint64_t* elems, size_t n, uint64_t out[4]);
int32_t ola_challenger_observe(OlaChallenger* ch, const uint64_t* elems, size_t n);
int32_t ola_challenger_get(OlaChallenger* ch, uint64_t* out, size_t n);
int32_t ola_challenger_compact(OlaChallenger* ch);

/* The tail of prove_single_table from `zeta` on (prover.rs:499-553) for three resident commitments
 * (trace, permutation/CTL Zs, quotient chunks): draws zeta, evaluates the opening set, observes it, runs FRI
 * (commit phase, minimal proof-of-work nonce, 28 query rounds).  Output is the reference wire format
 * (circuits/src/stark/serialization.rs:163-176 write_opening_set || :305-317 write_fri_proof).
 * Returns OLA_E_INVALID_ARG with *out_len = required size when `cap` is too small (challenger is then unchanged). */
int32_t ola_open_and_prove(OlaCtx* ctx, const OlaBatch* trace, const OlaBatch* zs, const OlaBatch* quotient,
                           uint32_t num_permutation_zs, OlaChallenger* challenger, uint8_t* out, size_t cap,
                           size_t* out_len, size_t* openings_len);

/* FRI proof of work (fri/prover.rs:126-148): the MINIMAL witness i such that
 * InnerHasher.hash_no_pad([h0..h3, i])[0] has >= bits leading zeros; InnerHasher is Poseidon2 under OLA_HASH_POSEIDON2 and
 * Poseidon under every other hasher. */
int32_t ola_pow(OlaCtx* ctx, const uint64_t h[4], uint32_t bits, uint64_t* witness);

/* ---- the same, one step per call (ABI revision 7): for a host that keeps the reference's own loops and its own Challenger and
 * hands over the device work only.  Each beta depends on the previous layer's cap through the host challenger
 * (fri/prover.rs:98-101), so the commit phase is layer-stepped.  The bytes the steps return reassemble to ola_open_and_prove's
 * (tests/test_gpu_fri_steps.py does exactly that with ola_challenger_*).  Single-device contexts; the three batches must outlive
 * the OlaFri.
 *   ola_open                   StarkOpeningSet::new (circuits/src/stark/proof.rs:198-233) at the caller's zeta: the opening set in
 *                              wire format (serialization.rs:164-175 write_opening_set; read it back with read_opening_set, :176-193) -- decode, then
 *                              challenger.observe_openings(&openings.to_fri_openings()) (fri/challenges.rs:16-23)
 *                              zeta is the caller's, any two words (reduced mod p).  Refused: a zeta with zeta^n = 1
 *                              (OLA_E_ZETA_IN_SUBGROUP, prover.rs:508-511) and zeta = 0 (OLA_E_INVALID_ARG: the division by
 *                              X - zeta goes through powers of 1 / zeta); ola_open_and_prove refuses the same two of a zeta
 *                              drawn from its transcript
 *   ola_fri_plan               fri_params.reduction_arity_bits (fri/reduction_strategies.rs:40-52) and the final polynomial's length
 *   ola_fri_commit_begin       PolynomialBatch::prove_openings up to the final polynomial (fri/oracle.rs:178-219), alpha =
 *                              challenger.get_extension_challenge()
 *   ola_fri_commit_next_layer  one turn of fri_committed_trees (fri/prover.rs:72-121): folds by the PREVIOUS layer's beta (NULL for the
 *                              first layer), commits the current polynomial's values on its coset, cap_out = 2^cap_height x 4 words
 *   ola_fri_commit_finish      folds by the last beta (NULL when the plan has no layer): the final polynomial, (a, b) pairs
 *                              (prover.rs:114-119); *n_out = its length
 *   ola_pow (above)            fri_proof_of_work (prover.rs:126-148), minimal witness
 *   ola_fri_query              fri_prover_query_rounds (prover.rs:150-204) for the caller's indices (challenger output mod the LDE
 *                              size): the query round proofs in wire format (write_fri_query_rounds, serialization.rs:275-292: count, per query the three
 *                              oracles' rows and paths and every layer's leaf and path); n = 0 is OLA_E_INVALID_ARG, and the
 *                              handle goes on answering */
typedef struct OlaFri OlaFri;
int32_t ola_open(OlaCtx* ctx, const OlaBatch* trace, const OlaBatch* zs, const OlaBatch* quotient, uint32_t num_permutation_zs,
                 const uint64_t zeta[2], uint8_t* out, size_t cap, size_t* out_len, OlaFri** fri_out);
int32_t ola_fri_plan(const OlaFri* fri, uint32_t* arity_bits, uint32_t cap, uint32_t* n_layers, uint32_t* final_poly_len);
int32_t ola_fri_commit_begin(OlaFri* fri, const uint64_t alpha[2]);
int32_t ola_fri_commit_next_layer(OlaFri* fri, const uint64_t* beta, uint64_t* cap_out);
int32_t ola_fri_commit_finish(OlaFri* fri, const uint64_t* beta, uint64_t* final_poly_out, size_t cap_elems, size_t* n_out);
int32_t ola_fri_query(OlaFri* fri, const uint64_t* x_index, uint32_t n, uint8_t* out, size_t cap, size_t* out_len);
int32_t ola_fri_free(OlaFri* fri);

/* ---- the whole multi-table proof: replaces prove_with_traces (circuits/src/stark/prover.rs:79-327) -------------
 * airset: the AIR-set description (tables, constraint programs, permutation pairs, cross-table lookups) as a u64
 *   array -- the data form of the reference's OlaStark (stark/ola_stark.rs:29-64, 122-560); format and generator in
 *   olavm_amd/air/dsl.py.
 * traces[t]: pointer to table t, column-major ncols x 2^log_n[t] (the [Vec<PolynomialValues<F>>; NUM_TABLES]
 *   that generate_traces returns, generation/mod.rs:77-213): host memory (pageable is fine; the upload overlaps the first
 *   commitments), or memory of this GPU for a table that is already resident -- table by table, the library looks at the
 *   pointer.  A resident table must be complete on the context's stream (or the device idle) when the call is made; the
 *   tables are not modified.
 * params: concatenated per-table constraint parameters (e.g. the bitwise/program compress challenge read inside
 *   the AIR), may be NULL when no table has any; compress_challenges: one per table as carried in AllProof
 *   (prover.rs:307-320), may be NULL (zeros).
 * out: AllProof in the reference wire format (serialization.rs:377-393 write_all_proof).  Returns
 * OLA_E_INVALID_ARG with *out_len = required size when `cap` is too small -- the finished proof then stays in the context
 * and ola_take_pending_proof copies it out without proving again -- and OLA_E_QUOTIENT_DEGREE when the trace does not
 * satisfy the constraints (prover.rs:469-473).  A 12-table proof is 0.8 - 1.2 MB. */
int32_t ola_prove_with_traces(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint64_t* const* traces,
                              const uint32_t* log_n, const uint64_t* params, const uint64_t* compress_challenges,
                              uint8_t* out, size_t cap, size_t* out_len);

/* The same proof from the reference's own trace type: prove_with_traces takes `&[Vec<PolynomialValues<F>>; NUM_TABLES]`
 * (circuits/src/stark/prover.rs:79-83) -- per table a Vec of columns, every column its own Vec<F>
 * (plonky2/field/src/polynomial/mod.rs:24-26), F = GoldilocksField = repr(transparent) u64 (goldilocks_field.rs:24-26).
 * cols[t][c]: pointer to the 2^log_n[t] values of column c of table t, wherever the caller's allocator put it; the Rust shim
 * passes `c.values.as_ptr() as *const u64` and copies nothing (precedent for per-column pointers: cfft/ntt/mod.rs:123-147).
 * ola_prove_with_traces is the special case cols[t][c] = traces[t] + c 2^log_n[t].  Everything else as above; host columns are
 * staged through the context's pinned ring by a few copier threads (OLA_UPLOAD_THREADS, default min(4, host threads per rank - 1); olavm_amd/csrc/upload.h),
 * a table whose FIRST column is device memory is taken as resident on this GPU column by column. */
int32_t ola_prove_with_traces_cols(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint64_t* const* const* cols,
                                   const uint32_t* log_n, const uint64_t* params, const uint64_t* compress_challenges,
                                   uint8_t* out, size_t cap, size_t* out_len);

/* ---- why a trace does not prove: the constraint check on the trace domain -------------------------------------------------
 * ola_prove_with_traces* answers a trace that breaks a constraint with OLA_E_QUOTIENT_DEGREE and nothing more.  This is the
 * reference's debugging aid for that case on the device: `check_constraints` (circuits/src/stark/prover.rs:711-819), which
 * evaluates a table's constraints on the trace domain H itself instead of the LDE, `verify_cross_table_lookups`
 * (cross_table_lookup.rs:551-584), which compares the last values of the CTL Z columns, and the per-table recipe that strings
 * them together (test_utils.rs:152-195).  Nothing is committed, extended or hashed.
 * airset, cols, log_n, params: as for ola_prove_with_traces_cols (per-column pointers: host memory, staged through the pinned
 *   ring, or a table whose first column is device memory is taken as resident); words may be >= p.  Only the tables of
 *   table_mask (bit t = table t; a bit beyond the set is OLA_E_INVALID_ARG) are read, cols[t] of the others may be NULL.
 * out[0 .. min(cap, *n_out)): the failures, sorted by (table, section, index, kind); *n_out is their TOTAL number also when it
 *   exceeds cap (out may be NULL when cap is 0), so one call sizes the buffer.  A trace that satisfies everything gives
 *   *n_out == 0; the return value is OLA_OK whether or not failures were found.
 *   OLA_CHECK_AIR          one entry per failing emit of the table's constraint program: index = ordinal of the emit in program
 *                          order, kind = OLA_CONSTRAINT_* (the ConstraintConsumer method, constraint_consumer.rs:57-78); the emit
 *                          fails at row i iff its value there is non-zero and the kind applies: every row (ALL), every row but
 *                          the last (TRANSITION), row 0 (FIRST_ROW), row n-1 (LAST_ROW) -- where z_last and the Lagrange
 *                          selectors are non-zero on H (constraint_consumer.rs:34-78).  The next row of row n-1 is row 0.
 *                          first_row = the smallest failing row, rows_failing = their number.
 *   OLA_CHECK_PERMUTATION  one entry per permutation batch (index) whose running product does not close,
 *                          Z[n-1] num(n-1) != den(n-1) Z[0] (permutation.rs:302-360): the two sides of a pair are not
 *                          permutations of each other.  first_row = n-1, rows_failing = 1, kind = 0.
 *   OLA_CHECK_LOOKUP       one entry per (cross-table lookup, challenge) for which the product of the looking tables' last CTL Z
 *                          values differs from the looked table's: table = the looked table, index = the lookup's position in
 *                          all_cross_table_lookups() order (the AIR set's), kind = the challenge, first_row = filter-selected
 *                          rows on the looking side (all looking tables), rows_failing = filter-selected rows of the looked
 *                          table.  A lookup is checked when all of its tables are in table_mask.  The per-row recurrences of
 *                          the CTL Z columns hold by construction (the library computes the columns) and are not evaluated.
 * ctl_challenges: [num_challenges][2] = (beta, gamma), or NULL.  The permutation challenges, and with NULL the CTL challenges
 *   too, come from a fresh Challenger of the context's hasher that has observed nothing: first num_challenges (beta, gamma)
 *   pairs for the lookups, then for every table of the set in order its permutation_batch_size x num_challenges pairs
 *   (tables without permutation pairs draw nothing).  Deterministic; a random trace error escapes with probability ~ n / p.
 * A multi-device context runs the check on its first device.  The proving state of the context is not touched.  Without a HIP
 * device there is no context to pass: a call whose other arguments are valid then returns OLA_E_NO_DEVICE (no CPU fallback). */
#define OLA_CHECK_AIR 0u
#define OLA_CHECK_PERMUTATION 1u
#define OLA_CHECK_LOOKUP 2u
#define OLA_CONSTRAINT_ALL 0u
#define OLA_CONSTRAINT_TRANSITION 1u
#define OLA_CONSTRAINT_FIRST_ROW 2u
#define OLA_CONSTRAINT_LAST_ROW 3u
typedef struct OlaConstraintFailure {
    uint32_t table;
    uint32_t section;           /* OLA_CHECK_AIR | OLA_CHECK_PERMUTATION | OLA_CHECK_LOOKUP                                   */
    uint32_t index;             /* AIR: emit ordinal; PERMUTATION: batch; LOOKUP: lookup index                                */
    uint32_t kind;              /* AIR: OLA_CONSTRAINT_*; LOOKUP: challenge index, 0 .. num_challenges - 1                    */
    uint64_t first_row;         /* LOOKUP: selected rows on the looking side                                                  */
    uint64_t rows_failing;      /* LOOKUP: selected rows on the looked side                                                   */
} OlaConstraintFailure;
int32_t ola_check_constraints(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint64_t* const* const* cols,
                              const uint32_t* log_n, const uint64_t* params, const uint64_t* ctl_challenges, uint32_t table_mask,
                              OlaConstraintFailure* out, uint32_t cap, uint32_t* n_out);

/* ---- which rows a failing cross-table lookup is missing ---------------------------------------------------------------------
 * An OLA_CHECK_LOOKUP entry says that lookup `index` fails and how many rows each side selects; the CTL Z products it compares
 * have no memory of WHICH tuple is unmatched.  The reference answers that by hand: one file per lookup under
 * circuits/src/generation/ctl_test/ (cpu_mem.rs, cpu_program.rs, poseidon_chunk_mem.rs, storage_access_poseidon.rs, ...)
 * filters the looking and the looked rows, projects the lookup's data columns and prints both lists for a person to diff
 * (generation/ctl_test/debug_trace_print.rs:64-88, :299-333).  This call computes the exact multiset difference of the two sides of ONE lookup on the
 * device -- what verify_cross_table_lookups (stark/cross_table_lookup.rs:551-584) can only refuse as a whole.  No challenge is
 * involved: the answer is exact, not probabilistic.
 * airset, cols, log_n: as for ola_check_constraints (per-column pointers: host memory, staged through the pinned ring, or a
 *   table whose first column is device memory is taken as resident; words may be >= p).  Only the tables the lookup names are
 *   read, cols[t] of the others may be NULL.
 * lookup: position in all_cross_table_lookups() order = OlaConstraintFailure.index of an OLA_CHECK_LOOKUP entry; out of range is
 *   OLA_E_INVALID_ARG, and so is a lookup of more than OLA_LOOKUP_MAX_VALUES data columns (a foreign AIR set).
 * A row of a side is selected when its filter column's canonical value is 1 (every row when the side has no filter), as the CTL Z
 *   columns select it; its tuple is the canonical values of the side's `Column` linear combinations.
 * out[0 .. min(cap, *n_out)): one entry per distinct tuple with looking_count != looked_count, sorted lexicographically by
 *   values[0 .. *width) as unsigned canonical words; *n_out is their TOTAL number also beyond cap (out may be NULL when cap is 0).
 *   The first carrier on the looking side is the minimum of (entry position in the lookup's looking list, row): looking_entry and
 *   looking_table name it (one table may appear in several entries).
 * totals: {selected looking rows (all entries), selected looked rows, distinct mismatching tuples, sum of |looking_count -
 *   looked_count|}; *width: the lookup's number of data columns.  n_out, totals and width must not be NULL.
 * The return value is OLA_OK whether or not anything mismatches.  The proving state of the context is not touched; a multi-device
 * context works on its first device; without a HIP device a call whose other arguments are valid returns OLA_E_NO_DEVICE.
 * OLA_LOOKUP_MAX_VALUES: the widest lookup of the 12-table OlaStark (olavm_amd/air/ola_tables.py), as `python -m olavm_amd.air.dump
 * --lookup-max-values` prints it. */
#define OLA_LOOKUP_MAX_VALUES 24
typedef struct OlaLookupMismatch {
    uint64_t looking_count;     /* filter-selected looking rows (all looking entries) that carry this tuple */
    uint64_t looked_count;      /* filter-selected rows of the looked table that carry it                   */
    uint32_t looking_entry;     /* position in the lookup's looking list of the first carrier, or UINT32_MAX */
    uint32_t looking_table;     /* that entry's table, or UINT32_MAX                                         */
    uint64_t looking_row;       /* smallest row of that entry carrying the tuple, or UINT64_MAX              */
    uint64_t looked_row;        /* smallest looked row carrying it, or UINT64_MAX                            */
    uint64_t values[OLA_LOOKUP_MAX_VALUES]; /* the tuple, canonical, the first `width` words; the rest zero  */
} OlaLookupMismatch;
int32_t ola_check_lookup(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint64_t* const* const* cols,
                         const uint32_t* log_n, uint32_t lookup, OlaLookupMismatch* out, uint32_t cap, uint32_t* n_out,
                         uint64_t totals[4], uint32_t* width);

/* Copies out (and forgets) the proof a preceding ola_prove_with_traces could not return because its buffer was too small. */
int32_t ola_take_pending_proof(OlaCtx* ctx, uint8_t* out, size_t cap, size_t* out_len);

/* One table of that proof with the orchestration left to the caller: replaces prove_single_table
 * (circuits/src/stark/prover.rs:330-513) together with this table's share of cross_table_lookup_data
 * (cross_table_lookup.rs:224-311), compute_permutation_z_polys (permutation.rs:103-155) and compute_quotient_polys
 * (prover.rs:571-705).  The caller has committed the traces (ola_commit_values -> trace_commitment, trace_cap), observed
 * all trace caps and drawn the CTL challenges (get_grand_product_challenge_set, permutation.rs:190-216:
 * ctl_challenges = num_challenges x (beta, gamma)); `challenger` is the shared transcript at the point where the
 * reference calls prove_single_table for table `table` and is advanced exactly as the reference advances it.
 * trace_cols: host pointers to the table's columns (values, 2^log_n each).  out: this table's StarkProof bytes
 * (serialization.rs:349-358 write_proof); an AllProof is u32 count, the proofs in table order, u32 count, the compress
 * challenges.  Same error codes as ola_prove_with_traces; on error the challenger is left untouched. */
int32_t ola_prove_single_table(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, uint32_t table,
                               const uint64_t* const* trace_cols, const OlaBatch* trace_commitment, const uint64_t* trace_cap,
                               const uint64_t* ctl_challenges, const uint64_t* params, OlaChallenger* challenger, uint8_t* out,
                               size_t cap, size_t* out_len);

/* ---- trace generation helper -------------------------------------------------------------------------
 * The 134-column Poseidon STARK table (circuits/src/builtins/poseidon/columns.rs) from the permutation inputs: what the
 * reference's executor records per hash (core/src/util/poseidon_utils.rs) and generate_poseidon_trace lays out
 * (circuits/src/generation/poseidon.rs:5-80).  inputs: 12 x n column-major; filters: 4 x n column-major
 * (FILTER_LOOKED_NORMAL, _TREEKEY, _STORAGE_LEAF, _STORAGE_BRANCH) or NULL for zeros; out: 134 x n column-major.  Padding
 * rows are rows with all-zero inputs (the reference's POSEIDON_ZERO_HASH_* constants). */
int32_t ola_generate_poseidon_trace(OlaCtx* ctx, const uint64_t* inputs, const uint64_t* filters, size_t n, uint64_t* out);
/* The permuted columns of one Halo2-style lookup (circuits/src/stark/lookup.rs:68-132 permuted_cols, called for every
 * looking column of the range-check, bitwise and program tables: generation/builtin.rs:121-200, generation/prog.rs):
 * permuted_inputs = the n inputs in canonical form, ascending; permuted_table = the n table values arranged as the
 * reference's merge loop arranges them (a value next to the first of its inputs, the unused ones in the other slots, in
 * the reference's stack order).  Inputs need not occur in the table.  Host buffers / buffers resident in HBM. */
int32_t ola_permuted_cols(OlaCtx* ctx, const uint64_t* inputs, const uint64_t* table, size_t n, uint64_t* permuted_inputs,
                          uint64_t* permuted_table);
int32_t ola_permuted_cols_dev(OlaCtx* ctx, const uint64_t* inputs_dev, const uint64_t* table_dev, size_t n,
                              uint64_t* permuted_inputs_dev, uint64_t* permuted_table_dev);

/* ---- whole derived tables from their primary columns --------------------------------------------------------
 * The range-check, bitwise and program tables are mostly columns that are a function of a few primary ones: limbs, the fixed
 * sub-tables, compress columns and the permuted pairs of their in-table lookups (one sequential merge loop per pair on the host,
 * lookup.rs:68-132).  The host keeps what is cheap and policy-laden -- row order, filler rows, the filters -- and these calls
 * write everything else on the device, the permuted pairs of a table as ONE batch (a table column that several pairs look into is
 * sorted once).
 * out: the table, column-major ncols x 2^log_n -- the layout ola_prove_with_traces takes -- in host memory or in memory of the
 *   context's GPU (the library looks at the pointer); a table written into HBM can be passed to ola_prove_with_traces as a
 *   resident table and never crosses the link.  Inputs may be host or device memory as well and may hold words >= p; every
 *   word written is canonical.  Device buffers, inputs and `out` alike, must be memory of the context's GPU (memory of
 *   another GPU is OLA_E_INVALID_ARG) and complete when the call is made: the work runs on the context's stream, which does
 *   not wait for copies or fills the caller enqueued on another stream.  Every column of `out` is written; rows beyond the
 *   live inputs are zero in the primary columns.  The calls return when the table is complete.
 * out == NULL (ola_generate_rc_trace, ola_generate_bitwise_trace): *log_n_out receives the height and nothing else happens; this
 *   sizing call takes ctx == NULL as well.
 * ctx == NULL in a call that would do work: OLA_E_NO_DEVICE when the machine has no HIP device (there is no CPU fallback),
 *   OLA_E_INVALID_ARG otherwise; the other arguments are validated first.
 *
 * ola_generate_rc_trace: the 12-column range-check table of generate_rc_trace (generation/builtin.rs:249-316).
 *   vals[n_rows]; filters: 4 x n_rows column-major (CPU, MEMORY_SORT, MEMORY_REGION, CMP filter) or NULL for zeros.
 *   n = next_pow2(max(n_rows, 2^range_bits)), at least 2 (range_bits = 16 in the reference, smaller for miniature tables).
 *   LIMB_LO = val mod 2^range_bits, LIMB_HI = val >> range_bits of the canonical value -- a value >= 2^(2 range_bits) is not
 *   refused: it gives a table the AIR rejects, as the reference's would; FIX_RANGE_CHECK_U16 = 0 .. 2^range_bits - 1, then the
 *   last value repeated; the two permuted pairs.
 * ola_generate_bitwise_trace: the 59-column bitwise table of generate_bitwise_trace (generation/builtin.rs:35-206).
 *   ops: 5 x n_ops column-major -- filter, tag, op0, op1, res, copied as given (res is not recomputed).
 *   n = next_pow2(max(2^limb_bits, 3 * 4^limb_bits, n_ops)) (limb_bits = 8 in the reference).  Written: the twelve limb columns
 *   (limb l = bits [l limb_bits, (l + 1) limb_bits) of the canonical operand), the fixed AND / OR / XOR table in the reference's
 *   row order with FIX_TAG, FIX_RANGE_CHECK_U8 = 0 .. 2^limb_bits - 1 then zeros, the four COMPRESS_LIMBS columns and
 *   FIX_COMPRESS = tag + a beta + b beta^2 + c beta^3, and the sixteen permuted pairs (twelve against FIX_RANGE_CHECK_U8, four
 *   against FIX_COMPRESS).  beta is the caller's: the reference draws it from a transcript over the twelve limb columns
 *   (generation/builtin.rs:120-131), a sequential sponge that stays on the host (ola_challenger_*).
 *   flags: OLA_TABLEGEN_REFERENCE_QUIRKS leaves the three limb-3 columns zero, as the reference's generator does
 *   (generation/builtin.rs:65,70,75 write them to the exclusive end of their range; include/ola_tracegen.h describes the defect).
 * ola_generate_prog_trace: the 18-column program table of generate_prog_trace (generation/prog.rs:18-156).
 *   exec, prog: each 7 x 2^log_n column-major -- four code-address words, pc, inst, filter -- the executed side and the listing
 *   side at full height, filler rows as the caller lays them out (the reference's zero rows, or a listed word repeated with
 *   filter 0).  The fourteen columns are copied, COL_PROG_EXEC_COMP_PROG and COL_PROG_COMP_PROG =
 *   a0 + a1 beta + a2 beta^2 + a3 beta^3 + pc beta^4 + inst beta^5 (generation/prog.rs:149-156), and the permuted pair. */
#define OLA_TABLEGEN_REFERENCE_QUIRKS 1u
int32_t ola_generate_rc_trace(OlaCtx* ctx, const uint64_t* vals, const uint64_t* filters, size_t n_rows, uint32_t range_bits,
                              uint64_t* out, uint32_t* log_n_out);
int32_t ola_generate_bitwise_trace(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint32_t limb_bits, uint64_t beta, uint32_t flags,
                                   uint64_t* out, uint32_t* log_n_out);
int32_t ola_generate_prog_trace(OlaCtx* ctx, const uint64_t* exec, const uint64_t* prog, uint32_t log_n, uint64_t beta, uint64_t* out);

/* ---- the CPU table and the program table's executed side from step records -------------------------------------------------
 * Both tables are per-row functions of the executor's `Step`s (generation/cpu.rs:11-218 maps one Step to one row of 94 columns: 66
 * copied words and 28 that follow from them -- 19 opcode selectors, 7 flags and filters, IS_PADDING and the constant TX_IDX; the
 * executed side of generation/prog.rs:31-108 is a stream compaction of the same steps), so the host hands over the
 * records and neither assembles, zero-fills nor uploads the widest table of the proof.  The contract is the one of the calls above:
 * `steps`, `prog` and `out` may each be host memory or memory of the context's GPU, words may be >= p, every word written is
 * canonical, every column of `out` is written (no memset of the table), the work runs on the context's stream and is complete on
 * return, arguments are validated first, ctx == NULL answers OLA_E_NO_DEVICE on a machine without a HIP device, a multi-device
 * context works on its first device, and `out` can go into ola_prove_with_traces* as a resident table.
 *
 * A step record is OLA_CPU_STEP_WORDS = 66 words per executed row, column-major 66 x n_steps:
 *   words 0 .. 64 = CPU columns 1 .. 65 (COL_ENV_IDX .. COL_IDX_STORAGE, then the 30 register-selector columns, cpu/columns.rs) --
 *     exactly the fields generation/cpu.rs:64-105 copies from a Step.  The selector columns travel as whole words because extension lines use
 *     them as data carriers (executor/src/lib.rs:165 the tape address, :1298-1312 the storage slot's addresses, key, value and tree
 *     key, :1937 the callee's context), which a bit mask cannot hold;
 *   word 65 = filter_tape_looking (generation/cpu.rs:146).
 *
 * ola_generate_cpu_trace: out = 94 x 2^log_n; 2^log_n < n_steps is OLA_E_INVALID_ARG.  Live rows follow generation/cpu.rs:62-179: TX_IDX = 0,
 *   the 65 copied columns, the opcode selector of generation/cpu.rs:20-60 (an opcode word that is none of the 25 masks sets none), IS_ENTRY_SC,
 *   IS_NEXT_LINE_DIFF_INST (ext_length == ext_cnt; TLOAD's ext_length op0 * op1 + (1 - op0) is computed in the field, the reference's
 *   u64 expression agrees wherever it does not overflow), IS_NEXT_LINE_SAME_TX, FILTER_TAPE_LOOKING, IS_SCCALL_EXT_LINE,
 *   IS_STORAGE_EXT_LINE, FILTER_SCCALL_END, FILTER_LOOKING_PROG_IMM; every comparison is on canonical values.  Rows n_steps .. 2^log_n
 *   are the padding rows of generation/cpu.rs:180-208 with INST and IDX_STORAGE of the last live row (2^20 and 0 when n_steps == 0).
 * ola_generate_prog_trace_steps: out = 18 x 2^log_n.  prog: the listing side, 7 x 2^log_n, as ola_generate_prog_trace takes it.  The
 *   executed side follows generation/prog.rs:31-44,59-108: a step with is_ext_line == 1 gives nothing, every other step the row (addr_code, pc,
 *   inst, filter 1) and, when op1_imm == 1 or the opcode is MLOAD or MSTORE, a second row (addr_code, pc + 1, imm_val, filter 1).
 *   *exec_rows_out receives the number of executed rows; more than 2^log_n is OLA_E_INVALID_ARG with the count still returned and
 *   `out` untouched, so that one call sizes the table.  n_steps >= 2^31 is OLA_E_INVALID_ARG.  Rows beyond the executed ones repeat
 *   executed row 0 with filter 0 (a listed word, so that the in-table lookup holds); with OLA_TABLEGEN_ZERO_FILLER, or when nothing
 *   was executed, they are generation/prog.rs:57's zero rows.  The rest is ola_generate_prog_trace. */
#define OLA_CPU_STEP_WORDS 66
#define OLA_TABLEGEN_ZERO_FILLER 1u
int32_t ola_generate_cpu_trace(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, uint32_t log_n, uint64_t* out);
int32_t ola_generate_prog_trace_steps(OlaCtx* ctx, const uint64_t* steps, size_t n_steps, const uint64_t* prog, uint32_t log_n,
                                      uint64_t beta, uint32_t flags, uint64_t* out, uint64_t* exec_rows_out);

/* ---- the memory table from raw cells, the comparison table from operand pairs ------------------------------------------------
 * The memory table is not a per-row function of the executor's records: it is a sort of the memory cells by (address, clock), per-row
 * differences against the predecessor row, one field inversion per row, the padding rows of the prophet region and the two value lists
 * the table sends to the range-check table (generation/memory.rs:5-153).  The comparison table is the other table whose rows need an
 * inversion each (generation/builtin.rs:208-247).  Both are made on the device; with them three of the four segments of
 * ola_generate_rc_trace's `vals` are in HBM already.  The contract is the one of the "whole derived tables" block above: every buffer
 * may be host memory or memory of the context's GPU, words may be >= p, every word written is canonical, every column of `out` is
 * written (no memset of the table), the work runs on the context's stream and is complete on return, arguments are validated first,
 * out == NULL is a sizing call that also takes ctx == NULL (*log_n_out is set; rc_counts must be there all the same and is left
 * alone), ctx == NULL in a call that would do work is OLA_E_NO_DEVICE on a machine without a HIP device and OLA_E_INVALID_ARG
 * otherwise, a multi-device context works on its first device, and `out` can go into ola_prove_with_traces* as a resident table.
 *
 * ola_generate_memory_trace: out = 29 x n, n = next_pow2(max(n_cells + 1, 8)), log2 n in *log_n_out.
 *   cells: OLA_MEM_CELL_WORDS = 5 words per cell, column-major 5 x n_cells, in any order: address, clock, op (the opcode's one-hot
 *     word, as COL_MEM_OP holds it), value, is_write.  n_cells >= 2^31 is OLA_E_INVALID_ARG.
 *   Row order: ascending in the key (canonical address, canonical clock, op rank, canonical value, canonical is_write); the op rank is
 *     the op's position in CALL, MLOAD, MSTORE, POSEIDON, RET, SLOAD, SSTORE, TLOAD, TSTORE; an op word that is none of the nine ranks
 *     behind them, ordered by its canonical word, and sets no selector.  Cells equal in all five are indistinguishable, so the table
 *     does not depend on the order of `cells`.
 *   Live rows: IS_RW, the five words, the op's selector; for an address >= ADDR_HEAP_PTR (memory/memory_stark.rs:81) REGION_HEAP,
 *     DIFF_ADDR_COND = 0 - (2^32 - 1) - address and FILTER_LOOKING_RC_COND.  The first heap row behind a non-heap row gets DIFF_ADDR
 *     and DIFF_ADDR_INV only (generation/memory.rs:77-86); every other row but the first gets DIFF_ADDR, DIFF_ADDR_INV, DIFF_CLK (on an
 *     unchanged address), RW_ADDR_UNCHANGED, RC_VALUE (the clock difference on an unchanged address, else the address difference) and
 *     FILTER_LOOKING_RC.  The inverse of 0 is 0.
 *   Padding rows: prophet-region rows from address p - (2^32 - 1) upwards (S_PROPHET, IS_WRITE, REGION_PROPHET, DIFF_ADDR_COND =
 *     RC_VALUE = 0 - address); the first takes DIFF_ADDR against the last live address, the others have 1.  A table without cells has
 *     one stack-region row first that carries S_PROPHET and IS_WRITE only (include/ola_tracegen.h says why).
 *   flags: OLA_TABLEGEN_REFERENCE_QUIRKS with n_cells == 0 gives generation/memory.rs:95-153's table as it is (every row a prophet row,
 *     row 0 without selector and address step); the flag is ignored when there are cells.
 *   rc_counts (not NULL) receives {number of range-checked sort values, number of range-checked region values}.  rc_out may be NULL;
 *     otherwise it has room for 2 n_cells words and receives RC_VALUE of the rows with FILTER_LOOKING_RC in row order, immediately
 *     followed by DIFF_ADDR_COND of the heap rows in row order -- the order in which they follow the CPU's and the comparison table's
 *     values in the range-check table, so a caller points rc_out into its `vals` buffer and copies nothing.  Words of rc_out beyond
 *     rc_counts[0] + rc_counts[1] are not written.
 * ola_generate_cmp_trace: out = 6 x n, n = next_pow2(n_ops), at least 2.  ops: column-major 2 x n_ops (op0, op1); n_ops >= 2^31 is
 *   OLA_E_INVALID_ARG.  Live rows: canonical OP0 and OP1, GTE = op0 >= op1, ABS_DIFF, ABS_DIFF_INV (0 for 0), FILTER_LOOKING_RC = 1;
 *   padding rows: OP0 = GTE = ABS_DIFF = ABS_DIFF_INV = 1, the rest 0.  abs_diff_out may be NULL; otherwise it has room for n_ops
 *   words and receives ABS_DIFF of the live rows in order. */
#define OLA_MEM_CELL_WORDS 5
int32_t ola_generate_memory_trace(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint32_t flags, uint64_t* out, uint32_t* log_n_out,
                                  uint64_t* rc_out, uint64_t rc_counts[2]);
int32_t ola_generate_cmp_trace(OlaCtx* ctx, const uint64_t* ops, size_t n_ops, uint64_t* out, uint32_t* log_n_out, uint64_t* abs_diff_out);

/* ---- the account-storage tree, the storage-access table and the Poseidon table ---------------------------------------------------
 * What is left of trace generation on the host after the calls above is mostly Poseidon hashing for the account-storage tree: a write
 * is 256 permutations, and every access contributes 512 rows -- the hash of every level in the tree after and before the access -- to
 * the Poseidon table (builtins/storage/storage_access_stark.rs:110-334, generation/storage.rs:7-123).  A batch of accesses is
 * 2 x 256 x n_access independent permutations per tree level with a dependency only from one level to the next, so the device hashes
 * the tree, one launch per level, and writes the storage table and the Poseidon table's inputs; a second call turns those inputs into
 * the 134-column table.  The contract is the one of the "whole derived tables" block above: every buffer may be host memory or memory
 * of the context's GPU, words may be >= p, every word written is canonical, every column of `out` is written (no memset of the
 * table), the work runs on the context's stream and is complete on return, arguments are validated first, out == NULL is a sizing
 * call that also takes ctx == NULL, ctx == NULL in a call that would do work is OLA_E_NO_DEVICE on a machine without a HIP device and
 * OLA_E_INVALID_ARG otherwise, a multi-device context works on its first device, and `out` can go into ola_prove_with_traces* as a
 * resident table.
 *
 * ola_generate_storage_trace: out = 48 x n, n = next_pow2(max(256 m, 8)) with m the number of accesses without OLA_STORAGE_SILENT, log2 n
 *   in *log_n_out.
 *   accesses: OLA_STORAGE_ACCESS_WORDS = 14 words per access, column-major 14 x n_access, in execution order: words 0..3 the tree key,
 *     4..7 `value` (the leaf after a write), 8..11 `pre_value` (used only with `siblings`), 12 flags, 13 psdn_row (the Poseidon-table row
 *     of this access's first hash).  n_access >= 2^23 and a flag bit nobody defined are OLA_E_INVALID_ARG.  The flags and psdn_row words
 *     are read by the host before any work (one copy when the records are in HBM).  In a sizing call `accesses` may be NULL: no access is
 *     then taken to be silent.
 *   The tree: 256 levels, the key's bits (most significant limb first) choose the child, an inner node is
 *     Poseidon(left || right || 0,0,0,0)[0..4], the lowest level hashes the two 4-word values with capacity word 1, untouched leaves are
 *     zero.  The hash is Poseidon whatever the context's hasher, because the AIR's is.
 *   siblings == NULL, the self-contained batch: the tree is empty before access 0.  The sibling of access i at layer L is the layer-L node
 *     of the latest access j < i whose key shares exactly L - 1 leading bits with key i (silent accesses included), the empty tree's node
 *     if there is none; the leaf before access i is the value left by the latest write j < i of the same key, zero otherwise.  A read
 *     leaves the leaf as it is: its `value` words and every `pre_value` are ignored.
 *   siblings != NULL, for a host with a persistent tree of its own: 1024 x n_access column-major, word w of layer L of access a at
 *     ((L - 1) * 4 + w) * n_access + a.  `pre_value` is the leaf before the access and `value` the leaf after it (for a read the caller
 *     passes the same words twice: the call copies and does not compare).  OLA_STORAGE_SILENT is OLA_E_INVALID_ARG.  The accesses are
 *     independent of each other; that one access's tree is the next one's is the caller's business (ola_check_constraints localises a
 *     break).
 *   out: 256 rows per access with rows, layer 1 (the root side) first, accesses in order; the columns of generation/storage.rs:23-82:
 *     ACCESS_IDX counts from 1 over the accesses with rows, ADDR_ACC = limb (L - 1) / 64 of the key shifted right by 63 - (L - 1) % 64,
 *     FILTER_IS_FOR_PROG on the layer-256 row of an access with OLA_STORAGE_FOR_PROG.  Padding rows (generation/storage.rs:84-114):
 *     IS_PADDING = 1, ROOT = the last live row's root, the rest 0; m == 0 gives the all-padding table with zero roots.
 *   psdn_inputs / psdn_filters: NULL together, or the 12 x psdn_stride and 4 x psdn_stride column-major input buffers of
 *     ola_generate_poseidon_table, both in host memory or both on the device.  For every access with rows, layer L and version v (0 = the
 *     tree after the access, 1 = before) the call writes row psdn_row + 2 (L - 1) + v -- StorageTree::access's order: the permutation's
 *     twelve inputs (the children in bit order, the capacity word L == 256, then 0, 0, 0) and the filters (0, 0, L == 256, L != 256).
 *     psdn_row + 512 > psdn_stride is OLA_E_INVALID_ARG, checked before any work.  Rows the call does not own keep what they hold (a host
 *     buffer travels to the device and back whole); two accesses must not claim the same rows.
 *   roots_out: NULL, or 8 words: 0..3 the root before the first access with rows (the root after the last access when none has rows),
 *     4..7 the root after the last access; with n_access == 0 both are the empty tree's root.  The generators' program-table challenge
 *     needs both (generation/prog.rs:23-29).
 *   The work: a resolver (self-contained mode: one thread per access scans the earlier ones, O(n_access^2) pair steps), 256 launches of
 *     one thread per (access, version), one launch that fills the remaining columns and the padding.
 * ola_generate_poseidon_table: out = 134 x n, n = next_pow2(max(n_rows, 8)), log2 n in *log_n_out.  inputs: 12 x stride column-major,
 *   filters: 4 x stride or NULL for zeros, stride >= n_rows (a smaller one and n_rows > 2^26 are OLA_E_INVALID_ARG); rows n_rows .. n are
 *   the rows of all-zero inputs (generation/poseidon.rs's POSEIDON_ZERO_HASH rows).  The rows are ola_generate_poseidon_trace's. */
#define OLA_STORAGE_ACCESS_WORDS 14
#define OLA_STORAGE_WRITE 1u      /* flags word, bit 0 */
#define OLA_STORAGE_FOR_PROG 2u   /* bit 1: a program-hash read (generation/storage.rs:74-80) */
#define OLA_STORAGE_SILENT 4u     /* bit 2: a write that establishes the tree before the run and emits no rows */
int32_t ola_generate_storage_trace(OlaCtx* ctx, const uint64_t* accesses, size_t n_access, const uint64_t* siblings,
                                   uint64_t* out, uint32_t* log_n_out,
                                   uint64_t* psdn_inputs, uint64_t* psdn_filters, size_t psdn_stride,
                                   uint64_t roots_out[8]);
int32_t ola_generate_poseidon_table(OlaCtx* ctx, const uint64_t* inputs, const uint64_t* filters, size_t n_rows, size_t stride,
                                    uint64_t* out, uint32_t* log_n_out);

/* ---- the tape, Poseidon-chunk and program-chunk tables ---------------------------------------------------------------------------
 * The narrow tables that were still assembled on the host.  None needs hashing the host has not done: every hash they hold is an
 * output word of a row of the Poseidon table that ola_generate_poseidon_table leaves resident (inputs in its columns 4..15, outputs in
 * 16..27), so a row is a gather -- thread = row, every column stored along rows.  The contract is the one of the "whole derived tables"
 * block above: every buffer may be host memory or memory of the context's GPU, words may be >= p, every word written is canonical,
 * every column of `out` is written (no memset of the table), the work runs on the context's stream and is complete on return,
 * arguments are validated first, out == NULL is a sizing call that also takes ctx == NULL, ctx == NULL in a call that would do work is
 * OLA_E_NO_DEVICE on a machine without a HIP device and OLA_E_INVALID_ARG otherwise, a multi-device context works on its first device,
 * and `out` can go into ola_prove_with_traces* as a resident table.  (The SCCALL table has no entry point: the executor produces no
 * cross-contract call, so it is the 26 x 8 padding table.)
 *
 * ola_generate_tape_trace (builtins/tape/tape_stark.rs:44-143): out = 6 x n, n = next_pow2(max(n_cells, 8)), log2 n in *log_n_out.
 *   cells: OLA_TAPE_CELL_WORDS = 3 words per cell, column-major 3 x n_cells, in execution order: the tape address, the opcode's one-hot
 *     word, the value.  n_cells >= 2^31 is OLA_E_INVALID_ARG.
 *   Rows ascend in the canonical address; cells of one address keep execution order (a stable radix sort of (address, 32-bit index)
 *   over the bits the addresses use).  Live rows: OPCODE, ADDR, VALUE, FILTER_LOOKED = 1, TX_IDX = IS_INIT_SEG = 0; padding rows repeat
 *   the last sorted cell's address and value with the TLOAD mask and filter 0; no cells: every row a TLOAD of address 0, value 0.
 *   Host waits: three.  One after the key pass, for the OR of the addresses that sizes the sort (all zero: no sort); one before the
 *   sort's work space goes back to the pool, which another thread's call on another stream could take at once; one at the end,
 *   behind the copy to a host `out`, because the table is complete on return (the stream is idle by then when `out` is device memory).
 * ola_generate_poseidon_chunk_trace (generation/poseidon_chunk.rs): out = 53 x n, n = next_pow2(max(rows, 8)), rows = the sum of
 *   1 + len / 8 over the calls, log2 n in *log_n_out.
 *   calls: OLA_POSEIDON_CALL_WORDS = 5 words per POSEIDON instruction, column-major 5 x n_calls, in execution order: clk, src, len, dst,
 *     psdn_row (the Poseidon-table row of the call's first block; block j is row psdn_row + j).
 *   poseidon_table: 134 x 2^psdn_log_n column-major (3 <= psdn_log_n <= 26); may be NULL in a sizing call.
 *   A call gives a header row (OP0 = src, FILTER_LOOKED_CPU = 1) and len / 8 extension rows; extension row j has OP0 = src + 8 j,
 *   ACC_CNT = 8 (j + 1), VALUE = inputs 0..7 of table row psdn_row + j, CAP = inputs 8..11, HASH = its twelve outputs, IS_EXT_LINE = 1,
 *   IS_RESULT_LINE on the last one, the eight memory filters and the Poseidon filter; both kinds carry CLK, OPCODE = the POSEIDON mask,
 *   OP1 = len, DST.  Row offsets are an exclusive scan over 1 + len / 8.  Padding rows: IS_PADDING_LINE = 1, the rest 0.
 *   The host reads the len and psdn_row words once before any work (one copy when the records are in HBM; also in a sizing call):
 *   len == 0, len % 8 != 0, psdn_row + len / 8 > 2^psdn_log_n (checked when the table is given), n_calls >= 2^26 and more than 2^26 rows
 *   are OLA_E_INVALID_ARG.
 *   Host waits: three, two without calls.  That read (it sizes the table and keeps every gather inside the Poseidon table; a
 *   blocking copy when the records are in HBM), one before the scan's work space goes back to the pool, and the one at the end, behind
 *   the copy to a host `out`.
 * ola_generate_prog_chunk_trace (generation/prog.rs, program/prog_chunk_stark.rs): out = 40 x n, n = next_pow2(max(n_words / 8, 8)),
 *   log2 n in *log_n_out.
 *   words: the zero-padded listing, n_words words; code_addr: 4 words; poseidon_table as above, whose row i hashed words 8 i .. 8 i + 7
 *   (may be NULL in a sizing call).
 *   Row i: CODE_ADDR, START_PC = 8 i, INST = the eight words, CAP = inputs 8..11 of table row i, HASH = its twelve outputs, IS_FIRST_LINE
 *   on row 0, IS_RESULT_LINE on the last row with OLA_PROG_CHUNK_RESULT_LINE, the eight looking filters 1.  Padding rows:
 *   IS_PADDING_LINE = 1, the rest 0.  n_words % 8 != 0, n_words / 8 > 2^psdn_log_n, n_words > 2^29 and a flag bit nobody defined are
 *   OLA_E_INVALID_ARG.
 *   Host waits: one, at the end (code_addr in HBM adds a 32-byte copy before the launch). */
#define OLA_TAPE_CELL_WORDS 3
#define OLA_POSEIDON_CALL_WORDS 5
#define OLA_PROG_CHUNK_RESULT_LINE 1u
int32_t ola_generate_tape_trace(OlaCtx* ctx, const uint64_t* cells, size_t n_cells, uint64_t* out, uint32_t* log_n_out);
int32_t ola_generate_poseidon_chunk_trace(OlaCtx* ctx, const uint64_t* calls, size_t n_calls, const uint64_t* poseidon_table,
                                          uint32_t psdn_log_n, uint64_t* out, uint32_t* log_n_out);
int32_t ola_generate_prog_chunk_trace(OlaCtx* ctx, const uint64_t* words, size_t n_words, const uint64_t* code_addr, uint32_t flags,
                                      const uint64_t* poseidon_table, uint32_t psdn_log_n, uint64_t* out, uint32_t* log_n_out);

/* ---- from the executor's records to the twelve tables, and to proof bytes -------------------------------------------------------
 * One call composes the generators above, so that a host restates none of it: their order, the range-check value buffer the
 * comparison and memory calls share with the CPU's values, the range-check filters, the Poseidon row numbering and the two compress
 * challenges.  OlaExecRecords is what the executor recorded -- what the native generator hands out under OLA_TRACEGEN_RECORDS_ONLY
 * (include/ola_tracegen.h).  `size` is sizeof(OlaExecRecords) as the caller compiled it, so that the struct can grow; every pointer may
 * be host memory or memory of the context's GPU (a device buffer must be complete when the call is made), and may be NULL where its
 * count is 0.
 *   steps / n_steps / cpu_log_n: ola_generate_cpu_trace's; prog_listing / prog_log_n: the listing side of ola_generate_prog_trace_steps
 *   mem_cells, cmp_ops, cpu_rc (the values of the RC instructions), bitwise_ops (5 x n: filter, tag, op0, op1, res), accesses with
 *   optional siblings, tape_cells, psdn_calls, listing_words / code_addr: as the generators take them
 *   psdn_inputs / psdn_filters: 12 x psdn_stride and 4 x psdn_stride with the accesses' rows free, psdn_rows <= psdn_stride live rows;
 *     the call works on copies, the caller's buffers are not written
 *   range_bits, limb_bits: of the AIR set's fixed tables (16 and 8 in the reference)
 *   flags: OLA_RECORDS_REFERENCE_QUIRKS (the bitwise and memory generators' OLA_TABLEGEN_REFERENCE_QUIRKS), OLA_RECORDS_ZERO_FILLER
 *     (OLA_TABLEGEN_ZERO_FILLER), OLA_RECORDS_RESULT_LINE (OLA_PROG_CHUNK_RESULT_LINE), OLA_RECORDS_EXPLICIT_BETAS: bitwise_beta and
 *     program_beta are taken as given; without it both are drawn inside the call by the host challenger, the bitwise one from the
 *     twelve limb columns of the operations (generation/builtin.rs:120-131), the program one from the storage call's two roots
 *     (generation/prog.rs:23-29)
 * ola_tables_from_records makes all twelve tables resident, in pool memory of the context's (first) device, each at its generator's own
 * height: the storage tree with the Poseidon inputs, the Poseidon table, the two chunk tables, the comparison and memory tables with
 * their value lists behind the CPU's, the four range-check filter columns from the four segment lengths (one fill kernel), then the
 * range-check, CPU, tape, SCCALL (the 26 x 8 padding table), bitwise and program tables.  A failure returns the failing generator's
 * code with its message behind the name of the step ("CPU table: ..."), and frees everything the call took.
 * ola_tables_get: the twelve device pointers and heights in `enum Table` order, params[2] = (bitwise, program) challenge and the
 * twelve compress_challenges -- what ola_check_constraints, ola_check_lookup and ola_prove_with_traces take.  ola_tables_free returns
 * the memory to the context's pool (before ola_gpu_free).
 * ola_prove_from_records: the tables, ola_prove_with_traces on them, the set freed; the too-small buffer and ola_take_pending_proof
 * behave as there.  No table crosses the link. */
#define OLA_RECORDS_REFERENCE_QUIRKS 1u
#define OLA_RECORDS_ZERO_FILLER 2u
#define OLA_RECORDS_RESULT_LINE 4u
#define OLA_RECORDS_EXPLICIT_BETAS 8u
typedef struct OlaExecRecords {
    uint32_t size;
    uint32_t flags;
    uint32_t cpu_log_n;
    uint32_t prog_log_n;
    uint32_t range_bits;
    uint32_t limb_bits;
    const uint64_t* steps;
    uint64_t n_steps;
    const uint64_t* prog_listing;
    const uint64_t* mem_cells;
    uint64_t n_mem_cells;
    const uint64_t* cmp_ops;
    uint64_t n_cmp_ops;
    const uint64_t* cpu_rc;
    uint64_t n_cpu_rc;
    const uint64_t* bitwise_ops;
    uint64_t n_bitwise_ops;
    const uint64_t* accesses;
    uint64_t n_access;
    const uint64_t* siblings;
    const uint64_t* psdn_inputs;
    const uint64_t* psdn_filters;
    uint64_t psdn_stride;
    uint64_t psdn_rows;
    const uint64_t* tape_cells;
    uint64_t n_tape_cells;
    const uint64_t* psdn_calls;
    uint64_t n_psdn_calls;
    const uint64_t* listing_words;
    uint64_t n_listing_words;
    uint64_t code_addr[4];
    uint64_t bitwise_beta;
    uint64_t program_beta;
} OlaExecRecords;
typedef struct OlaTableSet OlaTableSet;
int32_t ola_tables_from_records(OlaCtx* ctx, const OlaExecRecords* rec, OlaTableSet** out);
int32_t ola_tables_get(const OlaTableSet* set, const uint64_t* ptrs[12], uint32_t log_n[12], uint64_t params[2], uint64_t compress[12]);
int32_t ola_tables_free(OlaTableSet* set);
int32_t ola_prove_from_records(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const OlaExecRecords* rec, uint8_t* out,
                               size_t cap, size_t* out_len);

/* ---- verification: proof bytes to a verdict ------------------------------------------------------------------------------------
 * ola_verify_all_proof is the reference's `verify_proof` (circuits/src/stark/verifier.rs:35) for the context's configuration: the
 * hasher of the Merkle trees and the transcript is the context's (every OLA_HASH_*, the proof-of-work hasher as in ola_pow), the
 * FRI parameters are the context's OlaGpuConfig.  In the reference's order: get_challenges, CtlCheckVars::from_proofs, then per
 * table validate_proof_shape, eval_vanishing_poly over the extension field at zeta, the quotient identity and plonky2's
 * verify_fri_proof, and verify_cross_table_lookups last.
 * The sequential part -- reading the bytes, the transcript, the constraints at zeta, the proof of work, the lookup products -- runs
 * on the host; every Merkle path (one per table, query and oracle, one per table, query and FRI layer) and the FRI algebra of
 * every (table, query) run on the device: one upload, two kernel launches and one read-back of flags per call, whatever the
 * number of tables, queries and layers (olavm_amd/csrc/verify_host.h, verify.hip).
 * airset: as for ola_prove_with_traces.  params: the concatenated per-table constraint parameters as for ola_prove_with_traces, or
 *   NULL: every parameter of table t is then the proof's compress_challenges[t], as the reference's verifier takes them.
 * proof: AllProof in the reference wire format (serialization.rs read_all_proof), what ola_prove_with_traces* and
 *   ola_prove_from_records write.
 * Returns OLA_OK when verification RAN: the verdict is in *report, a rejected proof is not an error.  OLA_E_INVALID_ARG: a NULL
 * argument, a malformed AIR-set blob, or a multi-device context (as the per-phase entry points refuse one); OLA_E_NO_DEVICE without
 * a HIP device (no context can exist then; there is no CPU fallback).
 * When several checks fail, the report names the one the reference reaches first: tables in order; within a table its shape, the
 * quotient identity, the proof of work, then the queries in order; within a query the initial trees in oracle order (trace, Zs,
 * quotient), then per FRI layer the consistency check before that layer's Merkle path, then the final polynomial; the lookup
 * products last.
 * A field word >= p anywhere in the proof is refused as OLA_VERIFY_MALFORMED: an honest serializer never writes one
 * (serialization.rs:50-52), what the reference does with such a word is not defined by its wire format, and the kernels may then
 * assume canonical input.  The words of a Blake3 digest are bytes, not field elements, and may take any value.
 * Leaves are hashed by the rule of this library's commitments: hash_no_pad of the row for every width, rows of four words or fewer
 * included, as MerkleTree::new_v2 (hash/merkle_tree/mod.rs:180-266) and verify_merkle_proof_to_cap (hash/merkle_proofs.rs:51-80) hash them in
 * the reference; Blake3_256 / KeccakHash<25> of the canonical little-endian words under OLA_HASH_BLAKE3 / OLA_HASH_KECCAK. */
#define OLA_VERIFY_OK 0u
#define OLA_VERIFY_MALFORMED 1u                 /* truncated, trailing bytes, a word >= p, wrong number of table proofs        */
#define OLA_VERIFY_EMPTY_FRI 2u                 /* no query round or no initial tree to take the degree from                   */
#define OLA_VERIFY_SHAPE_OPENING_WIDTH 3u       /* validate_proof_shape: local_values / next_values                            */
#define OLA_VERIFY_SHAPE_ZS_WIDTH 4u            /*   permutation_ctl_zs / permutation_ctl_zs_next                              */
#define OLA_VERIFY_SHAPE_CTL_ZS_LAST_WIDTH 5u   /*   ctl_zs_last                                                               */
#define OLA_VERIFY_SHAPE_QUOTIENT_WIDTH 6u      /*   quotient_polys                                                            */
#define OLA_VERIFY_QUOTIENT_IDENTITY 7u         /* verifier.rs:295 "Mismatch between evaluation and opening of quotient polynomial" */
#define OLA_VERIFY_SHAPE_CAP_HEIGHT 8u          /* validate_fri_proof_shape (fri/validate_shape.rs:11-67): a commit-phase cap  */
#define OLA_VERIFY_SHAPE_QUERY_ROUNDS 9u        /*   number of query rounds                                                    */
#define OLA_VERIFY_SHAPE_INITIAL_PROOFS 10u     /*   number of initial trees of a query                                        */
#define OLA_VERIFY_SHAPE_LEAF_LEN 11u           /*   width of an opened row                                                    */
#define OLA_VERIFY_SHAPE_INITIAL_PATH_LEN 12u   /*   length of an initial tree's Merkle path                                   */
#define OLA_VERIFY_SHAPE_STEPS 13u              /*   number of FRI layers of a query (or of commit-phase caps)                 */
#define OLA_VERIFY_SHAPE_EVALS_LEN 14u          /*   a layer's coset                                                           */
#define OLA_VERIFY_SHAPE_STEP_PATH_LEN 15u      /*   length of a layer's Merkle path                                           */
#define OLA_VERIFY_SHAPE_FINAL_POLY_LEN 16u     /*   the final polynomial                                                      */
#define OLA_VERIFY_POW 17u                      /* fri/verifier.rs:59-73 "Invalid proof of work witness."                      */
#define OLA_VERIFY_MERKLE_INITIAL 18u           /* merkle_proofs.rs:71 for an initial tree; oracle_or_layer = 0 trace, 1 Zs, 2 quotient */
#define OLA_VERIFY_FRI_CONSISTENCY 19u          /* fri/verifier.rs:218: a layer's evals[x_index within coset] is not the folded value; oracle_or_layer = layer */
#define OLA_VERIFY_MERKLE_COMMIT 20u            /* merkle_proofs.rs:71 for a commit-phase tree; oracle_or_layer = layer        */
#define OLA_VERIFY_FINAL_POLY 21u               /* "Final polynomial evaluation is invalid."                                   */
#define OLA_VERIFY_CTL 22u                      /* cross_table_lookup.rs:551-584 "Cross-table lookup verification failed."      */
typedef struct OlaVerifyReport {
    uint32_t accepted;          /* 1 / 0                                                                                      */
    uint32_t reason;            /* OLA_VERIFY_*                                                                               */
    int32_t table;              /* where the reference stops; -1 where it does not apply                                      */
    int32_t query;
    int32_t oracle_or_layer;
    uint32_t merkle_jobs;       /* Merkle paths checked on the device                                                         */
    uint32_t query_jobs;        /* (table, query) pairs whose FRI algebra ran on the device                                   */
    uint32_t kernel_launches;   /* 2, or 0 when the host stage refused the proof before any table reached the device          */
    double host_ms;             /* the host stage: reading, transcript, constraints at zeta, image                            */
    double device_ms;           /* upload, the two kernels, read-back (wall clock around the stream)                          */
    char message[96];           /* starts with the reason in words, NUL-terminated                                            */
} OlaVerifyReport;
int32_t ola_verify_all_proof(OlaCtx* ctx, const uint64_t* airset, size_t airset_words, const uint64_t* params, const uint8_t* proof,
                             size_t proof_len, OlaVerifyReport* report);
/* The counterpart of ola_open_and_prove: verifies an opening set and its FRI proof (write_opening_set || write_fri_proof, the bytes
 * ola_open_and_prove returns) against the three commitments' caps, continuing the caller's transcript.  caps: 3 x 2^cap_height x 4
 * words (trace, Zs, quotient); num_polys: the three commitments' widths; degree_bits: log2 of the trace length.  *challenger must
 * stand where the prover's stood when it called ola_open_and_prove; when the proof is accepted it is left where the prover's
 * stands afterwards, otherwise it is unchanged.  table is -1 in the report.  Everything else as above; an opening set whose widths
 * are not the instance's is refused with the OLA_VERIFY_SHAPE_* reason of its vector. */
int32_t ola_verify_opening(OlaCtx* ctx, const uint64_t* caps, const uint32_t num_polys[3], uint32_t degree_bits,
                           uint32_t num_permutation_zs, const uint8_t* proof, size_t proof_len, OlaChallenger* challenger,
                           OlaVerifyReport* report);

/* ---- coset-partitioned proving over several GPUs ---------------------------------------------------------
 * One process per GPU; every process calls ola_prove_with_traces with the SAME traces.  Because the transcript is a
 * function of the (identical) commitments, all ranks draw the same challenges without talking to each other; only the
 * heavy work is divided.  For every table with at least 2^12 rows, rank r uploads 1/world of the columns (the values are
 * all-gathered device to device: xGMI instead of `world` copies over PCIe), extends and hashes cosets
 * [r*8/world, (r+1)*8/world) of all three commitments, and evaluates the quotient on those of its cosets that belong to the
 * quotient domain (the first 2^qdb cosets; all of them for the CPU, memory and Poseidon tables); it evaluates its 1/world of the
 * COLUMNS at the opening points, and extends / hashes its cosets of the first FRI layer.  The exchanges go through `all_gather`,
 * twelve per table -- the trace values (8n bytes per column, once), Merkle cap slices of the three commitments and of the first
 * FRI layer (512 B per tree), the two planes of quotient values (16 * 8n bytes per table), the opening values (a few KB), the
 * opened rows and paths of the 28 queries in the three commitments and in the first FRI layer -- and every rank ends up with the
 * complete, identical AllProof bytes.
 * all_gather(user, send_dev, recv_dev, bytes): gather `bytes` bytes of DEVICE memory from every rank into recv_dev in rank
 * order (world * bytes); return 0 when recv_dev is complete (or, with OLA_SHARD_STREAM_ORDERED, when the collective has been
 * enqueued on the context's stream).  world must be 1, 2, 4 or 8; world = 1 (or a NULL callback) restores single-GPU proving. */
typedef int32_t (*ola_all_gather_fn)(void* user, const void* send_dev, void* recv_dev, size_t bytes);
int32_t ola_set_shard(OlaCtx* ctx, uint32_t rank, uint32_t world, ola_all_gather_fn all_gather, void* user);
/* OLA_SHARD_STREAM_ORDERED: the callback enqueues the collective on the context's stream (ola_gpu_get_stream) -- RCCL launched
 * on that stream -- so the library neither synchronises before the call nor needs the result on return; without the flag the
 * library drains its stream before the call and expects recv_dev complete on return (host-staged collectives). */
#define OLA_SHARD_STREAM_ORDERED 1u
int32_t ola_set_shard_options(OlaCtx* ctx, uint32_t flags);
/* The hipStream_t all of the context's device work is issued on (the one given to ola_gpu_init, or the context's own). */
int32_t ola_gpu_get_stream(OlaCtx* ctx, void** stream_out);

/* Which tables of `airset` have an ahead-of-time specialised constraint-quotient kernel in this build (the counterpart of
 * the reference compiling each table's eval_packed_generic, e.g. cpu/cpu_stark.rs:325): has_kernel[t] = 1 or 0 for every
 * table.  Tables without one are proven with the generic interpreter kernel -- same bytes, fewer points per second.
 * The environment variable OLA_AIR_KERNELS=interpreter disables the specialised kernels, =crosscheck runs both and fails
 * with OLA_E_INTERNAL if they disagree (test hooks). */
int32_t ola_air_kernels_available(const uint64_t* airset, size_t airset_words, uint8_t* has_kernel, size_t ntables);
/* The same for a context created with `cfg` (NULL: the defaults, i.e. ola_air_kernels_available): a kernel is generated for one
 * num_challenges, so the answer depends on it.  Host only; OLA_E_INVALID_ARG for a configuration ola_gpu_init would refuse. */
int32_t ola_air_kernels_available_cfg(const OlaGpuConfig* cfg, const uint64_t* airset, size_t airset_words, uint8_t* has_kernel,
                                      size_t ntables);

#ifdef __cplusplus
}
#endif
#endif /* OLA_GPU_H */
