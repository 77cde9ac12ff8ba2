//! `prove_with_traces` on the MI355X backend: the body the `hip` feature substitutes for the CPU prover's
//! (circuits/src/stark/prover.rs:79-327).  Drop into `circuits/src/stark/hip_prover.rs`.
//!
//! One call crosses the boundary.  The twelve traces go in as they are -- `[Vec<PolynomialValues<F>>; NUM_TABLES]`, every column
//! its own `Vec<F>` (plonky2/field/src/polynomial/mod.rs:24-26), `F = GoldilocksField` = `repr(transparent) u64`
//! (goldilocks_field.rs:24-26): the shim hands the library one pointer per column (`ola_prove_with_traces_cols`) and copies
//! nothing.  The `AllProof` comes back in the reference's own wire format (`Buffer::write_all_proof`, serialization.rs:377-393)
//! and is decoded with `Buffer::read_all_proof` (:394-412).  The `timed!` scopes of the CPU prover come back with the GPU's
//! times and are replayed into the caller's `TimingTree`.  The executor / client path above (`client/src/main.rs:174-214`,
//! `circuits/benches/fibo_loop.rs:72-91`) does not change.  The hash configuration is the caller's `C`:
//! `PoseidonGoldilocksConfig`, `Blake3GoldilocksConfig` or `KeccakGoldilocksConfig`.
use std::any::type_name;
use std::ffi::CStr;
use std::sync::{Mutex, OnceLock};
use std::time::{Duration, Instant};

use anyhow::{bail, ensure, Result};
use plonky2::field::extension::Extendable;
use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::fri::reduction_strategies::FriReductionStrategy;
use plonky2::hash::hash_types::RichField;
use plonky2::plonk::config::GenericConfig;
use plonky2::util::timing::TimingTree;

use super::config::StarkConfig;
use super::ola_gpu_sys::*;
use super::ola_stark::{OlaStark, Table, NUM_TABLES};
use super::proof::{AllProof, PublicValues};
use super::serialization::Buffer;

/// The data form of `OlaStark`'s twelve `Stark` impls and `all_cross_table_lookups()` (stark/ola_stark.rs:29-64,122-560):
/// include/ola_airset.bin, staged by build.rs; little-endian u64 words.
static OLA_AIRSET_BYTES: &[u8] = include_bytes!(concat!(env!("OUT_DIR"), "/ola_airset.bin"));

fn airset() -> &'static [u64] {
    static WORDS: OnceLock<Vec<u64>> = OnceLock::new();
    WORDS.get_or_init(|| OLA_AIRSET_BYTES.chunks_exact(8).map(|c| u64::from_le_bytes(c.try_into().unwrap())).collect())
}

struct SendPtr(*mut OlaCtx);
unsafe impl Send for SendPtr {}

/// Start-up where the reference has it: `OlaStark::default()` calls `plonky2::field::cfft::ntt::init_gpu()`
/// (circuits/src/stark/ola_stark.rs:47, plonky2/field/src/cfft/ntt/mod.rs:53-99) before `prove()` generates the traces
/// (client/src/main.rs:191-200); the patch adds this call on the next line.  Returns at once: a helper thread inside the library
/// starts the HIP runtime, opens the device, loads the code objects, pins the upload ring and primes a context with a throw-away
/// proof of a small all-zero instance while the host generates traces; the first `with_ctx` waits for it and takes that context
/// over.  The hasher and the `StarkConfig` are not
/// known here (`OlaStark` is generic over `F, D` only) and are not needed.  Errors are left to the `ola_gpu_init` that follows.
pub fn init_early() {
    static ONCE: std::sync::Once = std::sync::Once::new();
    ONCE.call_once(|| {
        if check_abi().is_ok() {
            let words = airset();
            let _ = unsafe { ola_gpu_warmup(-1, OLA_WARMUP_PINNED_RING, words.as_ptr(), words.len()) };
        }
    });
}

/// What a context was created with: a later call with another `StarkConfig` gets a new context, not the stale one.
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
struct CtxKey {
    rate_bits: u32,
    cap_height: u32,
    proof_of_work_bits: u32,
    arity_bits: u32,
    final_poly_bits: u32,
    num_query_rounds: u32,
    num_challenges: u32,
    gpus: u32,
    /// `FriReductionStrategy` as `ola_gpu_set_fri_reduction` takes it: OLA_FRI_*, then its arguments
    strategy: u32,
    plan_n: u32,
    plan_args: [u32; 32],
}

/// One context per hash configuration for the life of the process, and ONE proof at a time on the GPU: a context is
/// thread-compatible, not re-entrant (the reference's own GPU state is process-wide behind a mutex as well:
/// cfft/ntt/mod.rs:14-17,48-50).  The slot is filled under its lock, so two threads that arrive together create one context,
/// not two (a second context would hold tens of GB of pooled HBM for nothing).  `OLA_GPUS` = 1, 2, 4 or 8: the context spans
/// that many devices and the partition and its exchanges happen inside the library (`OLA_COLLECTIVE` = peer | rccl selects who
/// moves the bytes).  The guard is held for the whole proof.
fn with_ctx<R>(hasher: u32, config: &StarkConfig, body: impl FnOnce(*mut OlaCtx) -> Result<R>) -> Result<R> {
    // one slot per OLA_HASH_* value, 0..=OLA_HASH_KECCAK (4 is unassigned and stays empty)
    static CTX: [OnceLock<Mutex<Option<(SendPtr, CtxKey)>>>; 6] =
        [OnceLock::new(), OnceLock::new(), OnceLock::new(), OnceLock::new(), OnceLock::new(), OnceLock::new()];
    let mut slot = CTX[hasher as usize].get_or_init(|| Mutex::new(None)).lock().unwrap_or_else(|e| e.into_inner());
    let fri = &config.fri_config;
    // all three variants (fri/reduction_strategies.rs:7-25); StarkConfig::standard_fast_config is ConstantArityBits(4, 5)
    // (config.rs:18-30), whose two numbers travel in OlaGpuConfig, the other two go through ola_gpu_set_fri_reduction
    let (mut arity_bits, mut final_poly_bits) = (4u32, 5u32);
    let (mut strategy, mut plan_n, mut plan_args) = (OLA_FRI_CONSTANT_ARITY_BITS, 0u32, [0u32; 32]);
    match fri.reduction_strategy {
        FriReductionStrategy::ConstantArityBits(a, f) => {
            arity_bits = a as u32;
            final_poly_bits = f as u32;
        }
        FriReductionStrategy::Fixed(ref layers) => {
            if layers.len() > plan_args.len() {
                bail!("the hip backend takes FriReductionStrategy::Fixed plans of at most 32 layers, the config has {}", layers.len());
            }
            strategy = OLA_FRI_FIXED;
            plan_n = layers.len() as u32;
            for (dst, &a) in plan_args.iter_mut().zip(layers.iter()) {
                *dst = a as u32;
            }
        }
        FriReductionStrategy::MinSize(max_arity_bits) => {
            strategy = OLA_FRI_MIN_SIZE;
            if let Some(m) = max_arity_bits {
                plan_n = 1;
                plan_args[0] = m as u32;
            }
        }
    }
    let key = CtxKey {
        rate_bits: fri.rate_bits as u32,
        cap_height: fri.cap_height as u32,
        proof_of_work_bits: fri.proof_of_work_bits,
        arity_bits,
        final_poly_bits,
        num_query_rounds: fri.num_query_rounds as u32,
        num_challenges: config.num_challenges as u32,
        gpus: std::env::var("OLA_GPUS").ok().and_then(|v| v.parse().ok()).unwrap_or(1),
        strategy,
        plan_n,
        plan_args,
    };
    if let Some((old, old_key)) = slot.as_ref() {
        if *old_key != key {
            // proving under the first call's FRI parameters would produce a proof the caller's verifier rejects
            check(unsafe { ola_gpu_free(old.0) })?;
            *slot = None;
        }
    }
    if slot.is_none() {
        init_early(); // a caller that never built an OlaStark::default(): the same start-up, then waited for below
        check_abi()?;
        let mut cfg: OlaGpuConfig = unsafe { std::mem::zeroed() };
        cfg.device = -1;
        cfg.rate_bits = key.rate_bits;
        cfg.cap_height = key.cap_height;
        cfg.proof_of_work_bits = key.proof_of_work_bits;
        cfg.fri_arity_bits = key.arity_bits;
        cfg.fri_final_poly_bits = key.final_poly_bits;
        cfg.num_query_rounds = key.num_query_rounds;
        cfg.num_challenges = key.num_challenges;
        cfg.hasher = hasher;
        let mut c = std::ptr::null_mut();
        check(unsafe { ola_gpu_init_multi(&cfg, std::ptr::null(), key.gpus, &mut c) })?;
        if key.strategy != OLA_FRI_CONSTANT_ARITY_BITS {
            // (a multi-device context refuses Fixed and MinSize: the error says so)
            if let Err(e) = check(unsafe { ola_gpu_set_fri_reduction(c, key.strategy, key.plan_args.as_ptr(), key.plan_n) }) {
                let _ = unsafe { ola_gpu_free(c) };
                return Err(e);
            }
        }
        *slot = Some((SendPtr(c), key));
    }
    body(slot.as_ref().unwrap().0 .0)
}

/// The `timed!` scopes of the proof that has just run, with the GPU's times (`ola_gpu_scope_times`), replayed into the
/// caller's tree under the names the CPU prover uses -- "compute trace commitments", "compute Zs commitment", "IFFT",
/// "FFT + blinding", "build Merkle tree", "compute quotient polys", "compute openings proof", "perform final FFT {n}",
/// "fold codewords in the commitment phase", "find proof-of-work witness" (prover.rs:111-553, fri/oracle.rs:56-90,221-225,
/// fri/prover.rs:41-58) -- so that `timing.print()` reads as it does for the CPU prover, one line per scope.  Only the
/// reference's scopes are replayed (the library's own grouping scopes, "table 3 prove_single_table", are skipped), at the depth
/// they have among themselves; `t0` is the host's clock when the call was made.  `TimingTree::record` is the one method the
/// patch adds to plonky2/plonky2/src/util/timing.rs (the tree's fields are private).
fn replay_scopes(c: *mut OlaCtx, timing: &mut TimingTree, t0: Instant) -> Result<()> {
    let mut n = 0u32;
    check(unsafe { ola_gpu_scope_times(c, -1, std::ptr::null_mut(), 0, &mut n) })?;
    if n == 0 {
        return Ok(());
    }
    let mut scopes: Vec<OlaScopeTime> = Vec::with_capacity(n as usize);
    check(unsafe { ola_gpu_scope_times(c, -1, scopes.as_mut_ptr(), n, &mut n) })?;
    unsafe { scopes.set_len(n as usize) };
    for s in scopes.iter().filter(|s| s.is_reference_scope != 0) {
        let name = unsafe { CStr::from_ptr(s.name.as_ptr()) }.to_string_lossy();
        timing.record(
            s.ref_depth as usize,
            &name,
            log::Level::Debug,
            t0 + Duration::from_secs_f64(s.start_ms * 1e-3),
            Duration::from_secs_f64(s.ms * 1e-3),
        );
    }
    Ok(())
}

/// `C::Hasher` -> OLA_HASH_*: the two configurations the reference instantiates the prover with
/// (client/src/main.rs:21,31: PoseidonGoldilocksConfig; circuits/benches/fibo_loop.rs:26: Blake3GoldilocksConfig), and the
/// fork's two Poseidon2 configurations, told apart by `C::InnerHasher` (plonk/config.rs:123-141: the proof-of-work hash).
fn hasher_of<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>() -> Result<u32> {
    let name = type_name::<C::Hasher>();
    if name.contains("Poseidon2Hash") {
        let inner = type_name::<C::InnerHasher>();
        if inner.contains("Poseidon2Hash") {
            Ok(OLA_HASH_POSEIDON2)
        } else if inner.contains("PoseidonHash") {
            Ok(OLA_HASH_POSEIDON2_POW_POSEIDON)
        } else {
            Err(anyhow::anyhow!("the hip backend has no proof-of-work hash for {inner}"))
        }
    } else if name.contains("PoseidonHash") {
        Ok(OLA_HASH_POSEIDON)
    } else if name.contains("Blake3") {
        Ok(OLA_HASH_BLAKE3)
    } else if name.contains("KeccakHash<25>") {
        // KeccakGoldilocksConfig (plonk/config.rs:145-151); another truncation is another wire format the backend does not write
        Ok(OLA_HASH_KECCAK)
    } else {
        Err(anyhow::anyhow!("the hip backend has no Merkle hasher for {name}"))
    }
}

/// The first three tuples a failing cross-table lookup is missing (`ola_check_lookup`), for the line that names the lookup.
fn describe_lookup(c: *mut OlaCtx, words: &[u64], tables: &[*const *const u64], log_n: &[u32], lookup: u32) -> String {
    let mut found = [OlaLookupMismatch::default(); 3];
    let (mut n, mut width, mut totals) = (0u32, 0u32, [0u64; 4]);
    let rc = unsafe {
        ola_check_lookup(c, words.as_ptr(), words.len(), tables.as_ptr(), log_n.as_ptr(), lookup, found.as_mut_ptr(), found.len() as u32, &mut n,
                         totals.as_mut_ptr(), &mut width)
    };
    if rc != OLA_OK || n == 0 {
        return String::new();
    }
    let tuples: Vec<String> = found.iter().take(n as usize).map(|m| {
        let looking = if m.looking_entry == u32::MAX { "-".to_string() } else { format!("entry {} table {} row {}", m.looking_entry, m.looking_table, m.looking_row) };
        let looked = if m.looked_row == u64::MAX { "-".to_string() } else { format!("row {}", m.looked_row) };
        format!("{:?}: looking {} (first: {}), looked {} (first: {})", &m.values[..(width as usize).min(OLA_LOOKUP_MAX_VALUES)], m.looking_count, looking,
                m.looked_count, looked)
    }).collect();
    format!(" -- {} tuples differ, {} rows unmatched: {}{}", totals[2], totals[3], tuples.join(", "), if n as usize > found.len() { ", ..." } else { "" })
}

/// The report of `ola_check_constraints` over all tables as one line per entry.
fn describe_failures(c: *mut OlaCtx, words: &[u64], tables: &[*const *const u64], log_n: &[u32], params: &[u64]) -> String {
    const KINDS: [&str; 4] = ["constraint", "constraint_transition", "constraint_first_row", "constraint_last_row"];
    let mut found = vec![OlaConstraintFailure::default(); 64];
    let mut n = 0u32;
    let mask = if tables.len() >= 32 { u32::MAX } else { (1u32 << tables.len()) - 1 };
    let rc = unsafe {
        ola_check_constraints(c, words.as_ptr(), words.len(), tables.as_ptr(), log_n.as_ptr(), params.as_ptr(), std::ptr::null(), mask,
                              found.as_mut_ptr(), found.len() as u32, &mut n)
    };
    if rc != OLA_OK {
        return format!("(the constraint check itself failed with code {rc})");
    }
    if n == 0 {
        return "the constraint check on the trace domain finds nothing wrong".to_string();
    }
    let mut lines: Vec<String> = found.iter().take(n as usize).map(|f| match f.section {
        OLA_CHECK_LOOKUP if f.kind == 0 => format!("table {}, cross-table lookup {} (challenge {}): {} looking rows, {} looked rows{}", f.table, f.index, f.kind,
                                                   f.first_row, f.rows_failing, describe_lookup(c, words, tables, log_n, f.index)),
        OLA_CHECK_AIR => format!("table {}, constraint #{} ({}), first at row {}, {} rows", f.table, f.index, KINDS[(f.kind & 3) as usize], f.first_row, f.rows_failing),
        OLA_CHECK_PERMUTATION => format!("table {}, permutation batch {}: the running product does not close", f.table, f.index),
        _ => format!("table {}, cross-table lookup {} (challenge {}): {} looking rows, {} looked rows", f.table, f.index, f.kind, f.first_row, f.rows_failing),
    }).collect();
    if n as usize > found.len() {
        lines.push(format!("... and {} more", n as usize - found.len()));
    }
    lines.join("; ")
}

/// From the executor's records to the proof: the twelve tables are generated in HBM by `ola_prove_from_records` and proven there, no
/// table crosses the link.  `rec.size` must be `size_of::<OlaExecRecords>()`; its pointers must outlive the call.
pub fn prove_from_records<F, C, const D: usize>(config: &StarkConfig, rec: &OlaExecRecords, public_values: PublicValues) -> Result<AllProof<F, C, D>>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F>,
{
    ensure!(D == 2, "the backend proves over the quadratic extension");
    ensure!(rec.size as usize == std::mem::size_of::<OlaExecRecords>(), "OlaExecRecords.size is not the size of the struct");
    let words = airset();
    let out = with_ctx(hasher_of::<F, C, D>()?, config, |c| {
        let mut out = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let rc = unsafe { ola_prove_from_records(c, words.as_ptr(), words.len(), rec as *const OlaExecRecords, out.as_mut_ptr(), out.len(), &mut len) };
        if rc == OLA_E_INVALID_ARG && len > out.len() {
            // the proof is larger than the buffer: it was kept, fetch it without proving again
            out.resize(len, 0);
            check(unsafe { ola_take_pending_proof(c, out.as_mut_ptr(), out.len(), &mut len) })?;
        } else {
            check(rc)?;
        }
        out.truncate(len);
        Ok(out)
    })?;
    let mut proof: AllProof<F, C, D> = Buffer::new(out).read_all_proof()?;
    proof.public_values = public_values; // not part of the wire format (serialization.rs:391)
    Ok(proof)
}

/// `verify_proof` (circuits/src/stark/verifier.rs:35) on the device: the `AllProof` goes over in the reference's own wire format
/// (`Buffer::write_all_proof`, serialization.rs:377-393), the per-table parameters are taken from its compress challenges as the
/// reference's verifier takes them, and a refusal comes back as the reference's error would: the first failing check, in words, with
/// its table, query and oracle or layer.  The Merkle paths and the FRI algebra run on the GPU (`ola_verify_all_proof`).
pub fn verify_proof_hip<F, C, const D: usize>(config: &StarkConfig, all_proof: &AllProof<F, C, D>) -> Result<()>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F>,
{
    ensure!(D == 2, "the backend verifies over the quadratic extension");
    let mut buffer = Buffer::new(Vec::new());
    buffer.write_all_proof(all_proof)?;
    let bytes = buffer.bytes();
    let words = airset();
    with_ctx(hasher_of::<F, C, D>()?, config, |c| {
        let mut report: OlaVerifyReport = unsafe { std::mem::zeroed() };
        check(unsafe { ola_verify_all_proof(c, words.as_ptr(), words.len(), std::ptr::null(), bytes.as_ptr(), bytes.len(), &mut report) })?;
        ensure!(report.accepted == 1, "{}", unsafe { CStr::from_ptr(report.message.as_ptr()) }.to_string_lossy());
        Ok(())
    })
}

pub fn prove_with_traces_hip<F, C, const D: usize>(
    ola_stark: &OlaStark<F, D>,
    config: &StarkConfig,
    trace_poly_values: &[Vec<PolynomialValues<F>>; NUM_TABLES],
    public_values: PublicValues,
    timing: &mut TimingTree,
) -> Result<AllProof<F, C, D>>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F>,
{
    ensure!(D == 2, "the backend proves over the quadratic extension");
    ensure!(std::mem::size_of::<F>() == 8, "the backend reads columns as u64 words (GoldilocksField is repr(transparent) u64)");
    // one pointer per column, no copy: values may be any representative, the library canonicalises on the device
    let cols: Vec<Vec<*const u64>> = trace_poly_values.iter().map(|t| t.iter().map(|c| c.values.as_ptr() as *const u64).collect()).collect();
    let tables: Vec<*const *const u64> = cols.iter().map(|t| t.as_ptr()).collect();
    for t in trace_poly_values.iter() {
        ensure!(!t.is_empty() && t.iter().all(|c| c.len() == t[0].len() && c.len().is_power_of_two()), "ragged trace table");
    }
    let log_n: Vec<u32> = trace_poly_values.iter().map(|t| t[0].len().trailing_zeros()).collect();
    // prover.rs:307-320: the two compress challenges come from trace generation, not from this transcript
    let bitwise = ola_stark.bitwise_stark.get_compress_challenge().unwrap().to_canonical_u64();
    let program = ola_stark.program_stark.get_compress_challenge().unwrap().to_canonical_u64();
    let params = [bitwise, program];
    let mut compress = [0u64; NUM_TABLES];
    compress[Table::Bitwise as usize] = bitwise;
    compress[Table::Program as usize] = program;

    let words = airset();
    let out = with_ctx(hasher_of::<F, C, D>()?, config, |c| {
        // the library reads cols[t][0 .. width of table t in the AIR set): a shorter table would be read past its pointer Vec
        for (t, table) in trace_poly_values.iter().enumerate() {
            let mut shape = [0u32; 6];
            check(unsafe { ola_table_shape(c, words.as_ptr(), words.len(), t as u32, shape.as_mut_ptr()) })?;
            ensure!(table.len() == shape[0] as usize, "table {t} has {} columns, its AIR has {}", table.len(), shape[0]);
        }
        // scope times cost two event records per scope; ask for them when somebody will read the tree (TimingTree logs at Debug)
        let want_scopes = log::log_enabled!(log::Level::Debug);
        check(unsafe { ola_gpu_scope_times(c, want_scopes as i32, std::ptr::null_mut(), 0, std::ptr::null_mut()) })?;
        let mut out = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let t0 = Instant::now();
        let rc = unsafe {
            ola_prove_with_traces_cols(c, words.as_ptr(), words.len(), tables.as_ptr(), log_n.as_ptr(), params.as_ptr(), compress.as_ptr(),
                                       out.as_mut_ptr(), out.len(), &mut len)
        };
        if rc == OLA_E_INVALID_ARG && len > out.len() {
            // the proof is larger than the buffer: it was kept, fetch it without proving again
            out.resize(len, 0);
            check(unsafe { ola_take_pending_proof(c, out.as_mut_ptr(), out.len(), &mut len) })?;
        } else if rc == OLA_E_QUOTIENT_DEGREE {
            // "vanishing polynomial is not divisible by Z_H" names neither table nor constraint: ask the device which
            // constraint fails at which row (the reference's check_constraints, prover.rs:711-819)
            let err = check(rc).unwrap_err();
            let why = describe_failures(c, words, &tables, &log_n, &params);
            return Err(anyhow::anyhow!("{err}: {why}"));
        } else {
            check(rc)?;
        }
        out.truncate(len);
        if want_scopes {
            replay_scopes(c, timing, t0)?;
        }
        Ok(out)
    })?;
    let mut proof: AllProof<F, C, D> = Buffer::new(out).read_all_proof()?;
    proof.public_values = public_values; // not part of the wire format (serialization.rs:391)
    Ok(proof)
}
