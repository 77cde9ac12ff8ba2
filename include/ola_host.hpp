// Host-side C++ mirror of the reference interfaces this backend replaces, over the C ABI of ola_gpu.h (header only, C++17,
// no HIP / torch types).  The reference is Rust; where its toolchain is missing this is the host layer a caller writes
// against -- same names, argument meaning and error behaviour as the Rust items cited at each declaration, so that code
// and tests read like the reference's own (tests/host_api_check.cpp).  INTEGRATION.md shows the Rust binding of the same
// entry points.
//
//   reference item                                                        here
//   plonky2/field/src/cfft/mod.rs:22,65,128,180  evaluate_poly ...        ola_host::fft::*
//   plonky2/plonky2/src/fri/oracle.rs:31-150     PolynomialBatch          ola_host::PolynomialBatch
//   plonky2/plonky2/src/iop/challenger.rs:19-170 Challenger               ola_host::Challenger
//   plonky2/plonky2/src/hash/poseidon.rs:593     PoseidonPermutation      ola_host::hash::permute / hash_no_pad / merkle_cap
//   plonky2/plonky2/src/fri/prover.rs:126        fri_proof_of_work        ola_host::fri_proof_of_work
//   circuits/src/stark/prover.rs:79              prove_with_traces        ola_host::prove_with_traces
//   circuits/src/stark/prover.rs:330             prove_single_table       ola_host::prove_single_table
//   circuits/src/stark/verifier.rs:35            verify_proof             ola_host::verify_proof
//   circuits/src/stark/verifier.rs:220 (FRI part) verify_stark_proof...   ola_host::verify_stark_proof_opening
//   circuits/src/stark/lookup.rs:68              permuted_cols            ola_host::permuted_cols
//   circuits/src/generation/poseidon.rs:5        generate_poseidon_trace  ola_host::generate_poseidon_trace
//   circuits/src/generation/cpu.rs:11            generate_cpu_trace       ola_host::generate_cpu_trace
//   circuits/src/generation/prog.rs:18           generate_prog_trace      ola_host::generate_prog_trace_steps
//   circuits/src/generation/memory.rs:5          generate_memory_trace    ola_host::generate_memory_trace
//   circuits/src/generation/builtin.rs:208       generate_cmp_trace       ola_host::generate_cmp_trace
//
// Errors: the Rust code returns anyhow::Result / panics on contract violations; here every failing call throws
// ola_host::Error carrying the C ABI's code (OLA_E_*) and message.  Field elements are plain uint64_t words
// (GoldilocksField is #[repr(transparent)] u64); any representative is accepted on input, outputs are canonical.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ola_gpu.h"

namespace ola_host {

using F = uint64_t;                       // GoldilocksField
using HashOut = std::array<F, 4>;         // hash/hash_types.rs:19-21
using MerkleCap = std::vector<HashOut>;   // hash/merkle_tree.rs:20
using PolynomialValues = std::vector<F>;  // field/src/polynomial/mod.rs:20
using PolynomialCoeffs = std::vector<F>;  // field/src/polynomial/mod.rs:128

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int32_t rc) {
    if (rc != OLA_OK) throw Error(rc, std::string("ola_gpu error ") + std::to_string(rc) + ": " + ola_gpu_last_error());
}

inline uint32_t log2_strict(size_t n) {   // util/src/lib.rs log2_strict: panics unless n is a power of two
    uint32_t k = 0;
    while (((size_t)1 << k) < n) k++;
    if (((size_t)1 << k) != n || n == 0) throw Error(OLA_E_INVALID_ARG, "length is not a power of two");
    return k;
}

// FriReductionStrategy (plonky2/plonky2/src/fri/reduction_strategies.rs:7-25).  The default, ConstantArityBits, takes its two numbers
// from StarkConfig::fri_arity_bits / fri_final_poly_bits.
struct FriReductionStrategy {
    uint32_t kind = OLA_FRI_CONSTANT_ARITY_BITS;
    std::vector<uint32_t> args;
    static FriReductionStrategy ConstantArityBits() { return FriReductionStrategy{}; }
    static FriReductionStrategy Fixed(std::vector<uint32_t> arity_bits) { FriReductionStrategy s; s.kind = OLA_FRI_FIXED; s.args = std::move(arity_bits); return s; }
    static FriReductionStrategy MinSize() { FriReductionStrategy s; s.kind = OLA_FRI_MIN_SIZE; return s; }                       // MinSize(None)
    static FriReductionStrategy MinSize(uint32_t max_arity_bits) { FriReductionStrategy s = MinSize(); s.args.push_back(max_arity_bits); return s; }
    // strategy.reduction_arity_bits(degree_bits, rate_bits, cap_height, num_queries) (ola_fri_reduction_arity_bits: host only)
    std::vector<uint32_t> reduction_arity_bits(const OlaGpuConfig* cfg, uint32_t degree_bits) const {
        uint32_t out[64], n = 0;
        check(ola_fri_reduction_arity_bits(cfg, kind, args.data(), (uint32_t)args.size(), degree_bits, out, 64, &n));
        return std::vector<uint32_t>(out, out + n);
    }
};

// FriConfig / StarkConfig::standard_fast_config (circuits/src/stark/config.rs:20-35) with the fields the backend reads.
struct StarkConfig {
    uint32_t rate_bits = 3, cap_height = 4, proof_of_work_bits = 16, fri_arity_bits = 4, fri_final_poly_bits = 5, num_query_rounds = 28,
             num_challenges = 2;
    // GenericConfig::Hasher (plonk/config.rs:112-161): OLA_HASH_POSEIDON = PoseidonGoldilocksConfig, OLA_HASH_BLAKE3 = Blake3GoldilocksConfig, OLA_HASH_KECCAK = KeccakGoldilocksConfig
    // OLA_HASH_POSEIDON2 = Poseidon2GoldilocksConfig, OLA_HASH_POSEIDON2_POW_POSEIDON = Poseidon2GoldilocksConfig2
    uint32_t hasher = OLA_HASH_POSEIDON;
    FriReductionStrategy reduction_strategy;      // single-device contexts take all three variants, multi-device ones the default
    static StarkConfig standard_fast_config() { return StarkConfig{}; }
};

// Which tables of the AIR set have a generated quotient kernel under `c` (ola_air_kernels_available_cfg: host only; the
// configuration's num_challenges decides -- a table without one runs the interpreter kernel, same bytes).
inline std::vector<bool> air_kernels_available(const std::vector<uint64_t>& airset, size_t ntables,
                                               const StarkConfig& c = StarkConfig::standard_fast_config()) {
    OlaGpuConfig g{};
    g.device = -1; g.stream = nullptr; g.rate_bits = c.rate_bits; g.cap_height = c.cap_height;
    g.proof_of_work_bits = c.proof_of_work_bits; g.fri_arity_bits = c.fri_arity_bits; g.fri_final_poly_bits = c.fri_final_poly_bits;
    g.num_query_rounds = c.num_query_rounds; g.num_challenges = c.num_challenges; g.hasher = c.hasher;
    std::vector<uint8_t> flags(ntables, 0);
    check(ola_air_kernels_available_cfg(&g, airset.data(), airset.size(), flags.data(), ntables));
    return std::vector<bool>(flags.begin(), flags.end());
}

// One device context (replaces the reference's process-wide init_gpu()/GPU_LOCK, cfft/ntt/mod.rs:21-50).
class Gpu {
public:
    explicit Gpu(int32_t device = -1, const StarkConfig& c = StarkConfig::standard_fast_config(), void* stream = nullptr) : config(c) {
        OlaGpuConfig g{};
        g.device = device; g.stream = stream; g.rate_bits = c.rate_bits; g.cap_height = c.cap_height;
        g.proof_of_work_bits = c.proof_of_work_bits; g.fri_arity_bits = c.fri_arity_bits; g.fri_final_poly_bits = c.fri_final_poly_bits;
        g.num_query_rounds = c.num_query_rounds; g.num_challenges = c.num_challenges; g.hasher = c.hasher;
        check(ola_gpu_init(&g, &ctx_));
        set_reduction_strategy(c.reduction_strategy);
    }
    // One context spanning several GPUs of the node (ola_gpu_init_multi): prove_with_traces then runs on all of them in one call.
    explicit Gpu(const std::vector<int32_t>& devices, const StarkConfig& c = StarkConfig::standard_fast_config()) : config(c) {
        OlaGpuConfig g{};
        g.device = -1; g.stream = nullptr; g.rate_bits = c.rate_bits; g.cap_height = c.cap_height;
        g.proof_of_work_bits = c.proof_of_work_bits; g.fri_arity_bits = c.fri_arity_bits; g.fri_final_poly_bits = c.fri_final_poly_bits;
        g.num_query_rounds = c.num_query_rounds; g.num_challenges = c.num_challenges; g.hasher = c.hasher;
        check(ola_gpu_init_multi(&g, devices.data(), (uint32_t)devices.size(), &ctx_));
        set_reduction_strategy(c.reduction_strategy);
    }
    uint32_t device_count() const { uint32_t n = 0; check(ola_gpu_device_count(ctx_, &n)); return n; }
    ~Gpu() { if (ctx_) ola_gpu_free(ctx_); }
    Gpu(const Gpu&) = delete;
    Gpu& operator=(const Gpu&) = delete;
    OlaCtx* ctx() const { return ctx_; }
    void sync() const { check(ola_gpu_sync(ctx_)); }
    void trim() const { check(ola_gpu_trim(ctx_)); }
    const StarkConfig config;

private:
    // (from the constructors: a refused strategy frees the context, whose destructor will not run)
    void set_reduction_strategy(const FriReductionStrategy& s) {
        if (s.kind == OLA_FRI_CONSTANT_ARITY_BITS && s.args.empty()) return;
        const int32_t rc = ola_gpu_set_fri_reduction(ctx_, s.kind, s.args.data(), (uint32_t)s.args.size());
        if (rc != OLA_OK) { const Error e(rc, ola_gpu_last_error()); ola_gpu_free(ctx_); ctx_ = nullptr; throw e; }
    }
    OlaCtx* ctx_ = nullptr;
};

// ---- cfft/mod.rs: transforms of one polynomial (natural order in, natural order out) --------------------------------------
namespace fft {
inline std::vector<F> run(const Gpu& g, int32_t op, const std::vector<F>& in, F shift, uint32_t blowup_log) {
    const uint32_t log_n = log2_strict(in.size());
    const bool grows = op == OLA_NTT_COSET_LDE || op == OLA_NTT_COSET_LDE_LEAF_ORDER;
    std::vector<F> out(grows ? in.size() << blowup_log : in.size());
    check(ola_ntt_batch(g.ctx(), op, in.data(), out.data(), log_n, 1, shift, blowup_log));
    return out;
}
inline PolynomialValues evaluate_poly(const Gpu& g, const PolynomialCoeffs& coeffs) { return run(g, OLA_NTT_EVALUATE, coeffs, 7, 0); }               // :22
inline PolynomialCoeffs interpolate_poly(const Gpu& g, const PolynomialValues& values) { return run(g, OLA_NTT_INTERPOLATE, values, 7, 0); }        // :128
// coset_fft with zero padding to n << rate_bits (polynomial/mod.rs:253-270 lde + coset_fft; shift = F::coset_shift() = 7)
inline PolynomialValues evaluate_poly_with_offset(const Gpu& g, const PolynomialCoeffs& coeffs, F shift = 7, uint32_t rate_bits = 0) {              // :65
    return run(g, OLA_NTT_COSET_LDE, coeffs, shift, rate_bits);
}
inline PolynomialCoeffs interpolate_poly_with_offset(const Gpu& g, const PolynomialValues& values, F shift = 7) {                                    // :180
    return run(g, OLA_NTT_COSET_INTERPOLATE, values, shift, 0);
}
}  // namespace fft

// ---- hash/poseidon.rs, hashing.rs, merkle_tree.rs -----------------------------------------------------------------------------
namespace hash {
inline std::array<F, 12> permute(const Gpu& g, std::array<F, 12> state) {            // PoseidonPermutation::permute, poseidon.rs:593-603
    check(ola_poseidon_permute(g.ctx(), state.data(), 1));
    return state;
}
inline HashOut hash_no_pad(const Gpu& g, const std::vector<F>& input) {              // hashing.rs:84-111
    HashOut h{};
    if (input.empty()) {            // absorbing nothing leaves the zero state; the squeeze returns its first four words
        return h;
    }
    check(ola_hash_rows(g.ctx(), input.data(), 1, input.size(), h.data()));
    return h;
}
inline HashOut two_to_one(const Gpu& g, const HashOut& l, const HashOut& r) {        // hashing.rs:67-82 compress
    std::array<F, 12> s{l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    s = permute(g, s);
    return HashOut{s[0], s[1], s[2], s[3]};
}
// MerkleTree::new(leaves, cap_height).cap (merkle_tree/mod.rs:180-233); leaves row-major, all of one length
inline MerkleCap merkle_cap(const Gpu& g, const std::vector<std::vector<F>>& leaves, uint32_t cap_height) {
    if (leaves.empty()) throw Error(OLA_E_INVALID_ARG, "no leaves");
    const size_t len = leaves[0].size();
    std::vector<F> flat;
    flat.reserve(leaves.size() * len);
    for (const auto& l : leaves) {
        if (l.size() != len) throw Error(OLA_E_INVALID_ARG, "ragged leaves");
        flat.insert(flat.end(), l.begin(), l.end());
    }
    MerkleCap cap((size_t)1 << cap_height);
    check(ola_merkle_cap(g.ctx(), flat.data(), leaves.size(), len, cap_height, cap[0].data()));
    return cap;
}
// verify_merkle_proof_to_cap (merkle_proofs.rs:51-76), hashing on the device like everything else here
inline bool verify_merkle_proof_to_cap(const Gpu& g, const std::vector<F>& leaf_data, size_t leaf_index, const MerkleCap& cap,
                                       const std::vector<HashOut>& siblings) {
    HashOut cur = hash_no_pad(g, leaf_data);
    size_t idx = leaf_index;
    for (const HashOut& s : siblings) {
        cur = (idx & 1) ? two_to_one(g, s, cur) : two_to_one(g, cur, s);
        idx >>= 1;
    }
    return idx < cap.size() && cap[idx] == cur;
}
}  // namespace hash

// ---- fri/oracle.rs:31-150 ---------------------------------------------------------------------------------------------------------
// A committed batch of polynomials: coefficients, their low-degree extension and its Merkle tree stay in HBM.
class PolynomialBatch {
public:
    // from_values (oracle.rs:45-64): one vector per polynomial, all of the same power-of-two length.  rate_bits / cap_height
    // are the context's (StarkConfig); blinding is always false in this prover.
    static PolynomialBatch from_values(const Gpu& g, const std::vector<PolynomialValues>& values) { return make(g, values, false); }
    static PolynomialBatch from_coeffs(const Gpu& g, const std::vector<PolynomialCoeffs>& coeffs) { return make(g, coeffs, true); }   // :66-100

    PolynomialBatch(PolynomialBatch&& o) noexcept : g_(o.g_), h_(o.h_), cap_(std::move(o.cap_)), ncols_(o.ncols_), degree_log(o.degree_log), rate_bits(o.rate_bits) { o.h_ = nullptr; }
    PolynomialBatch(const PolynomialBatch&) = delete;
    ~PolynomialBatch() { if (h_) ola_batch_free(g_->ctx(), h_); }

    const MerkleCap& merkle_cap() const { return cap_; }                 // merkle_tree.cap
    size_t num_polynomials() const { return ncols_; }
    const OlaBatch* handle() const { return h_; }
    std::vector<PolynomialCoeffs> polynomials() const {                  // the `polynomials` field
        const size_t n = (size_t)1 << degree_log;
        std::vector<F> flat(ncols_ * n);
        check(ola_batch_get_coeffs(g_->ctx(), h_, flat.data()));
        std::vector<PolynomialCoeffs> out(ncols_);
        for (size_t c = 0; c < ncols_; c++) out[c].assign(flat.begin() + c * n, flat.begin() + (c + 1) * n);
        return out;
    }
    // get_lde_values(index, step) (oracle.rs:131-137): row `index * step` of the LDE in natural order of the coset
    std::vector<F> get_lde_values(size_t index, size_t step) const {
        std::vector<F> row(ncols_);
        check(ola_batch_get_lde_row(g_->ctx(), h_, index, step, row.data()));
        return row;
    }
    // merkle_tree.get(leaf_index) and merkle_tree.prove(leaf_index) (merkle_tree/mod.rs:235-308)
    std::pair<std::vector<F>, std::vector<HashOut>> leaf_with_proof(size_t leaf_index) const {
        const size_t depth = degree_log + rate_bits - g_->config.cap_height;
        std::vector<F> row(ncols_);
        std::vector<HashOut> sib(depth);
        check(ola_batch_get_leaf(g_->ctx(), h_, leaf_index, row.data(), depth ? sib[0].data() : nullptr));
        return {row, sib};
    }

private:
    PolynomialBatch(const Gpu* g, OlaBatch* h, MerkleCap cap, size_t ncols, uint32_t dl, uint32_t rb)
        : g_(g), h_(h), cap_(std::move(cap)), ncols_(ncols), degree_log(dl), rate_bits(rb) {}
    static PolynomialBatch make(const Gpu& g, const std::vector<std::vector<F>>& cols, bool coeffs) {
        if (cols.empty()) throw Error(OLA_E_INVALID_ARG, "empty batch");
        const uint32_t log_n = log2_strict(cols[0].size());
        std::vector<const F*> ptrs;
        for (const auto& c : cols) {
            if (c.size() != cols[0].size()) throw Error(OLA_E_INVALID_ARG, "polynomials of different lengths");
            ptrs.push_back(c.data());
        }
        MerkleCap cap((size_t)1 << g.config.cap_height);
        OlaBatch* h = nullptr;
        check((coeffs ? ola_commit_coeffs : ola_commit_values)(g.ctx(), ptrs.data(), (uint32_t)cols.size(), log_n, &h, cap[0].data()));
        return PolynomialBatch(&g, h, std::move(cap), cols.size(), log_n, g.config.rate_bits);
    }
    const Gpu* g_;
    OlaBatch* h_;
    MerkleCap cap_;
    size_t ncols_;

public:
    const uint32_t degree_log, rate_bits;
};

// ---- iop/challenger.rs:19-170 (duplex sponge over the hasher's permutation; host arithmetic, no device needed) -----------
class Challenger {
public:
    Challenger() { check(ola_challenger_init(&ch_)); }                                                        // :37
    explicit Challenger(const Gpu& g) {                                                                       // Challenger::<F, C::Hasher>::new()
        check(g.config.hasher == OLA_HASH_KECCAK ? ola_challenger_init_keccak(&ch_) : ola_challenger_init_hasher(&ch_, g.config.hasher));
    }
    void observe_element(F e) { check(ola_challenger_observe(&ch_, &e, 1)); }                                  // :46
    void observe_elements(const std::vector<F>& es) { check(ola_challenger_observe(&ch_, es.data(), es.size())); }   // :64
    void observe_hash(const HashOut& h) { check(ola_challenger_observe_cap(&ch_, h.data(), 1)); }              // :79
    void observe_cap(const MerkleCap& cap) { for (const auto& h : cap) observe_hash(h); }                      // :83
    F get_challenge() { F c; check(ola_challenger_get(&ch_, &c, 1)); return c; }                               // :89
    std::vector<F> get_n_challenges(size_t n) { std::vector<F> v(n); for (auto& c : v) c = get_challenge(); return v; }   // :102
    HashOut get_hash() { HashOut h; for (auto& x : h) x = get_challenge(); return h; }                         // :106
    std::array<F, 2> get_extension_challenge() { F a = get_challenge(); F b = get_challenge(); return {a, b}; }   // :117
    std::array<F, 12> compact() { check(ola_challenger_compact(&ch_)); std::array<F, 12> s; for (int i = 0; i < 12; i++) s[i] = ch_.sponge_state[i]; return s; }   // :155
    OlaChallenger& raw() { return ch_; }

private:
    OlaChallenger ch_;
};

// ---- fri/prover.rs:126-156: smallest nonce whose hash with the transcript digest has `bits` leading zeros -------------------
inline F fri_proof_of_work(const Gpu& g, const HashOut& current_hash, uint32_t bits) {
    F w = 0;
    check(ola_pow(g.ctx(), current_hash.data(), bits, &w));
    return w;
}

// ---- circuits/src/stark/prover.rs:499-553 + fri/oracle.rs:167-241 + fri/prover.rs:20-204: the opening proof of one table ----------
// One call with the transcript inside the library (the fast path): returns {opening-set bytes, FriProof bytes}, `challenger` advances as
// the reference's does.
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> open_and_prove(const Gpu& g, const PolynomialBatch& trace, const PolynomialBatch& zs,
                                                                            const PolynomialBatch& quotient, uint32_t num_permutation_zs,
                                                                            Challenger& challenger) {
    std::vector<uint8_t> out((size_t)1 << 20);
    size_t len = 0, olen = 0;
    auto call = [&]() {
        return ola_open_and_prove(g.ctx(), trace.handle(), zs.handle(), quotient.handle(), num_permutation_zs, &challenger.raw(), out.data(), out.size(), &len, &olen);
    };
    int32_t rc = call();
    if (rc == OLA_E_INVALID_ARG && len > out.size()) { out.resize(len); rc = call(); }
    check(rc);
    return {std::vector<uint8_t>(out.begin(), out.begin() + (long)olen), std::vector<uint8_t>(out.begin() + (long)olen, out.begin() + (long)len)};
}
// The same one step per call, for a caller that keeps the reference's loops and its own Challenger (ABI revision 7).
class FriSteps {
public:
    // StarkOpeningSet::new (proof.rs:198-233): the opening set in wire format (Buffer::read_opening_set reads it)
    FriSteps(const Gpu& g, const PolynomialBatch& trace, const PolynomialBatch& zs, const PolynomialBatch& quotient, uint32_t num_permutation_zs,
             const std::array<F, 2>& zeta)
        : g_(&g) {
        openings.resize((size_t)1 << 16);
        size_t len = 0;
        auto call = [&]() { return ola_open(g.ctx(), trace.handle(), zs.handle(), quotient.handle(), num_permutation_zs, zeta.data(), openings.data(), openings.size(), &len, &h_); };
        int32_t rc = call();
        if (rc == OLA_E_INVALID_ARG && len > openings.size()) { openings.resize(len); rc = call(); }
        check(rc);
        openings.resize(len);
        uint32_t n = 0, fl = 0;
        check(ola_fri_plan(h_, nullptr, 0, &n, &fl));
        reduction_arity_bits.resize(n);
        check(ola_fri_plan(h_, reduction_arity_bits.data(), n, &n, &fl));
        final_poly_len = fl;
    }
    FriSteps(const FriSteps&) = delete;
    ~FriSteps() { if (h_) ola_fri_free(h_); }
    void begin(const std::array<F, 2>& alpha) { check(ola_fri_commit_begin(h_, alpha.data())); }                       // fri/oracle.rs:178-219
    MerkleCap next_layer(const std::array<F, 2>* beta) {                                                               // fri/prover.rs:72-121, one turn
        MerkleCap cap((size_t)1 << g_->config.cap_height);
        check(ola_fri_commit_next_layer(h_, beta ? beta->data() : nullptr, cap[0].data()));
        return cap;
    }
    std::vector<std::array<F, 2>> finish(const std::array<F, 2>* beta) {                                               // prover.rs:114-119
        std::vector<std::array<F, 2>> poly(final_poly_len ? final_poly_len : 1);
        size_t n = 0;
        check(ola_fri_commit_finish(h_, beta ? beta->data() : nullptr, poly[0].data(), poly.size(), &n));
        poly.resize(n);
        return poly;
    }
    std::vector<uint8_t> query_rounds(const std::vector<F>& x_index) {                                                 // prover.rs:150-204, wire format
        std::vector<uint8_t> out((size_t)1 << 20);
        size_t len = 0;
        auto call = [&]() { return ola_fri_query(h_, x_index.data(), (uint32_t)x_index.size(), out.data(), out.size(), &len); };
        int32_t rc = call();
        if (rc == OLA_E_INVALID_ARG && len > out.size()) { out.resize(len); rc = call(); }
        check(rc);
        out.resize(len);
        return out;
    }
    std::vector<uint8_t> openings;                  // write_opening_set's bytes (serialization.rs:164-175)
    std::vector<uint32_t> reduction_arity_bits;     // fri_params.reduction_arity_bits
    size_t final_poly_len = 0;

private:
    const Gpu* g_;
    OlaFri* h_ = nullptr;
};

// ---- circuits/src/stark/prover.rs:79-327 --------------------------------------------------------------------------------------------
// `airset`: the tables and cross-table lookups as data (olavm_amd/air/dsl.py blob); traces[t]: table t column-major,
// width_t columns of 2^log_n[t] words; params: per-table public parameters in blob order; compress_challenges: one per
// table (0 where unused).  Returns the AllProof wire bytes (serialization.rs:377-393).
inline std::vector<uint8_t> prove_with_traces(const Gpu& g, const std::vector<F>& airset, const std::vector<std::vector<F>>& traces,
                                              const std::vector<uint32_t>& log_n, const std::vector<F>& params,
                                              const std::vector<F>& compress_challenges) {
    if (traces.size() != log_n.size()) throw Error(OLA_E_INVALID_ARG, "one height per trace");
    std::vector<const F*> ptrs;
    for (const auto& t : traces) ptrs.push_back(t.data());
    std::vector<uint8_t> out((size_t)8 << 20);
    size_t len = 0;
    int32_t rc = ola_prove_with_traces(g.ctx(), airset.data(), airset.size(), ptrs.data(), log_n.data(), params.empty() ? nullptr : params.data(),
                                       compress_challenges.empty() ? nullptr : compress_challenges.data(), out.data(), out.size(), &len);
    if (rc == OLA_E_INVALID_ARG && len > out.size()) {      // buffer too small: the finished proof waits in the context
        out.resize(len);
        rc = ola_take_pending_proof(g.ctx(), out.data(), out.size(), &len);
    }
    check(rc);
    out.resize(len);
    return out;
}

// ---- circuits/src/stark/verifier.rs:35-206 ------------------------------------------------------------------------------------------
// verify_proof(ola_stark, all_proof, config): the reference returns Ok(()) or the first failing `ensure!` as an anyhow::Error.  Here the
// report is returned: `accepted`, and for a refusal the OLA_VERIFY_* reason, the table, query and oracle-or-layer where the reference
// stops, and its words.  params empty: the per-table parameters are the proof's compress challenges, as in the reference.  A rejected
// proof is a report, not an exception; only a call that could not run throws.
inline OlaVerifyReport verify_proof(const Gpu& g, const std::vector<F>& airset, const std::vector<uint8_t>& all_proof, const std::vector<F>& params = {}) {
    OlaVerifyReport rep{};
    check(ola_verify_all_proof(g.ctx(), airset.data(), airset.size(), params.empty() ? nullptr : params.data(), all_proof.data(), all_proof.size(), &rep));
    return rep;
}
// The verifier's side of open_and_prove: the FRI half of verify_stark_proof_with_challenges (verifier.rs:298-323, plonky2's verify_fri_proof)
// for one table's opening set and FRI proof, continuing the caller's transcript; `challenger` advances as the prover's did when the proof
// is accepted.  caps: the trace, Zs and quotient commitments' caps; num_polys: their widths.
inline OlaVerifyReport verify_stark_proof_opening(const Gpu& g, const std::array<MerkleCap, 3>& caps, const std::array<uint32_t, 3>& num_polys,
                                                  uint32_t degree_bits, uint32_t num_permutation_zs, const std::vector<uint8_t>& openings,
                                                  const std::vector<uint8_t>& fri_proof, Challenger& challenger) {
    std::vector<F> cap_words;
    for (const MerkleCap& cap : caps) {
        if (cap.size() != (size_t)1 << g.config.cap_height) throw Error(OLA_E_INVALID_ARG, "a cap of 2^cap_height digests per commitment");
        for (const HashOut& h : cap) cap_words.insert(cap_words.end(), h.begin(), h.end());
    }
    std::vector<uint8_t> bytes(openings);
    bytes.insert(bytes.end(), fri_proof.begin(), fri_proof.end());
    OlaVerifyReport rep{};
    check(ola_verify_opening(g.ctx(), cap_words.data(), num_polys.data(), degree_bits, num_permutation_zs, bytes.data(), bytes.size(), &challenger.raw(), &rep));
    return rep;
}

// From the executor's records (OlaExecRecords: set `size` to sizeof, pointers host or device memory) to the AllProof wire bytes: the
// twelve tables are generated resident and proven, no table crosses the link (ola_prove_from_records).
inline std::vector<uint8_t> prove_from_records(const Gpu& g, const std::vector<F>& airset, const OlaExecRecords& rec) {
    std::vector<uint8_t> out((size_t)8 << 20);
    size_t len = 0;
    int32_t rc = ola_prove_from_records(g.ctx(), airset.data(), airset.size(), &rec, out.data(), out.size(), &len);
    if (rc == OLA_E_INVALID_ARG && len > out.size()) {      // buffer too small: the finished proof waits in the context
        out.resize(len);
        rc = ola_take_pending_proof(g.ctx(), out.data(), out.size(), &len);
    }
    check(rc);
    out.resize(len);
    return out;
}

// ---- circuits/src/stark/prover.rs:711-819, cross_table_lookup.rs:551-584, test_utils.rs:152-195 ------------------------------------
// Why a trace does not prove: the constraint programs, permutation arguments and cross-table lookups of the tables in `table_mask`
// on the trace domain (ola_check_constraints).  traces / log_n / params as for prove_with_traces (a table outside the mask may be
// empty); ctl_challenges: num_challenges x {beta, gamma}, or empty for the library's deterministic ones.  Returns the failures
// sorted by (table, section, index); empty for a trace that satisfies everything.
inline std::vector<OlaConstraintFailure> check_constraints(const Gpu& g, const std::vector<F>& airset, const std::vector<std::vector<F>>& traces,
                                                           const std::vector<uint32_t>& log_n, const std::vector<F>& params = {},
                                                           uint32_t table_mask = 0xFFFFFFFFu, const std::vector<std::array<F, 2>>& ctl_challenges = {}) {
    if (traces.size() != log_n.size() || traces.size() > 32) throw Error(OLA_E_INVALID_ARG, "one height per trace, at most 32 tables");
    if (traces.size() < 32) table_mask &= ((uint32_t)1 << traces.size()) - 1;
    std::vector<std::vector<const F*>> cols(traces.size());
    std::vector<const F* const*> tabs;
    for (size_t t = 0; t < traces.size(); t++) {
        const size_t n = (size_t)1 << log_n[t];
        if (traces[t].size() % n) throw Error(OLA_E_INVALID_ARG, "a table is not a whole number of columns");
        for (size_t c = 0; c * n < traces[t].size(); c++) cols[t].push_back(traces[t].data() + c * n);
        tabs.push_back(cols[t].empty() ? nullptr : cols[t].data());
    }
    std::vector<F> ctl;
    for (const auto& c : ctl_challenges) { ctl.push_back(c[0]); ctl.push_back(c[1]); }
    std::vector<OlaConstraintFailure> out(64);
    uint32_t n = 0;
    auto call = [&]() {
        return ola_check_constraints(g.ctx(), airset.data(), airset.size(), tabs.data(), log_n.data(), params.empty() ? nullptr : params.data(),
                                     ctl.empty() ? nullptr : ctl.data(), table_mask, out.data(), (uint32_t)out.size(), &n);
    };
    check(call());
    if (n > out.size()) { out.resize(n); check(call()); }
    out.resize(n);
    return out;
}

// ---- circuits/src/generation/ctl_test/*.rs, cross_table_lookup.rs:551-584 ---------------------------------------------------------
// Which tuples cross-table lookup `lookup` (the `index` of an OLA_CHECK_LOOKUP failure) is missing: the exact multiset difference of its
// two sides (ola_check_lookup).  traces / log_n as for check_constraints; tables the lookup does not name may be empty.  max_tuples:
// report at most that many (0: all).
struct LookupReport {
    uint32_t lookup = 0, width = 0;
    uint64_t totals[4] = {0, 0, 0, 0};          // selected looking rows, selected looked rows, mismatching tuples, unmatched rows
    std::vector<OlaLookupMismatch> mismatches;  // sorted by values[0 .. width)
    // one line per tuple, the text of olavm_amd.backend.format_lookup_report
    std::string text() const {
        auto num = [](uint64_t v) { return std::to_string((unsigned long long)v); };
        std::string s = "lookup " + num(lookup) + ": width " + num(width) + ", " + num(totals[0]) + " looking rows, " + num(totals[1]) +
                        " looked rows, " + num(totals[2]) + " mismatching tuples, " + num(totals[3]) + " rows unmatched";
        for (const OlaLookupMismatch& m : mismatches) {
            s += "\n  (";
            for (uint32_t k = 0; k < width && k < OLA_LOOKUP_MAX_VALUES; k++) s += (k ? ", " : "") + num(m.values[k]);
            s += "): looking " + num(m.looking_count) + " (first: ";
            s += m.looking_entry == UINT32_MAX ? std::string("-")
                                               : "entry " + num(m.looking_entry) + " table " + num(m.looking_table) + " row " + num(m.looking_row);
            s += "), looked " + num(m.looked_count) + " (first: ";
            s += m.looked_row == UINT64_MAX ? std::string("-") : "row " + num(m.looked_row);
            s += ")";
        }
        if (mismatches.size() < totals[2]) s += "\n  ... " + num(totals[2] - mismatches.size()) + " more";
        return s;
    }
};
inline LookupReport check_lookup(const Gpu& g, const std::vector<F>& airset, const std::vector<std::vector<F>>& traces,
                                 const std::vector<uint32_t>& log_n, uint32_t lookup, uint32_t max_tuples = 0) {
    if (traces.size() != log_n.size()) throw Error(OLA_E_INVALID_ARG, "one height per trace");
    std::vector<std::vector<const F*>> cols(traces.size());
    std::vector<const F* const*> tabs;
    for (size_t t = 0; t < traces.size(); t++) {
        if (log_n[t] > 30) throw Error(OLA_E_INVALID_ARG, "table size out of range");
        const size_t n = (size_t)1 << log_n[t];
        if (traces[t].size() % n) throw Error(OLA_E_INVALID_ARG, "a table is not a whole number of columns");
        for (size_t c = 0; c * n < traces[t].size(); c++) cols[t].push_back(traces[t].data() + c * n);
        tabs.push_back(cols[t].empty() ? nullptr : cols[t].data());
    }
    LookupReport rep;
    rep.lookup = lookup;
    rep.mismatches.resize(max_tuples ? max_tuples : 64);
    uint32_t n = 0;
    auto call = [&]() {
        return ola_check_lookup(g.ctx(), airset.data(), airset.size(), tabs.data(), log_n.data(), lookup, rep.mismatches.data(),
                                (uint32_t)rep.mismatches.size(), &n, rep.totals, &rep.width);
    };
    check(call());
    if (!max_tuples && n > rep.mismatches.size()) { rep.mismatches.resize(n); check(call()); }
    rep.mismatches.resize(std::min<size_t>(n, rep.mismatches.size()));
    return rep;
}

// prove_single_table (prover.rs:330-513) for callers that keep the reference's orchestration: `trace` = the table's columns,
// `commitment` = PolynomialBatch::from_values of them, ctl_challenges = num_challenges x {beta, gamma}; the shared challenger
// advances as in the reference.  Returns the table's StarkProof bytes (serialization.rs:349-358).
inline std::vector<uint8_t> prove_single_table(const Gpu& g, const std::vector<F>& airset, uint32_t table, const std::vector<PolynomialValues>& trace,
                                               const PolynomialBatch& commitment, const std::vector<std::array<F, 2>>& ctl_challenges,
                                               const std::vector<F>& params, Challenger& challenger) {
    std::vector<const F*> cols;
    for (const auto& c : trace) cols.push_back(c.data());
    std::vector<F> cap, ctl;
    for (const auto& h : commitment.merkle_cap()) cap.insert(cap.end(), h.begin(), h.end());
    for (const auto& c : ctl_challenges) { ctl.push_back(c[0]); ctl.push_back(c[1]); }
    std::vector<uint8_t> out((size_t)4 << 20);
    size_t len = 0;
    auto call = [&]() {
        return ola_prove_single_table(g.ctx(), airset.data(), airset.size(), table, cols.data(), commitment.handle(), cap.data(), ctl.data(),
                                      params.empty() ? nullptr : params.data(), &challenger.raw(), out.data(), out.size(), &len);
    };
    int32_t rc = call();
    if (rc == OLA_E_INVALID_ARG && len > out.size()) { out.resize(len); rc = call(); }
    check(rc);
    out.resize(len);
    return out;
}

// ---- trace-generation helpers -----------------------------------------------------------------------------------------------------
inline std::pair<std::vector<F>, std::vector<F>> permuted_cols(const Gpu& g, const std::vector<F>& inputs, const std::vector<F>& table) {   // lookup.rs:68
    if (inputs.size() != table.size()) throw Error(OLA_E_INVALID_ARG, "inputs and table differ in length");
    std::vector<F> pi(inputs.size()), pt(inputs.size());
    check(ola_permuted_cols(g.ctx(), inputs.data(), table.data(), inputs.size(), pi.data(), pt.data()));
    return {pi, pt};
}
// inputs: 12 x n column-major -> the 134 x n Poseidon table (generation/poseidon.rs:5-80)
inline std::vector<F> generate_poseidon_trace(const Gpu& g, const std::vector<F>& inputs, size_t n, const std::vector<F>& filters = {}) {
    if (inputs.size() != 12 * n || (!filters.empty() && filters.size() != 4 * n)) throw Error(OLA_E_INVALID_ARG, "shape");
    std::vector<F> out(134 * n);
    check(ola_generate_poseidon_trace(g.ctx(), inputs.data(), filters.empty() ? nullptr : filters.data(), n, out.data()));
    return out;
}
// step records (OLA_CPU_STEP_WORDS x n_steps column-major) -> the 94 x 2^log_n CPU table (generation/cpu.rs:11-218)
inline std::vector<F> generate_cpu_trace(const Gpu& g, const std::vector<F>& steps, size_t n_steps, uint32_t log_n) {
    if (steps.size() != OLA_CPU_STEP_WORDS * n_steps || log_n > 26) throw Error(OLA_E_INVALID_ARG, "shape");
    std::vector<F> out((size_t)94 << log_n);
    check(ola_generate_cpu_trace(g.ctx(), n_steps ? steps.data() : nullptr, n_steps, log_n, out.data()));
    return out;
}
// step records and the listing side (7 x 2^log_n) -> the 18 x 2^log_n program table (generation/prog.rs:18-156); *exec_rows
// receives the number of executed rows also when they do not fit (the call then throws OLA_E_INVALID_ARG)
inline std::vector<F> generate_prog_trace_steps(const Gpu& g, const std::vector<F>& steps, size_t n_steps, const std::vector<F>& prog,
                                                uint32_t log_n, F beta, uint64_t* exec_rows = nullptr, uint32_t flags = 0) {
    if (steps.size() != OLA_CPU_STEP_WORDS * n_steps || log_n > 26 || prog.size() != (size_t)7 << log_n) throw Error(OLA_E_INVALID_ARG, "shape");
    std::vector<F> out((size_t)18 << log_n);
    uint64_t rows = 0;
    const int32_t rc = ola_generate_prog_trace_steps(g.ctx(), n_steps ? steps.data() : nullptr, n_steps, prog.data(), log_n, beta, flags,
                                                     out.data(), &rows);
    if (exec_rows) *exec_rows = rows;
    check(rc);
    return out;
}
// raw memory cells (OLA_MEM_CELL_WORDS x n_cells column-major, any order) -> the 29 x n memory table (generation/memory.rs:5-153), sorted on
// the device; rc_values, when given, receives the range-checked sort values followed by the region values, rc_counts how many of each
inline std::vector<F> generate_memory_trace(const Gpu& g, const std::vector<F>& cells, size_t n_cells, std::vector<F>* rc_values = nullptr,
                                            uint64_t rc_counts[2] = nullptr, uint32_t flags = 0) {
    if (cells.size() != OLA_MEM_CELL_WORDS * n_cells) throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    uint64_t counts[2] = {0, 0};
    check(ola_generate_memory_trace(nullptr, nullptr, n_cells, flags, nullptr, &log_n, nullptr, counts));
    std::vector<F> out((size_t)29 << log_n), rc(2 * n_cells);
    check(ola_generate_memory_trace(g.ctx(), n_cells ? cells.data() : nullptr, n_cells, flags, out.data(), &log_n, n_cells ? rc.data() : nullptr,
                                    counts));
    rc.resize(counts[0] + counts[1]);
    if (rc_values) *rc_values = std::move(rc);
    if (rc_counts) { rc_counts[0] = counts[0]; rc_counts[1] = counts[1]; }
    return out;
}
// operand pairs (2 x n_ops column-major) -> the 6 x n comparison table (generation/builtin.rs:208-247); abs_diffs, when given, receives
// ABS_DIFF of the live rows
inline std::vector<F> generate_cmp_trace(const Gpu& g, const std::vector<F>& ops, size_t n_ops, std::vector<F>* abs_diffs = nullptr) {
    if (ops.size() != 2 * n_ops) throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    check(ola_generate_cmp_trace(nullptr, nullptr, n_ops, nullptr, &log_n, nullptr));
    std::vector<F> out((size_t)6 << log_n), diffs(n_ops);
    check(ola_generate_cmp_trace(g.ctx(), n_ops ? ops.data() : nullptr, n_ops, out.data(), &log_n, n_ops ? diffs.data() : nullptr));
    if (abs_diffs) *abs_diffs = std::move(diffs);
    return out;
}

// access records (OLA_STORAGE_ACCESS_WORDS x n_access column-major, execution order) -> the 48 x n storage-access table
// (generation/storage.rs:7-123), the state tree hashed on the device.  siblings: empty = the self-contained batch on an empty tree, else
// 1024 x n_access from the caller's tree.  psdn_inputs / psdn_filters, when given, are the 12 x psdn_stride and 4 x psdn_stride input
// buffers of generate_poseidon_table whose storage rows the call fills; roots, when given, receives the root before the first access
// with rows and the root after the last access
inline std::vector<F> generate_storage_trace(const Gpu& g, const std::vector<F>& accesses, size_t n_access, const std::vector<F>& siblings = {},
                                             std::vector<F>* psdn_inputs = nullptr, std::vector<F>* psdn_filters = nullptr, size_t psdn_stride = 0,
                                             uint64_t roots[8] = nullptr) {
    if (accesses.size() != OLA_STORAGE_ACCESS_WORDS * n_access || (!siblings.empty() && siblings.size() != 1024 * n_access) ||
        !psdn_inputs != !psdn_filters || (psdn_inputs && (psdn_inputs->size() != 12 * psdn_stride || psdn_filters->size() != 4 * psdn_stride)))
        throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    check(ola_generate_storage_trace(nullptr, n_access ? accesses.data() : nullptr, n_access, nullptr, nullptr, &log_n, nullptr, nullptr, 0, nullptr));
    std::vector<F> out((size_t)48 << log_n);
    check(ola_generate_storage_trace(g.ctx(), n_access ? accesses.data() : nullptr, n_access, siblings.empty() ? nullptr : siblings.data(), out.data(),
                                     &log_n, psdn_inputs ? psdn_inputs->data() : nullptr, psdn_filters ? psdn_filters->data() : nullptr, psdn_stride, roots));
    return out;
}
// permutation inputs (12 x stride column-major, the first n_rows of every column live) -> the 134 x n Poseidon table at its padded
// height n = next_pow2(max(n_rows, 8)) (generation/poseidon.rs:5-80)
inline std::vector<F> generate_poseidon_table(const Gpu& g, const std::vector<F>& inputs, size_t n_rows, size_t stride, const std::vector<F>& filters = {},
                                              uint32_t* log_n_out = nullptr) {
    if (inputs.size() != 12 * stride || (!filters.empty() && filters.size() != 4 * stride)) throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    check(ola_generate_poseidon_table(nullptr, nullptr, nullptr, n_rows, stride, nullptr, &log_n));
    std::vector<F> out((size_t)134 << log_n);
    check(ola_generate_poseidon_table(g.ctx(), stride ? inputs.data() : nullptr, filters.empty() ? nullptr : filters.data(), n_rows, stride, out.data(), &log_n));
    if (log_n_out) *log_n_out = log_n;
    return out;
}

// tape cells (OLA_TAPE_CELL_WORDS x n_cells column-major, execution order) -> the 6 x n tape table, sorted by address on the device
inline std::vector<F> generate_tape_trace(const Gpu& g, const std::vector<F>& cells, size_t n_cells, uint32_t* log_n_out = nullptr) {
    if (cells.size() != OLA_TAPE_CELL_WORDS * n_cells) throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    check(ola_generate_tape_trace(nullptr, nullptr, n_cells, nullptr, &log_n));
    std::vector<F> out((size_t)6 << log_n);
    check(ola_generate_tape_trace(g.ctx(), n_cells ? cells.data() : nullptr, n_cells, out.data(), &log_n));
    if (log_n_out) *log_n_out = log_n;
    return out;
}
// POSEIDON call records (OLA_POSEIDON_CALL_WORDS x n_calls column-major: clk, src, len, dst, psdn_row) and the Poseidon table
// (134 x 2^psdn_log_n; host or device memory) -> the 53 x n Poseidon-chunk table
inline std::vector<F> generate_poseidon_chunk_trace(const Gpu& g, const std::vector<F>& calls, size_t n_calls, const F* poseidon_table,
                                                    uint32_t psdn_log_n, uint32_t* log_n_out = nullptr) {
    if (calls.size() != OLA_POSEIDON_CALL_WORDS * n_calls) throw Error(OLA_E_INVALID_ARG, "shape");
    uint32_t log_n = 0;
    check(ola_generate_poseidon_chunk_trace(nullptr, n_calls ? calls.data() : nullptr, n_calls, nullptr, psdn_log_n, nullptr, &log_n));
    std::vector<F> out((size_t)53 << log_n);
    check(ola_generate_poseidon_chunk_trace(g.ctx(), n_calls ? calls.data() : nullptr, n_calls, poseidon_table, psdn_log_n, out.data(), &log_n));
    if (log_n_out) *log_n_out = log_n;
    return out;
}
// the zero-padded listing, the code address and the Poseidon table whose row i hashed words 8 i .. 8 i + 7 -> the 40 x n program-chunk table
inline std::vector<F> generate_prog_chunk_trace(const Gpu& g, const std::vector<F>& words, const uint64_t code_addr[4], bool result_line,
                                                const F* poseidon_table, uint32_t psdn_log_n, uint32_t* log_n_out = nullptr) {
    const uint32_t flags = result_line ? OLA_PROG_CHUNK_RESULT_LINE : 0u;
    uint32_t log_n = 0;
    check(ola_generate_prog_chunk_trace(nullptr, nullptr, words.size(), nullptr, flags, nullptr, psdn_log_n, nullptr, &log_n));
    std::vector<F> out((size_t)40 << log_n);
    check(ola_generate_prog_chunk_trace(g.ctx(), words.empty() ? nullptr : words.data(), words.size(), code_addr, flags, poseidon_table, psdn_log_n, out.data(), &log_n));
    if (log_n_out) *log_n_out = log_n;
    return out;
}

}  // namespace ola_host
