// FriReductionStrategy::reduction_arity_bits (plonky2/plonky2/src/fri/reduction_strategies.rs:27-164) in plain C++: the arity of
// every FRI layer of a table, for all three variants.  Host only (no HIP: compiles with g++ alone, tests/host_fri_plan_check.cpp);
// the prover (fri.hip), the verifier's host stage (verify_host.h) and ola_fri_reduction_arity_bits all call fri_plan_arity_bits,
// so the ConstantArityBits loop and the MinSize search exist once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ola_gpu.h"

namespace ola {

enum { FRI_PLAN_MAX_LAYERS = 32, FRI_PLAN_MAX_ARITY_BITS = 4 };   // the verifier keeps one coset of a layer in registers (vfy::MAX_ARITY_BITS)

// the strategy a context runs with (ola_gpu_set_fri_reduction).  ConstantArityBits takes its two numbers from the configuration
// (OlaGpuConfig::fri_arity_bits, fri_final_poly_bits), as it always did.
struct FriPlanSpec {
    uint32_t strategy = OLA_FRI_CONSTANT_ARITY_BITS;
    uint32_t n = 0;                             // Fixed: the number of layers; MinSize: 0 = None, 1 = Some(args[0])
    uint32_t args[FRI_PLAN_MAX_LAYERS] = {0};
    bool operator==(const FriPlanSpec& o) const {
        if (strategy != o.strategy || n != o.n) return false;
        for (uint32_t i = 0; i < n; i++) if (args[i] != o.args[i]) return false;
        return true;
    }
};

// what ola_gpu_set_fri_reduction and ola_fri_reduction_arity_bits accept; nullptr: fine, else what is wrong with it
inline const char* fri_plan_spec_check(uint32_t strategy, const uint32_t* args, uint32_t n) {
    if (n > 0 && !args) return "args is NULL";
    switch (strategy) {
        case OLA_FRI_CONSTANT_ARITY_BITS:
            if (n != 0) return "OLA_FRI_CONSTANT_ARITY_BITS takes no arguments (cfg.fri_arity_bits, cfg.fri_final_poly_bits)";
            return nullptr;
        case OLA_FRI_FIXED:
            if (n > FRI_PLAN_MAX_LAYERS) return "OLA_FRI_FIXED takes at most 32 layers";
            for (uint32_t i = 0; i < n; i++)
                if (args[i] < 1 || args[i] > FRI_PLAN_MAX_ARITY_BITS) return "OLA_FRI_FIXED: every layer's arity bits must be in 1..4";
            return nullptr;
        case OLA_FRI_MIN_SIZE:
            if (n > 1) return "OLA_FRI_MIN_SIZE takes no argument (None) or one (the maximum arity bits)";
            if (n == 1 && (args[0] < 1 || args[0] > FRI_PLAN_MAX_ARITY_BITS)) return "OLA_FRI_MIN_SIZE: the maximum arity bits must be in 1..4";
            return nullptr;
        default: return "unknown FRI reduction strategy";
    }
}
inline FriPlanSpec fri_plan_spec(uint32_t strategy, const uint32_t* args, uint32_t n) {
    FriPlanSpec s;
    s.strategy = strategy; s.n = n;
    for (uint32_t i = 0; i < n && i < FRI_PLAN_MAX_LAYERS; i++) s.args[i] = args[i];
    return s;
}

// reduction_strategies.rs:136-164 relative_proof_size: the FRI part of a proof in field elements, for a plan given as `len` arity bits
inline size_t fri_relative_proof_size(int degree_bits, int rate_bits, size_t num_queries, const int* arity_bits, size_t len) {
    const size_t D = 4;                                                      // :142
    int current_layer_bits = degree_bits + rate_bits;                        // :144
    size_t total_elems = 0;                                                  // :146
    for (size_t i = 0; i < len; i++) {                                       // :147
        const size_t arity = (size_t)1 << arity_bits[i];                     // :148
        total_elems += (arity - 1) * D * num_queries;                        // :151 neighbouring evaluations
        total_elems += (size_t)current_layer_bits * 4 * num_queries;         // :153 siblings in the Merkle path
        current_layer_bits -= arity_bits[i];                                 // :155
    }
    const size_t final_poly_len = (size_t)1 << (current_layer_bits - rate_bits);   // :159-160 (the search never goes below rate_bits)
    return total_elems + D * final_poly_len;                                 // :161-163
}

// reduction_strategies.rs:89-130 min_size_arity_bits_helper: depth first over non-increasing sequences, the first smallest one wins
// (`size < best_size`, :123).  prefix is the path of the search; best receives the best plan that begins with it.
inline size_t fri_min_size_helper(int degree_bits, int rate_bits, size_t num_queries, int global_max_arity_bits, std::vector<int>& prefix,
                                  std::vector<int>& best) {
    int sum_of_arities = 0;                                                  // :96
    for (int a : prefix) sum_of_arities += a;
    const int current_layer_bits = degree_bits + rate_bits - sum_of_arities; // :97
    best = prefix;                                                           // :100
    size_t best_size = fri_relative_proof_size(degree_bits, rate_bits, num_queries, prefix.data(), prefix.size());   // :101
    int max_arity_bits = prefix.empty() ? global_max_arity_bits : prefix.back();   // :106-109
    if (current_layer_bits - rate_bits < max_arity_bits) max_arity_bits = current_layer_bits - rate_bits;             // :110
    for (int next = 1; next <= max_arity_bits; next++) {                     // :112
        prefix.push_back(next);                                              // :113-114
        std::vector<int> cand;
        const size_t size = fri_min_size_helper(degree_bits, rate_bits, num_queries, max_arity_bits, prefix, cand);   // :116-122
        prefix.pop_back();
        if (size < best_size) { best.swap(cand); best_size = size; }        // :123-126
    }
    return best_size;                                                        // :129
}

// reduction_strategies.rs:30-57 reduction_arity_bits.  The spec has passed fri_plan_spec_check.
inline std::vector<int> fri_plan_arity_bits(const FriPlanSpec& s, int arity_bits, int final_poly_bits, int degree_bits, int rate_bits, int cap_height,
                                            size_t num_queries) {
    std::vector<int> result;
    if (s.strategy == OLA_FRI_FIXED) {                                       // :38
        for (uint32_t i = 0; i < s.n; i++) result.push_back((int)s.args[i]);
        return result;
    }
    if (s.strategy == OLA_FRI_MIN_SIZE) {                                    // :53-55, :60-86 min_size_arity_bits
        const int max_arity_bits = s.n ? (int)s.args[0] : 4;                 // :69 opt_max_arity_bits.unwrap_or(4)
        std::vector<int> prefix;
        fri_min_size_helper(degree_bits, rate_bits, num_queries, max_arity_bits, prefix, result);   // :72-73
        return result;
    }
    // :40-51 ConstantArityBits(arity_bits, final_poly_bits); `assert!(degree_bits >= arity_bits)` (:46) is left to the callers'
    // check of the total (fri_plan_fits), which refuses such a plan with the reference's words for the neighbouring failure
    while (degree_bits > final_poly_bits && degree_bits + rate_bits - arity_bits >= cap_height) {
        result.push_back(arity_bits);
        degree_bits -= arity_bits;
    }
    return result;
}

// a plan fits a table when the last layer's tree is at least as high as its cap ("FRI total reduction arity is too large.",
// plonk/circuit_builder.rs:922-925) and the final polynomial has a length (the reference's final_poly_len underflows beyond degree_bits)
inline bool fri_plan_fits(const std::vector<int>& arities, int degree_bits, int rate_bits, int cap_height) {
    int tot = 0;
    for (int a : arities) tot += a;
    return tot <= degree_bits + rate_bits - cap_height && tot <= degree_bits;
}

}  // namespace ola
