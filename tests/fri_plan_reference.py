"""FRI reduction plans for the tests: FriReductionStrategy::reduction_arity_bits (plonky2 fri/reduction_strategies.rs) restated on
Python integers -- written for the tests, not shared with the library or with tools/rust_air_eval.py, which interprets the
reference's source -- and the commit phase of tests/opening_reference.py under a plan with its own arity per layer.

A strategy is what olavm_amd.backend takes: ("constant_arity_bits",), ("fixed", [4, 3, 3]), ("min_size", None | k)."""
import numpy as np

from tests import opening_reference as R

P = R.P
DEFAULTS = {"rate_bits": 3, "cap_height": 4, "num_query_rounds": 28, "fri_arity_bits": 4, "fri_final_poly_bits": 5}


def relative_proof_size(degree_bits, rate_bits, num_queries, arity_bits):
    """the FRI part of a proof in field elements: per layer the other values of the coset and a Merkle path per query, then the final
    polynomial (four elements per coefficient, as the reference counts)"""
    bits, total = degree_bits + rate_bits, 0
    for ab in arity_bits:
        total += ((1 << ab) - 1) * 4 * num_queries + bits * 4 * num_queries
        bits -= ab
    assert bits >= rate_bits
    return total + 4 * (1 << (bits - rate_bits))


def min_size(degree_bits, rate_bits, num_queries, max_arity_bits=None):
    """the smallest plan among the non-increasing sequences of arity bits <= max_arity_bits (4 when None) whose sum is at most
    degree_bits; of equal sizes the one the reference's depth-first search meets first"""
    limit = 4 if max_arity_bits is None else max_arity_bits

    def search(prefix, cap):
        best, best_size = list(prefix), relative_proof_size(degree_bits, rate_bits, num_queries, prefix)
        top = min(prefix[-1] if prefix else cap, degree_bits - sum(prefix))
        for nxt in range(1, top + 1):
            cand, size = search(prefix + [nxt], top)
            if size < best_size:
                best, best_size = cand, size
        return best, best_size
    return search([], limit)[0]


def constant_arity_bits(degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits):
    out = []
    while degree_bits > final_poly_bits and degree_bits + rate_bits - arity_bits >= cap_height:
        out.append(arity_bits)
        degree_bits -= arity_bits
    return out


def arity_bits(strategy, degree_bits, **cfg):
    c = dict(DEFAULTS, **cfg)
    name, arg = strategy[0], (strategy[1] if len(strategy) > 1 else None)
    if name == "fixed":
        return list(arg)
    if name == "min_size":
        return min_size(degree_bits, c["rate_bits"], c["num_query_rounds"], arg)
    return constant_arity_bits(degree_bits, c["rate_bits"], c["cap_height"], c["fri_arity_bits"], c["fri_final_poly_bits"])


def strategy_of(entry):
    """[variant, payload] of tests/golden/ref_fri_plans.json -> (the backend's strategy, configuration overrides)"""
    variant, payload = entry
    if variant == "Fixed":
        return ("fixed", list(payload[0])), {}
    if variant == "MinSize":
        return ("min_size", payload[0]), {}
    return ("constant_arity_bits",), {"fri_arity_bits": payload[0], "fri_final_poly_bits": payload[1]}


# ------------------------------------------------------------------------------------------------ the commit phase under a plan
def fri_layers(trace_c, zs_c, quot_c, nperm, zeta, alpha, betas, arities, rate_bits=3):
    """opening_reference.fri_layers with the plan's own arity per layer: [(non-zero prefix as pairs, length)], first what the first
    layer commits, then what is left after each fold; the last entry is what the final polynomial is cut from"""
    assert len(betas) == len(arities), "one beta per layer of the reduction plan"
    n = len(trace_c[0])
    c, _ = R.composed_quotients(trace_c, zs_c, quot_c, nperm, zeta, alpha)
    out = [(c, n << rate_bits)]
    for ab, beta in zip(arities, betas):
        out.append(R.fold(out[-1][0], out[-1][1], R.ext(beta), 1 << ab))
    return out


def final_poly(layers, rate_bits=3):
    c, length = layers[-1]
    keep = length >> rate_bits
    return (c + [(0, 0)] * keep)[:keep]


def bit_reversed(length):
    bits = length.bit_length() - 1
    j = np.arange(length, dtype=np.uint64)
    rev = np.zeros(length, dtype=np.uint64)
    for b in range(bits):
        rev |= ((j >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return rev


def layer_caps(oracle, layers, arities, cap_height=4, merkle=None):
    """The Merkle caps of the committed layers (all of `layers` but the last), layer i with leaves of 2 * 2^arities[i] words: the
    polynomial's values on its coset in bit-reversed order, from the oracle's transform; the tree is the oracle's under the hasher it is
    set to, or `merkle(leaves, cap_height)` (Keccak: tests/keccak_ref.py)."""
    caps, shift = [], 7
    for (c, length), ab in zip(layers[:-1], arities):
        arity = 1 << ab
        planes = np.zeros((2, length), dtype=np.uint64)
        planes[:, :len(c)] = np.array(c, dtype=np.uint64).T
        va, vb = (oracle.evaluate_poly_with_offset(pl, shift, 1) for pl in planes)
        rev = bit_reversed(length)
        leaves = np.stack([va[rev], vb[rev]], axis=1).reshape(length // arity, 2 * arity)
        caps.append(merkle(leaves, cap_height) if merkle else oracle.merkle(leaves, cap_height))
        shift = pow(shift, arity, P)
    return caps
