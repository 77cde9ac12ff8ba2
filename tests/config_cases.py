"""Case tables of tests/test_gpu_configs.py: StarkConfig values other than standard_fast_config, as the six integers the oracle takes,
(rate_bits, cap_height, proof_of_work_bits, fri_arity_bits, fri_final_poly_bits, num_query_rounds), and the walk through an opening
proof's bytes that the corruption cases need.  No LDE of a case exceeds 2^16 points."""
import struct

DEFAULT = (3, 4, 16, 4, 5, 28)
FIELDS = ("rate_bits", "cap_height", "proof_of_work_bits", "fri_arity_bits", "fri_final_poly_bits", "num_query_rounds")


def kwargs(cfg):
    """the six integers as Backend(**kwargs)"""
    return dict(zip(FIELDS, cfg))


def cfg_id(cfg):
    return "r%d-c%d-w%d-a%d-f%d-q%d" % tuple(cfg)


# 1. commitments: (rate_bits, cap_height) -> log_n.  log_n + rate_bits >= cap_height, with equality (depth 0: the leaves' digests are the
# cap) in (8, 13) and (3, 16); (3, 9) has a cap above the 256 nodes that launch_merkle_build's last launch takes; (4, 7) and (5, 2) have
# levels on both sides of it; the LDE is 2^8 .. 2^16 points.
COMMIT = [((1, 0), 9), ((1, 4), 7), ((2, 1), 10), ((4, 7), 8), ((5, 2), 9), ((8, 13), 5), ((8, 0), 6), ((3, 9), 11), ((3, 16), 13), ((3, 0), 8)]
COMMIT_COLS = 5

# 2. opening proofs: (cfg, log_n, the FRI plan the oracle gives, the verifier takes the configuration)
OPENING = [((1, 4, 16, 4, 5, 28), 12, [4, 4], True),       # LDE of 2 cosets, 2^13 points
           ((2, 0, 1, 1, 0, 1), 7, [1] * 7, True),         # cap of one digest, one query, 1-bit work, final polynomial of one coefficient
           ((4, 7, 10, 2, 3, 84), 9, [2, 2, 2], True),     # 16 cosets, 84 queries
           ((8, 13, 8, 4, 5, 3), 5, [], True),             # 256 cosets, depth 0, no layer
           ((8, 0, 8, 3, 0, 3), 6, [3, 3], True),          # 256 cosets, paths down to the root
           ((3, 9, 16, 4, 5, 28), 10, [4], True),          # cap above top = 256 of launch_merkle_build
           ((3, 16, 16, 4, 5, 28), 13, [], True),          # largest cap, depth 0
           ((3, 0, 16, 4, 5, 1024), 8, [4], True),         # the largest query count
           ((5, 2, 20, 4, 5, 28), 10, [4, 4], True),       # 20-bit work
           ((3, 4, 16, 5, 5, 28), 10, [5], False),         # arity 32: prover only, the verifier supports arities of 2 to 16
           ((3, 4, 16, 6, 0, 28), 9, [6], False),          # arity 64
           ((3, 4, 8, 7, 0, 4), 8, [7], False),            # arity 128: wider than gather_ext_leaves_kernel's 64 threads
           ((3, 0, 8, 8, 0, 4), 8, [8], False)]            # arity 256
OPENING_COLS, OPENING_NPERM = (5, 4, 2), 2

# 3. the stepped ABI
STEPPED = [((2, 0, 1, 1, 0, 1), 7), ((4, 7, 10, 2, 3, 84), 9)]

# 4. whole proofs.  The miniature 12-table set has constraint degrees 7, 8, 3, 3, 3, 7, 3, 4, 5, 1, 3, 4: its quotients live on 2, 4 or 8
# cosets, fewer than the LDE has under these rates (step = 2 .. 32), and a rate below 8 cannot hold them
MINI_DEGREES = [7, 8, 3, 3, 3, 7, 3, 4, 5, 1, 3, 4]
MINI_PROVEN = [(4, 4, 16, 4, 5, 28), (4, 0, 1, 1, 0, 1), (8, 1, 10, 3, 2, 5), (5, 5, 12, 2, 1, 100)]
MINI_REFUSED = [(2, 1, 8, 4, 5, 28), (1, 1, 8, 4, 5, 28)]
DEGREE_WORDS = "Having constraints of degree higher than the rate is not supported yet."
TWO_TABLES = [(2, 1, 8, 4, 5, 28), (1, 1, 8, 4, 5, 28), (3, 0, 16, 4, 5, 1024)]         # cmp + rangecheck, degrees 3 and 3
NO_ORACLE = (4, 2, 12, 4, 5, 20)                                                      # Poseidon2 and Keccak: the product against itself

# 5. proof of work
POW_BITS = [1, 8, 12, 20]
POW_SECOND_LAUNCH = (1012, 25, 12, 19073)        # seed, draw, bits, the minimal witness the oracle finds: beyond the first 2^14 nonces

# 6. the proof held to the reference (tests/make_ref_verdict_config.py)
REFERENCE_CFG = (4, 2, 12, 4, 5, 20)


def opening_spans(proof_fri, cols, depth0, plan_depths):
    """Where the parts of FriProof bytes lie (serialization.rs:305-317; a digest is 32 bytes under Poseidon and Blake3): -> dict of
    name -> (offset, length) for query 0's first opened row and first initial path, its first layer's evaluations and path, the final
    polynomial's words and the witness.  depth0 = the initial trees' path length, plan_depths = [(arity, path length)] per layer.
    A part of length 0 is one the proof does not have."""
    at = 0
    (ncaps,) = struct.unpack_from("<I", proof_fri, at)
    at += 4
    assert ncaps == len(plan_depths)
    for _ in range(ncaps):
        (k,) = struct.unpack_from("<I", proof_fri, at)
        at += 4 + 32 * k
    (nq,) = struct.unpack_from("<I", proof_fri, at)
    at += 4
    spans = {}
    for q in range(nq):
        (three,) = struct.unpack_from("<I", proof_fri, at)
        assert three == 3
        at += 4
        for i, c in enumerate(cols):
            (k,) = struct.unpack_from("<I", proof_fri, at)
            assert k == c
            if q == 0 and i == 0:
                spans["row"] = (at + 4, 8 * c)
            at += 4 + 8 * c
            assert proof_fri[at] == depth0
            if q == 0 and i == 0:
                spans["initial_path"] = (at + 1, 32 * depth0)
            at += 1 + 32 * depth0
        (steps,) = struct.unpack_from("<I", proof_fri, at)
        assert steps == len(plan_depths)
        at += 4
        for li, (arity, depth) in enumerate(plan_depths):
            (k,) = struct.unpack_from("<I", proof_fri, at)
            assert k == arity
            if q == 0 and li == 0:
                spans["layer_leaf"] = (at + 4, 16 * arity)
            at += 4 + 16 * arity
            assert proof_fri[at] == depth
            if q == 0 and li == 0:
                spans["layer_path"] = (at + 1, 32 * depth)
            at += 1 + 32 * depth
    (k,) = struct.unpack_from("<I", proof_fri, at)
    spans["final_poly"] = (at + 4, 16 * k)
    at += 4 + 16 * k
    spans["witness"] = (at, 8)
    assert at + 8 == len(proof_fri)
    return spans
