"""The stepped opening of the stress columns under a Fixed reduction plan, in a process of its own:

    python -m tests.fri_plan_child LOG_N HASHER PLAN SETS OUT.json        PLAN = 4,3,3 or - for no layer; SETS = random,x_zeta

The library reads OLA_POOL_POISON, OLA_FOLD16 and OLA_LEAF_EXT_STAGED once per process, so tests/test_gpu_fri_plans.py sets one in this
process' environment and compares what comes back: {set: {"final": [[a, b], ..], "caps": [[[4 words] x 16] per layer]}}.
`run_steps` and `commit_stress` are what the test uses in its own process too."""
import json
import sys

import numpy as np

from tests import opening_cases as OC


def commit_stress(be, oracle, log_n, cols=OC.MAIN_COLS):
    """the three batches of tests/opening_cases.py on the device -> (batches, coefficient lists)"""
    trace_c, zs_c, quot_c = OC.stress_batches(log_n, cols)
    batches = (be.commit(np.stack([oracle.evaluate_poly(c) for c in trace_c])),
               be.commit(np.stack([oracle.evaluate_poly(c) for c in zs_c])),
               be.commit(quot_c, from_coeffs=True))
    for b, want in zip(batches, (trace_c, zs_c, quot_c)):
        assert np.array_equal(b.coeffs(), want)
    return batches, [c.tolist() for c in (trace_c, zs_c, quot_c)]


def run_steps(be, batches, nperm, plan, zeta, alpha, betas):
    """set the plan, then ola_open -> begin -> next_layer .. -> finish -> free: (final polynomial as a list of pairs, layer caps)"""
    be.set_fri_reduction(("fixed", list(plan)))
    _, fri = be.open(*batches, nperm, zeta)
    try:
        assert fri.arity_bits == list(plan) and len(betas) == len(plan)
        fri.begin(alpha)
        beta, caps = None, []
        for b in betas:
            caps.append(fri.next_layer(beta))
            beta = b
        final = fri.finish(beta)
        assert final.shape == (fri.final_poly_len, 2)
    finally:
        fri.free()
    return [tuple(r) for r in final.tolist()], caps


def main(argv):
    if len(argv) != 5:
        print(__doc__, file=sys.stderr)
        return 2
    log_n, hasher, out = int(argv[0]), argv[1], argv[4]
    plan = [] if argv[2] == "-" else [int(x) for x in argv[2].split(",")]
    from olavm_amd.backend import Backend
    from tests import oracle_lib
    be = Backend(device=0, hasher=hasher)
    batches, _ = commit_stress(be, oracle_lib.load(), log_n)
    sets = {s[0]: s[1:] for s in OC.challenge_sets(log_n, len(plan))}
    result = {}
    for name in argv[3].split(","):
        zeta, alpha, betas = sets[name]
        final, caps = run_steps(be, batches, OC.MAIN_NPERM, plan, zeta, alpha, betas)
        result[name] = {"final": [[int(a), int(b)] for a, b in final], "caps": [c.tolist() for c in caps]}
    for b in batches:
        b.free()
    be.close()
    with open(out, "w") as f:
        json.dump(result, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
