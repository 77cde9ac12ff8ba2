"""One job on the GPU in a process of its own: `python -m tests.alt_path_child [--dry] JOB OUT.json`.

The library reads its path switches (OLA_NTT2_TFORM, OLA_EVAL_WIDE, OLA_EVAL_WIDE_KH, OLA_FOLD16, OLA_LEAF_EXT_STAGED,
OLA_MERKLE_FUSED_LEVELS, OLA_POW_DEFER, OLA_POOL_POISON) once per process, so tests/test_gpu_fallback_paths.py sets one in this process' environment, runs one job and
reads the JSON file it leaves:

  transforms:L   the transform matrix of tests/transform_cases.py at 2^L against the oracle, with the pass kernels that
                 ola_gpu_ntt_pass_times saw (none when the canonical-arithmetic passes ran);
  open:HASHER    three seeded commitments of 2^15 rows (6, 3 and 2 columns, one permutation Z), ola_open_and_prove, the bytes
                 and the transcript's next challenge;
  prove          the 12-table padding instances of test_twelve_table_all_proof_bytes_match_oracle, the AllProof bytes;
  openeval:L     the stress columns of tests/opening_cases.py at 2^L rows (9, 5 and 4 columns, two permutation Zs) through the
                 stepped opening (ola_open .. ola_fri_commit_finish) at the challenge sets OPENEVAL_SETS, the opening-set bytes
                 the final polynomials and the layers' caps; the expected side is tests/opening_reference.py, not the oracle
                 (whose transform and tree turn the reference's folded polynomials into the expected caps).

The inputs and the oracle's side of each job are functions of this module, so that the parent computes the expected bytes
from the same inputs.  --dry builds both and opens no context (the GPU library is not even loaded)."""
import hashlib
import json
import sys
import time

import numpy as np

from tests import opening_cases as OC, opening_reference, oracle_lib, transform_cases as TC

OPENEVAL_SETS = ("random", "minus_ones", "order3_zeta")
OPEN_LOG_N, OPEN_COLS, OPEN_NUM_PERM_ZS = 15, (6, 3, 2), 1
PROVE_LOG_NS = (3, 8)


# ------------------------------------------------------------------------------------------------ inputs and the oracle side
def open_inputs():
    rng = np.random.default_rng(1500 + OPEN_LOG_N)
    return [oracle_lib.rand_field(rng, (c, 1 << OPEN_LOG_N)) for c in OPEN_COLS]


def open_expected(oracle, hasher):
    """(opening-set bytes, FRI proof bytes, the transcript's next challenge) of the oracle prover under `hasher`."""
    tv, zv, qc = open_inputs()
    with oracle.hasher(hasher):
        batches = [oracle.batch(tv), oracle.batch(zv), oracle.batch(qc, from_coeffs=True)]
        ch = oracle.challenger()
        for b in batches:
            ch.observe_cap(b.cap())
        _, o_open, o_fri = oracle.open_and_prove(*batches, OPEN_NUM_PERM_ZS, ch)
        return o_open, o_fri, ch.get()


def prove_inputs():
    from olavm_amd.air import ola_tables as T       # the AIR descriptions: Python only
    from tests import tracegen
    blob = T.ola_stark(range_bits=4, limb_bits=2).blob()
    return blob, [tracegen.empty_program_instance(log_n=log_n, live=np.random.default_rng(log_n)) for log_n in PROVE_LOG_NS]


def prove_expected(oracle):
    blob, instances = prove_inputs()
    return [oracle.prove_with_traces(blob, traces, params, compress) for traces, params, compress in instances]


def openeval_inputs(L):
    """(coefficient columns of the three batches, [(name, zeta, alpha, betas)])"""
    sets = [c for c in OC.challenge_sets(L, len(opening_reference.fri_arity_bits(L))) if c[0] in OPENEVAL_SETS]
    return OC.stress_batches(L, OC.MAIN_COLS), sets


def openeval_expected(L, oracle=None):
    """{set name: (opening-set bytes, final polynomial as a list of pairs, layer caps)} on Python integers; the caps (None without
    `oracle`) are the oracle's transform and Merkle tree over the reference's folded polynomials"""
    R = opening_reference
    batches, sets = openeval_inputs(L)
    coeffs = [b.tolist() for b in batches]
    out = {}
    for name, zeta, alpha, betas in sets:
        layers = R.fri_layers(*coeffs, OC.MAIN_NPERM, zeta, alpha, betas)
        out[name] = (R.open_set_bytes(R.open_set(*coeffs, OC.MAIN_NPERM, zeta)),
                     R.final_poly(*coeffs, OC.MAIN_NPERM, zeta, alpha, betas, layers=layers),
                     None if oracle is None else [c.tolist() for c in R.layer_caps(oracle, layers)])
    return out


def transform_inputs(L):
    return TC.stress_columns(L, TC.stress_rng(L))


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the jobs
def job_transforms(L, dry):
    oracle = oracle_lib.load()
    cols = transform_inputs(L)
    out = {"L": L, "ops": [], "mismatches": [], "seconds": {}}
    if dry:
        out["oracle_sha256"] = {}
        for op in TC.operations(L):
            want = TC.reference(oracle, op, L, cols)
            out["oracle_sha256"][op] = _sha(*[want[k] for k in sorted(want, key=repr)])
            out["ops"].append(op)
        return out
    from olavm_amd.backend import Backend
    be = Backend(device=0)
    be.ntt_pass_times(True)
    kernels = set()
    for op in TC.operations(L):
        want = TC.reference(oracle, op, L, cols)
        t0 = time.perf_counter()
        out["mismatches"] += [list(m) for m in TC.run_case(be, oracle, op, L, cols, want=want)]
        out["seconds"][op] = time.perf_counter() - t0
        kernels |= set(be.ntt_pass_times())
        out["ops"].append(op)
    out["pass_kernels"] = sorted(kernels)
    be.close()
    return out


def job_open(hasher, dry):
    tv, zv, qc = open_inputs()
    if dry:
        o_open, o_fri, nxt = open_expected(oracle_lib.load(), hasher)
        return {"oracle_sha256": _sha(o_open, o_fri), "challenge": nxt}
    from olavm_amd.backend import Backend, Challenger
    be = Backend(device=0, hasher=hasher)
    t0 = time.perf_counter()
    gt, gz, gq = be.commit(tv), be.commit(zv), be.commit(qc, from_coeffs=True)
    ch = Challenger(hasher=hasher)
    for b in (gt, gz, gq):
        ch.observe_cap(b.cap())
    g_open, g_fri = be.open_and_prove(gt, gz, gq, OPEN_NUM_PERM_ZS, ch)
    out = {"open": g_open.hex(), "fri": g_fri.hex(), "challenge": ch.get(), "caps": np.stack([gt.cap(), gz.cap(), gq.cap()]).tolist(),
           "seconds": time.perf_counter() - t0}
    for b in (gt, gz, gq):
        b.free()
    be.close()
    return out


def job_prove(dry):
    blob, instances = prove_inputs()
    if dry:
        return {"oracle_sha256": [_sha(p) for p in prove_expected(oracle_lib.load())]}
    from olavm_amd.backend import Backend
    be = Backend(device=0)
    t0 = time.perf_counter()
    proofs = [be.prove_with_traces(blob, traces, params, compress) for traces, params, compress in instances]
    be.close()
    return {"proofs": [p.hex() for p in proofs], "seconds": time.perf_counter() - t0}


def job_openeval(L, dry):
    (trace_c, zs_c, quot_c), sets = openeval_inputs(L)
    if dry:
        want = openeval_expected(L)
        return {"sets": [c[0] for c in sets], "reference_sha256": {k: _sha(v[0], np.array(v[1], dtype=np.uint64)) for k, v in want.items()}}
    oracle = oracle_lib.load()              # (for the values of the trace and Z columns: the library interpolates them back)
    from olavm_amd.backend import Backend
    be = Backend(device=0)
    t0 = time.perf_counter()
    gt = be.commit(np.stack([oracle.evaluate_poly(c) for c in trace_c]))
    gz = be.commit(np.stack([oracle.evaluate_poly(c) for c in zs_c]))
    gq = be.commit(quot_c, from_coeffs=True)
    out = {"sets": [c[0] for c in sets], "open": {}, "final": {}, "caps": {},
           "coeffs_kept": all(np.array_equal(b.coeffs(), c) for b, c in ((gt, trace_c), (gz, zs_c), (gq, quot_c)))}
    for name, zeta, alpha, betas in sets:
        opened, fri = be.open(gt, gz, gq, OC.MAIN_NPERM, zeta)
        fri.begin(alpha)
        beta, caps = None, []
        for b in betas:
            caps.append(fri.next_layer(beta).tolist())
            beta = b
        out["open"][name], out["final"][name], out["caps"][name] = opened.hex(), fri.finish(beta).tolist(), caps
        fri.free()
    out["seconds"] = time.perf_counter() - t0
    for b in (gt, gz, gq):
        b.free()
    be.close()
    return out


def main(argv):
    dry = "--dry" in argv
    args = [a for a in argv if a != "--dry"]
    if len(args) != 2:
        print("usage: python -m tests.alt_path_child [--dry] transforms:L | open:HASHER | prove | openeval:L  OUT.json", file=sys.stderr)
        return 2
    job, out_path = args
    kind, _, arg = job.partition(":")
    if kind == "transforms":
        out = job_transforms(int(arg), dry)
    elif kind == "open":
        out = job_open(arg, dry)
    elif kind == "prove":
        out = job_prove(dry)
    elif kind == "openeval":
        out = job_openeval(int(arg), dry)
    else:
        print("unknown job %r" % job, file=sys.stderr)
        return 2
    out["job"], out["dry"] = job, dry
    backend = sys.modules.get("olavm_amd.backend")
    out["gpu_library_loaded"] = bool(backend is not None and backend._lib is not None)
    with open(out_path, "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
