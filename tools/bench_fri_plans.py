#!/usr/bin/env python3
"""FRI reduction strategies on the padding instance of tools/bench_prove.py (12-table OlaStark, CPU and memory tables of 2^log_n rows).

  sizes   one process, per hasher a ConstantArityBits(4, 5) context and a MinSize(None) context taking turns round after round:
          seconds and proof bytes of both, the sha256 of the default proof (it must not move), and ola_verify_all_proof of each proof
          by its own context.
  ab      one process, one hasher, one strategy; the library reads OLA_FOLD16 and OLA_LEAF_EXT_STAGED once per process, so tools/gpu.sh
          starts this mode with both switches 1 / 0 / 1 / 0: wall, fold kernels and extension-leaf + commitment leaf kernels
          (ola_gpu_phase_stats; the leaf phase also holds the three oracles' leaves, which the switches do not touch), best of `rounds`.
No thresholds: docs/EXPERIMENTS.md records what it printed.
usage: python tools/bench_fri_plans.py sizes [log_n=22] [rounds=5] [--hashers blake3,keccak] [--json PATH]
       python tools/bench_fri_plans.py ab STRATEGY [log_n=22] [rounds=4] [--hasher blake3]      STRATEGY = min_size | min_size:3 | constant:2 | fixed:4,3 | default
A Fixed list serves all twelve tables, so one that suits the 2^22-row tables does not fit the small ones: MinSize(Some(3)) is the way to put
arity 8 on every layer of every table."""
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olavm_amd.air import ola_tables as T, tracegen  # noqa: E402
from olavm_amd.backend import Backend, fri_reduction_arity_bits  # noqa: E402


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def strategy_of(word):
    if word == "default":
        return ("constant_arity_bits",)
    if word.startswith("min_size"):
        return ("min_size", int(word.split(":", 1)[1]) if ":" in word else None)
    return ("fixed", [int(x) for x in word.split(":", 1)[1].split(",")])


skip = {"--hashers", "--hasher", "--json"}
args = [a for i, a in enumerate(sys.argv[1:]) if not a.startswith("--") and sys.argv[i] not in skip]
mode = args[0]
blob = T.ola_stark().blob()

if mode == "sizes":
    L = int(args[1]) if len(args) > 1 else 22
    rounds = int(args[2]) if len(args) > 2 else 5
    traces, params, compress = tracegen.empty_program_instance(log_n=10, range_bits=16, limb_bits=8, log_n_cpu=L, log_n_mem=L)
    heights = [int(t.shape[1]).bit_length() - 1 for t in traces]
    print("heights", heights, "MinSize(None) plans", [fri_reduction_arity_bits(("min_size", None), h) for h in heights], flush=True)
    out = {"log_n_cpu": L, "rounds": rounds, "heights": heights, "hashers": {}}
    for hasher in option("--hashers", "blake3,keccak").split(","):
        be = {"default": Backend(device=0, hasher=hasher), "min_size": Backend(device=0, hasher=hasher, fri_reduction=("min_size", None))}
        proofs = {k: bytes(b.prove_with_traces(blob, traces, params, compress)) for k, b in be.items()}      # first proofs: allocations, code objects
        for k, b in be.items():
            assert b.verify_all_proof(blob, proofs[k], params), k
        assert not be["default"].verify_all_proof(blob, proofs["min_size"], params)
        wall = {k: [] for k in be}
        for _ in range(rounds):
            for k, b in be.items():
                t0 = time.perf_counter()
                p = bytes(b.prove_with_traces(blob, traces, params, compress))
                wall[k].append((time.perf_counter() - t0) * 1e3)
                assert p == proofs[k]
        res = {k: {"median_ms": round(statistics.median(wall[k]), 2), "min_ms": round(min(wall[k]), 2), "max_ms": round(max(wall[k]), 2),
                   "proof_bytes": len(proofs[k]), "proof_sha256": hashlib.sha256(proofs[k]).hexdigest()} for k in be}
        out["hashers"][hasher] = res
        for k in be:
            print("%-8s %-9s prove %s" % (hasher, k, res[k]), flush=True)
        for b in be.values():
            b.close()
    if "--json" in sys.argv:
        open(option("--json", None), "w").write(json.dumps(out, indent=1) + "\n")
else:
    # constant:K = ConstantArityBits(K, 5) through the configuration: arity 2^K on every layer of every table
    extra = {"fri_arity_bits": int(args[1].split(":", 1)[1])} if args[1].startswith("constant:") else {}
    strategy = ("constant_arity_bits",) if extra else strategy_of(args[1])
    L = int(args[2]) if len(args) > 2 else 22
    rounds = int(args[3]) if len(args) > 3 else 4
    hasher = option("--hasher", "blake3")
    traces, params, compress = tracegen.empty_program_instance(log_n=10, range_bits=16, limb_bits=8, log_n_cpu=L, log_n_mem=L)
    be = Backend(device=0, hasher=hasher, fri_reduction=strategy, **extra)
    be.proof_stats(enable=True)
    best = None
    for _ in range(rounds):
        proof = be.prove_with_traces(blob, traces, params, compress)
        st, ph = be.proof_stats(), be.phase_stats()
        if best is None or st["wall_ms"] < best[0]:
            best = (st["wall_ms"], ph["fri_fold"][0], ph["fri_fold"][2] / 1e9, ph["leaf_hash"][0])
    print(hasher, args[1], "OLA_FOLD16=%s OLA_LEAF_EXT_STAGED=%s" % (os.environ.get("OLA_FOLD16", "1"), os.environ.get("OLA_LEAF_EXT_STAGED", "1")),
          "wall %.1f ms, folds %.3f ms (%.2f G coefficients), leaf kernels %.2f ms" % best, "proof %d bytes sha256 %s" % (len(proof), hashlib.sha256(bytes(proof)).hexdigest()[:16]))
    be.close()
