#!/usr/bin/env python3
"""KeccakGoldilocksConfig beside the other configurations: the padding instance of tools/bench_prove.py (12-table OlaStark, CPU and memory tables
of 2^log_n rows) proven under Keccak, Blake3 and Poseidon in ONE process, the three contexts taking turns round after round, and
ola_verify_all_proof of the Keccak proof timed in the same rounds.  Prints medians and spans, and the leaf-hash kernels' share of the proof
(ola_gpu_phase_stats).  No thresholds: docs/EXPERIMENTS.md records what it printed.
usage: python tools/bench_keccak.py [log_n_cpu=22] [rounds=5] [--json PATH]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olavm_amd.air import ola_tables as T, tracegen  # noqa: E402
from olavm_amd.backend import Backend  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
L = int(args[0]) if args else 22
rounds = int(args[1]) if len(args) > 1 else 5
blob = T.ola_stark().blob()
traces, params, compress = tracegen.empty_program_instance(log_n=10, range_bits=16, limb_bits=8, log_n_cpu=L, log_n_mem=L)
print("heights", [int(t.shape[1]).bit_length() - 1 for t in traces], flush=True)
HASHERS = ["keccak", "blake3", "poseidon"]
be = {h: Backend(device=0, hasher=h) for h in HASHERS}
proofs = {}
for h in HASHERS:                                   # first proof of each context: allocations, code objects
    be[h].proof_stats(enable=True)
    proofs[h] = bytes(be[h].prove_with_traces(blob, traces, params, compress))
assert be["keccak"].verify_all_proof(blob, proofs["keccak"], params)
assert not be["blake3"].verify_all_proof(blob, proofs["keccak"], params)
wall = {h: [] for h in HASHERS}
leaf = {h: [] for h in HASHERS}
levels = {h: [] for h in HASHERS}
verify = []
for r in range(rounds):
    for h in HASHERS:
        t0 = time.perf_counter()
        p = bytes(be[h].prove_with_traces(blob, traces, params, compress))
        wall[h].append((time.perf_counter() - t0) * 1e3)
        assert p == proofs[h]
        ph = be[h].phase_stats()
        leaf[h].append(ph["leaf_hash"][0])
        levels[h].append(ph["merkle_levels"][0])
    t0 = time.perf_counter()
    res = be["keccak"].verify_all_proof(blob, proofs["keccak"], params)
    verify.append((time.perf_counter() - t0) * 1e3)
    assert res


def line(xs):
    return {"median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2), "max_ms": round(max(xs), 2)}


out = {"log_n_cpu": L, "rounds": rounds, "proof_bytes": {h: len(proofs[h]) for h in HASHERS}, "prove": {}, "verify_all_proof_keccak": line(verify)}
for h in HASHERS:
    out["prove"][h] = dict(line(wall[h]), leaf_hash_ms=round(statistics.median(leaf[h]), 2), merkle_levels_ms=round(statistics.median(levels[h]), 2),
                           leaf_hash_share=round(statistics.median(leaf[h]) / statistics.median(wall[h]), 3))
    print("%-8s prove %s  leaf kernels %.2f ms (%.1f %% of the proof), Merkle levels %.2f ms, %d bytes" % (
        h, out["prove"][h], out["prove"][h]["leaf_hash_ms"], 100 * out["prove"][h]["leaf_hash_share"], out["prove"][h]["merkle_levels_ms"], len(proofs[h])))
print("verify_all_proof (keccak)", out["verify_all_proof_keccak"])
if "--json" in sys.argv:
    open(sys.argv[sys.argv.index("--json") + 1], "w").write(json.dumps(out, indent=1) + "\n")
for b in be.values():
    b.close()
