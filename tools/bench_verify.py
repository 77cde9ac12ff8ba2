"""Times ola_verify_all_proof on a proof of tools/bench_prove.py's instance (the 12-table OlaStark, empty-program execution of a given
CPU-table height): the host stage and the device stage of the report separately, the oracle's verify_all_proof on the same bytes in the
same process, and the job counts.  Usage: python tools/bench_verify.py [log_n_cpu] [reps] [--json PATH]; OLA_HASHER = poseidon | blake3"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from olavm_amd.air import ola_tables as T, tracegen
from olavm_amd.backend import Backend
from tests import oracle_lib

args = [a for a in sys.argv[1:] if not a.startswith("--")]
L = int(args[0]) if len(args) > 0 else 18
reps = int(args[1]) if len(args) > 1 else 5
out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
HASHER = os.environ.get("OLA_HASHER", "poseidon")
blob = T.ola_stark().blob()
traces, params, compress = tracegen.empty_program_instance(log_n=10, range_bits=16, limb_bits=8, log_n_cpu=L, log_n_mem=L)
be = Backend(device=0, hasher=HASHER)
proof = bytes(be.prove_with_traces(blob, traces, params, compress))
runs = []
for r in range(reps):
    t0 = time.perf_counter()
    res = be.verify_all_proof(blob, proof, params)
    wall = (time.perf_counter() - t0) * 1e3
    assert res, res
    runs.append({"wall_ms": wall, "host_ms": res.host_ms, "device_ms": res.device_ms})
o = oracle_lib.load()
oracle_ms = []
with o.hasher(HASHER):
    for r in range(max(1, reps // 2)):
        t0 = time.perf_counter()
        rc, why = o.verify_all_proof(blob, proof, params)
        oracle_ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, why
best = min(runs, key=lambda x: x["wall_ms"])
rec = {"hasher": HASHER, "log_n_cpu": L, "proof_bytes": len(proof), "merkle_jobs": res.merkle_jobs, "query_jobs": res.query_jobs,
       "kernel_launches": res.kernel_launches, "runs": runs, "best": best, "oracle_ms": oracle_ms}
print("%s 2^%d rows, proof %d bytes: ola_verify_all_proof %.2f ms (host stage %.2f ms, device stage %.2f ms; first call %.2f ms), "
      "oracle verify_all_proof %.1f ms; %d Merkle jobs, %d query jobs, %d launches"
      % (HASHER, L, len(proof), best["wall_ms"], best["host_ms"], best["device_ms"], runs[0]["wall_ms"], min(oracle_ms), res.merkle_jobs, res.query_jobs,
         res.kernel_launches), flush=True)
if out:
    json.dump(rec, open(out, "w"), indent=1)
