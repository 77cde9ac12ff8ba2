#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_cfg.{proof,json}: the GPU prover's AllProof of tests.make_ref_verdict.instance() under
PoseidonGoldilocksConfig with a StarkConfig that is NOT standard_fast_config -- `config.fri_config.rate_bits = 4`, `cap_height = 2`,
`proof_of_work_bits = 12`, `num_query_rounds = 20` -- and what the REFERENCE, run from its source (tools/ref_verifier.py with
config_overrides), says of it.  Outside the default configuration the oracle is tied to the reference by this one proof.

    python -m tests.make_ref_verdict_config --prove [PATH]   on the GPU, first: Backend(rate_bits=4, cap_height=2, ...), ola_prove_with_traces
    python -m tests.make_ref_verdict_config                  needs the reference tree; about ten minutes

The record holds: the interpreted `Buffer::write_all_proof` gives back the bytes; `verify_proof` under the changed configuration returns
Ok(()); every challenge of `AllProof::get_challenges`; the verdict and the place for nineteen one-bit corruptions -- those of
tests/make_ref_verdict.py, a span the proof does not have (a query beyond the twenty) moved as tests/make_ref_verdict_minsize.py moves its
own; and the reference's verdict under standard_fast_config, which must refuse the proof.  A verifier that refuses the honest proof
stops the run: that is a defect to find, not a record to write.  tests/test_gpu_configs.py holds the GPU's bytes and verdicts to both
files, tests/test_ref_verifier.py the oracle's verifier."""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_cfg"
REFERENCE = os.environ.get("OLA_REFERENCE", "/root/reference")
CONFIG = {"rate_bits": 4, "cap_height": 2, "proof_of_work_bits": 12, "num_query_rounds": 20}
CFG = (4, 2, 12, 4, 5, 20)                      # the oracle's order: rate, cap, work, arity, final polynomial, queries
# twenty query rounds: the span of query 27 is taken from the last query the proof has
MOVED = {"table 4: fri.query[27].initial_trees_proof[2].path": "table 4: fri.query[19].initial_trees_proof[2].path"}


def tamper_list():
    from tests.make_ref_verdict import TAMPER
    return [MOVED.get(name, name) for name in TAMPER]


def prove(out):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    traces, params, compress = instance()
    be = Backend(device=0, hasher="poseidon", **CONFIG)
    raw = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
    again = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
    assert raw == again, "two runs give different bytes"
    be.close()
    open(out, "wb").write(raw)
    print("wrote", out, len(raw), "bytes")


def verdict(raw):
    from tests.make_ref_verdict import instance, tamper
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    import ref_verifier as V
    rv = V.RefVerifier(REFERENCE, hasher="poseidon", config_overrides=CONFIG)
    proof = V.decode_all_proof(raw, "poseidon")
    assert rv.encode(proof) == raw, "write_all_proof does not reproduce the bytes"
    challenges = rv.challenges(proof)
    t = time.time()
    ok, where = rv.verify(proof)
    print("reference verify_proof (PoseidonGoldilocksConfig, %s): %s (%.0f s)" % (CONFIG, "Ok(())" if ok else "Err at " + where, time.time() - t), flush=True)
    assert ok
    assert rv.challenges(proof) == challenges and rv.encode(proof) == raw          # the verifier left the proof as it was
    ok_default, where_default = V.RefVerifier(REFERENCE, hasher="poseidon").verify(raw)
    print("reference verify_proof under standard_fast_config: %s" % ("Ok(())" if ok_default else "Err " + where_default), flush=True)
    assert not ok_default
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    names = tamper_list()
    missing = [n for n in names if not n.startswith("compress_challenges[") and not any(s.startswith(n) for s in spans)]
    assert not missing, "spans the proof does not have: %s" % missing
    tampered = []
    for name in names:
        bad, off = tamper(raw, spans, name)
        t = time.time()
        ok, where = rv.verify(bad)
        print("%-55s reference: %s (%.0f s)" % (name, "Ok(())" if ok else "Err " + where, time.time() - t), flush=True)
        tampered.append({"span": name, "byte": off, "bit": 0, "reference": "Ok(())" if ok else "Err " + where})
    traces, _, _ = instance()
    layers = [len(s["fri_challenges"]["fri_betas"]) for s in challenges["stark_challenges"]]
    record = {"generated_by": "python -m tests.make_ref_verdict_config",
              "instance": "miniexec.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True; ola_stark(); standard_fast_config with "
                          "fri_config.rate_bits = 4, cap_height = 2, proof_of_work_bits = 12, num_query_rounds = 20",
              "config": "PoseidonGoldilocksConfig", "config_overrides": CONFIG, "oracle_cfg": list(CFG), "prover": "ola_prove_with_traces (GPU)",
              "trace_shapes": [[int(x) for x in tr.shape] for tr in traces], "fri_layers": layers,
              "proof_bytes": len(raw), "proof_sha256": hashlib.sha256(raw).hexdigest(),
              "write_all_proof_reproduces_the_bytes": True, "verify_proof": "Ok(())",
              "verify_proof_under_standard_fast_config": "Err " + where_default,
              "challenges": challenges, "tampered": tampered}
    open(os.path.join(OUT, STEM + ".json"), "w").write(json.dumps(record, indent=1) + "\n")
    print("wrote", os.path.join(OUT, STEM + ".json"))


def main():
    sys.setrecursionlimit(20000)
    path = os.path.join(OUT, STEM + ".proof")
    if "--prove" in sys.argv[1:]:
        k = sys.argv.index("--prove")
        prove(sys.argv[k + 1] if len(sys.argv) > k + 1 else path)
        return
    verdict(open(path, "rb").read())


if __name__ == "__main__":
    main()
