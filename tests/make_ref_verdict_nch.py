#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_nch3.{proof,json}: the GPU prover's AllProof of tests.make_ref_verdict.instance() under
PoseidonGoldilocksConfig and standard_fast_config with `config.num_challenges = 3`, and what the REFERENCE, run from its source
(tools/ref_verifier.py with num_challenges=3), says of it.  The oracle's C interface cannot set the challenge count, so outside two
challenges this one proof is what ties the prover to the reference.

    python -m tests.make_ref_verdict_nch --prove [PATH]   on the GPU, first: Backend(num_challenges=3), ola_prove_with_traces
    python -m tests.make_ref_verdict_nch                  needs the reference tree; about ten minutes

The record holds: the interpreted `Buffer::write_all_proof` gives back the bytes; `verify_proof` with three challenges returns Ok(());
every challenge of `AllProof::get_challenges` (three lookup pairs, three alphas and permutation_batch_size x 3 pairs per table); the
verdict and the place for the nineteen one-bit corruptions of tests/make_ref_verdict.py; the reference's verdict under
standard_fast_config, which must refuse the proof; and the reference's interpreted `prove_single_table` at three challenges writing the
proof's bytes for the tables of PROVE_TABLES_NCH (tests/make_ref_verdict.PROVE_TABLES lists what the two-challenge record covers; the
rest was not run here: NOT_RUN).  A verifier that refuses the honest proof stops the run: that is a defect to find, not a record to write.
tests/test_ref_verdict_nch.py holds the library's host stages and, with -m gpu, the GPU's bytes and verdicts to both files."""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_nch3"
REFERENCE = os.environ.get("OLA_REFERENCE", "/root/reference")
NUM_CHALLENGES = 3
PROVE_TABLES_NCH = [3]                           # what tests/test_ref_verifier.py::test_the_references_prover_today re-proves: the cmp table
NOT_RUN = [0, 1, 5, 6, 7, 8, 9, 10, 11]          # the other tables of tests/make_ref_verdict.PROVE_TABLES


def prove(out):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    traces, params, compress = instance()
    be = Backend(device=0, hasher="poseidon", num_challenges=NUM_CHALLENGES)
    raw = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
    again = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
    assert raw == again, "two runs give different bytes"
    assert be.verify_all_proof(T.ola_stark().blob(), raw)
    be.close()
    open(out, "wb").write(raw)
    print("wrote", out, len(raw), "bytes")


def verdict(raw):
    from tests.make_ref_verdict import PROVE_TABLES, TAMPER, instance, tamper
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    import ref_verifier as V
    assert sorted(PROVE_TABLES_NCH + NOT_RUN) == sorted(PROVE_TABLES)
    rv = V.RefVerifier(REFERENCE, hasher="poseidon", num_challenges=NUM_CHALLENGES)
    proof = V.decode_all_proof(raw, "poseidon")
    assert rv.encode(proof) == raw, "write_all_proof does not reproduce the bytes"
    challenges = rv.challenges(proof)
    t = time.time()
    ok, where = rv.verify(proof)
    print("reference verify_proof (PoseidonGoldilocksConfig, num_challenges = %d): %s (%.0f s)" % (NUM_CHALLENGES, "Ok(())" if ok else "Err at " + where, time.time() - t), flush=True)
    assert ok
    assert rv.challenges(proof) == challenges and rv.encode(proof) == raw          # the verifier left the proof as it was
    ok_default, where_default = V.RefVerifier(REFERENCE, hasher="poseidon").verify(raw)
    print("reference verify_proof under standard_fast_config: %s" % ("Ok(())" if ok_default else "Err " + where_default), flush=True)
    assert not ok_default
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    missing = [n for n in TAMPER if not n.startswith("compress_challenges[") and not any(s.startswith(n) for s in spans)]
    assert not missing, "spans the proof does not have: %s" % missing
    tampered = []
    for name in TAMPER:
        bad, off = tamper(raw, spans, name)
        t = time.time()
        ok, where = rv.verify(bad)
        print("%-55s reference: %s (%.0f s)" % (name, "Ok(())" if ok else "Err " + where, time.time() - t), flush=True)
        tampered.append({"span": name, "byte": off, "bit": 0, "reference": "Ok(())" if ok else "Err " + where})
    traces, _, _ = instance()
    rp = V.RefProver(REFERENCE, hasher="poseidon", num_challenges=NUM_CHALLENGES)
    proved = []
    for k in PROVE_TABLES_NCH:
        t = time.time()
        got, state_ok = rp.prove_table(raw, traces, k)
        a, b = V.table_span(raw, k)
        proved.append({"table": k, "rows": int(traces[k].shape[1]), "columns": int(traces[k].shape[0]), "bytes": b - a, "equal": got == raw[a:b],
                       "transcript_after_equal": bool(state_ok), "sha256": hashlib.sha256(got).hexdigest()})
        print("prove_single_table of table %d at %d challenges: %d bytes, equal %s, transcript after equal %s (%.0f s)" % (
            k, NUM_CHALLENGES, b - a, got == raw[a:b], state_ok, time.time() - t), flush=True)
    assert all(x["equal"] and x["transcript_after_equal"] for x in proved)
    layers = [len(s["fri_challenges"]["fri_betas"]) for s in challenges["stark_challenges"]]
    record = {"generated_by": "python -m tests.make_ref_verdict_nch",
              "instance": "miniexec.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True; ola_stark(); standard_fast_config with "
                          "num_challenges = 3",
              "config": "PoseidonGoldilocksConfig", "num_challenges": NUM_CHALLENGES, "prover": "ola_prove_with_traces (GPU)",
              "trace_shapes": [[int(x) for x in tr.shape] for tr in traces], "fri_layers": layers,
              "proof_bytes": len(raw), "proof_sha256": hashlib.sha256(raw).hexdigest(),
              "write_all_proof_reproduces_the_bytes": True, "verify_proof": "Ok(())",
              "verify_proof_under_standard_fast_config": "Err " + where_default,
              "challenges": challenges, "tampered": tampered, "prove_single_table": proved, "prove_single_table_not_run": NOT_RUN}
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
