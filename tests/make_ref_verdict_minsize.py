#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_blake3_minsize.{proof,json}: the GPU prover's AllProof of tests.make_ref_verdict.instance()
under Blake3GoldilocksConfig with `config.fri_config.reduction_strategy = FriReductionStrategy::MinSize(None)`, and what the REFERENCE,
run from its source (tools/ref_verifier.py), says of it.  The oracle folds with constant arities only, so the proof comes from the device.

    python -m tests.make_ref_verdict_minsize --prove      on the GPU, first: ola_gpu_set_fri_reduction(OLA_FRI_MIN_SIZE), ola_prove_with_traces
    python -m tests.make_ref_verdict_minsize              needs the reference tree; about seven minutes

The tables of the instance have 2^3 .. 2^18 rows, so the plans are [] (up to 2^9 rows), [3] (2^10), [4, 4] (2^16) and [4, 3, 3] (2^18).
The record holds: the interpreted `Buffer::write_all_proof` gives back the bytes; `verify_proof` returns Ok(()); every challenge of
`AllProof::get_challenges`; the verdict and the place for nineteen one-bit corruptions -- those of tests/make_ref_verdict.py, with the two
spans that tables 0 and 10 no longer have (they have no FRI layer under MinSize) taken from table 5; and the reference's verdict under
its default ConstantArityBits(4, 5), which must refuse the proof.  A verifier that refuses the honest proof stops the run: that is a
defect to find, not a record to write.  tests/test_gpu_fri_plans.py holds the GPU's bytes and verdicts to both files."""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_blake3_minsize"
REFERENCE = os.environ.get("OLA_REFERENCE", "/root/reference")
MOVED = {"table 10: fri.commit_phase_merkle_caps[0]": "table 5: fri.commit_phase_merkle_caps[0]",
         "table 0: fri.query[9].step[0].path": "table 5: fri.query[9].step[0].path"}


def tamper_list():
    from tests.make_ref_verdict import TAMPER
    return [MOVED.get(name, name) for name in TAMPER]


def prove(out):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    traces, params, compress = instance()
    be = Backend(device=0, hasher="blake3", fri_reduction=("min_size", None))
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
    rv = V.RefVerifier(REFERENCE, hasher="blake3", reduction_strategy=("MinSize", [None]))
    proof = V.decode_all_proof(raw, "blake3")
    assert rv.encode(proof) == raw, "write_all_proof does not reproduce the bytes"
    challenges = rv.challenges(proof)
    t = time.time()
    ok, where = rv.verify(proof)
    print("reference verify_proof (Blake3GoldilocksConfig, MinSize(None)): %s (%.0f s)" % ("Ok(())" if ok else "Err at " + where, time.time() - t), flush=True)
    assert ok
    assert rv.challenges(proof) == challenges and rv.encode(proof) == raw          # the verifier left the proof as it was
    ok_default, where_default = V.RefVerifier(REFERENCE, hasher="blake3").verify(raw)
    print("reference verify_proof under ConstantArityBits(4, 5): %s" % ("Ok(())" if ok_default else "Err " + where_default), flush=True)
    assert not ok_default
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    tampered = []
    for name in tamper_list():
        bad, off = tamper(raw, spans, name)
        t = time.time()
        ok, where = rv.verify(bad)
        print("%-55s reference: %s (%.0f s)" % (name, "Ok(())" if ok else "Err " + where, time.time() - t), flush=True)
        tampered.append({"span": name, "byte": off, "bit": 0, "reference": "Ok(())" if ok else "Err " + where})
    traces, _, _ = instance()
    layers = [len(s["fri_challenges"]["fri_betas"]) for s in challenges["stark_challenges"]]
    record = {"generated_by": "python -m tests.make_ref_verdict_minsize",
              "instance": "miniexec.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True; ola_stark(); standard_fast_config with "
                          "fri_config.reduction_strategy = FriReductionStrategy::MinSize(None)",
              "config": "Blake3GoldilocksConfig", "reduction_strategy": "MinSize(None)", "prover": "ola_prove_with_traces (GPU)",
              "trace_shapes": [[int(x) for x in tr.shape] for tr in traces], "fri_layers": layers,
              "proof_bytes": len(raw), "proof_sha256": hashlib.sha256(raw).hexdigest(),
              "write_all_proof_reproduces_the_bytes": True, "verify_proof": "Ok(())",
              "verify_proof_under_constant_arity_bits_4_5": "Err " + where_default,
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
