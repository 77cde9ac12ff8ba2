#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_keccak.json: what the REFERENCE, run from its source (tools/ref_verifier.py --hasher keccak:
hash/keccak.rs interpreted, only `keccak_hash::keccak` under it restated), says of the GPU prover's proof of tests.make_ref_verdict.instance()
under KeccakGoldilocksConfig.  The oracle has no Keccak configuration, so wide_program_keccak.proof comes from `ola_prove_with_traces`
(tools/prove_fixture_keccak.py, on the GPU, first).

    python -m tests.make_ref_verdict_keccak --part verify | prover[=0,1,3] ...  then  --merge
    (needs the reference tree; the parts are independent and can run side by side)

  * verify  the interpreted `Buffer::write_all_proof` gives back the bytes, `verify_proof` returns Ok(()), every challenge of
            `AllProof::get_challenges`, and the verdict and place for the nineteen one-bit corruptions of tests/make_ref_verdict.py;
  * prover  the reference's `prove_single_table`, interpreted, for the given tables (default: the ten of make_ref_verdict.PROVE_TABLES):
            its StarkProof bytes against the proof's, proof-of-work witness included, and the transcript it leaves.
A verifier that refuses the proof, or a table whose bytes differ, stops the part: that is a defect to find, not a record to write.
tests/test_keccak.py ties the record to the proof; tests/test_gpu_keccak.py holds the GPU's bytes and verdicts to both."""
import hashlib
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_keccak"
REFERENCE = os.environ.get("OLA_REFERENCE", "/root/reference")
PARTS = os.environ.get("OLA_VERDICT_PARTS", os.path.join(tempfile.gettempdir(), "ola_ref_verdict_keccak"))
DIGEST_BYTES = 25


def _setup():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    import ref_verifier as V
    return V, CD


def part_verify(raw):
    from tests.make_ref_verdict import TAMPER, tamper
    V, CD = _setup()
    rv = V.RefVerifier(REFERENCE, hasher="keccak")
    proof = V.decode_all_proof(raw, "keccak")
    assert rv.encode(proof) == raw, "write_all_proof does not reproduce the bytes"
    challenges = rv.challenges(proof)
    t = time.time()
    ok, where = rv.verify(proof)
    print("reference verify_proof (KeccakGoldilocksConfig): %s (%.0f s)" % ("Ok(())" if ok else "Err at " + where, time.time() - t), flush=True)
    assert ok
    assert rv.challenges(proof) == challenges and rv.encode(proof) == raw          # the verifier left the proof as it was
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw, digest_bytes=DIGEST_BYTES)}
    tampered = []
    for name in TAMPER:
        bad, off = tamper(raw, spans, name)
        t = time.time()
        ok, where = rv.verify(bad)
        print("%-55s reference: %s (%.0f s)" % (name, "Ok(())" if ok else "Err " + where, time.time() - t), flush=True)
        tampered.append({"span": name, "byte": off, "bit": 0, "reference": "Ok(())" if ok else "Err " + where})
    return {"write_all_proof_reproduces_the_bytes": True, "verify_proof": "Ok(())", "challenges": challenges, "tampered": tampered}


def part_prover(raw, tables):
    from tests.make_ref_verdict import instance
    V, _ = _setup()
    traces, _, _ = instance()
    rp = V.RefProver(REFERENCE, hasher="keccak")
    out = []
    for k in tables:
        t = time.time()
        got, state_ok = rp.prove_table(raw, traces, k)
        a, b = V.table_span(raw, k, DIGEST_BYTES)
        out.append({"table": k, "rows": int(traces[k].shape[1]), "columns": int(traces[k].shape[0]), "bytes": b - a, "equal": got == raw[a:b],
                    "transcript_after_equal": bool(state_ok), "sha256": hashlib.sha256(got).hexdigest()})
        print("prove_single_table of table %d: equal %s, transcript after equal %s (%.0f s)" % (k, got == raw[a:b], state_ok, time.time() - t), flush=True)
        assert got == raw[a:b] and state_ok, "table %d: the interpreted prover's bytes or transcript differ" % k
    return {"prove_single_table": out}


def merge(raw):
    from tests.make_ref_verdict import PROVE_TABLES, instance
    traces, _, _ = instance()
    record = {"generated_by": "python -m tests.make_ref_verdict_keccak",
              "instance": "miniexec.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True; ola_stark(); standard_fast_config",
              "config": "KeccakGoldilocksConfig", "prover": "ola_prove_with_traces (GPU)",
              "trace_shapes": [[int(x) for x in tr.shape] for tr in traces],
              "proof_bytes": len(raw), "proof_sha256": hashlib.sha256(raw).hexdigest()}
    prove = []
    for f in sorted(os.listdir(PARTS)):
        part = json.load(open(os.path.join(PARTS, f)))
        if part.get("proof_sha256") != record["proof_sha256"]:
            raise SystemExit(f + " belongs to another proof")
        prove += part.pop("prove_single_table", [])
        part.pop("proof_sha256")
        record.update(part)
    record["prove_single_table"] = sorted(prove, key=lambda r: r["table"])
    record["prove_single_table_tables_not_run"] = sorted(set(PROVE_TABLES) - {r["table"] for r in prove})
    assert record.get("verify_proof") == "Ok(())"
    assert all(r["equal"] and r["transcript_after_equal"] for r in prove)
    open(os.path.join(OUT, STEM + ".json"), "w").write(json.dumps(record, indent=1) + "\n")
    print("wrote", os.path.join(OUT, STEM + ".json"))


def main():
    from tests.make_ref_verdict import PROVE_TABLES
    sys.setrecursionlimit(20000)
    raw = open(os.path.join(OUT, STEM + ".proof"), "rb").read()
    args = sys.argv[1:]
    if "--merge" in args:
        merge(raw)
        return
    os.makedirs(PARTS, exist_ok=True)
    name = args[args.index("--part") + 1]
    if name == "verify":
        data = part_verify(raw)
    elif name.startswith("prover"):
        tables = [int(x) for x in name.split("=", 1)[1].split(",")] if "=" in name else PROVE_TABLES
        data = part_prover(raw, tables)
    else:
        raise SystemExit("unknown part " + name)
    data["proof_sha256"] = hashlib.sha256(raw).hexdigest()
    open(os.path.join(PARTS, name.replace("=", "_").replace(",", "-") + ".json"), "w").write(json.dumps(data) + "\n")


if __name__ == "__main__":
    main()
