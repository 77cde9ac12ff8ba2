#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_poseidon2.json: what the REFERENCE, run from its source (tools/ref_verifier.py), says of the
GPU prover's proof of tests.make_ref_verdict.instance() under the fork's Poseidon2 configurations (the oracle proves under Poseidon and Blake3
only, so wide_program_poseidon2.proof comes from `ola_prove_with_traces`, tools/prove_fixture_poseidon2.py).

    python -m tests.make_ref_verdict_poseidon2 --part verify | config2 | prover[=0,1,3] ...  then  --merge
    (this container only: needs /root/reference; the parts are independent and can run side by side)

  * verify  (Poseidon2GoldilocksConfig): the interpreted `Buffer::write_all_proof` gives back the bytes, `verify_proof` returns Ok(()), every
            challenge of `AllProof::get_challenges`, and the verdict on the nineteen one-bit corruptions of tests/make_ref_verdict.py;
  * config2 (Poseidon2GoldilocksConfig2): the same transcript with a Poseidon proof of work.  The witness enters no challenge (F5), so the
            Config2 proof is the Poseidon2 proof with its twelve witnesses replaced; the interpreted verifier hands over the twelve inputs
            of C::InnerHasher::hash_no_pad (fri/challenges.rs:52), the minimal Poseidon nonce of each is searched with the oracle's Poseidon,
            and the patched proof is re-encoded and verified: Ok(()).  Recorded: its length, sha256, the inputs and the witnesses;
  * prover  the reference's `prove_single_table`, interpreted, for the given tables (default: the ten of make_ref_verdict.PROVE_TABLES):
            its StarkProof bytes against the proof's, proof-of-work witness included.
tests/test_poseidon2.py ties the record to the proof; tests/test_gpu_poseidon2.py holds the GPU's Config2 bytes to the recorded sha256."""
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_poseidon2"
PARTS = os.environ.get("OLA_VERDICT_PARTS", os.path.join(tempfile.gettempdir(), "ola_ref_verdict_poseidon2"))


def _setup():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    import ref_verifier as V
    return V, CD


def part_verify(raw):
    from tests.make_ref_verdict import TAMPER, tamper
    V, CD = _setup()
    rv = V.RefVerifier("/root/reference", hasher="poseidon2")
    proof = V.decode_all_proof(raw, "poseidon2")
    assert rv.encode(proof) == raw, "write_all_proof does not reproduce the bytes"
    challenges = rv.challenges(proof)
    ok, where = rv.verify(proof)
    print("reference verify_proof (Poseidon2GoldilocksConfig):", "Ok(())" if ok else "Err at " + where, flush=True)
    assert ok
    spans = {n: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    tampered = []
    for name in TAMPER:
        bad, off = tamper(raw, spans, name)
        t = time.time()
        ok, where = rv.verify(bad)
        print("%-55s reference: %s (%.0f s)" % (name, "Ok(())" if ok else "Err " + where, time.time() - t), flush=True)
        tampered.append({"span": name, "byte": off, "bit": 0, "reference": "Ok(())" if ok else "Err " + where})
    return {"write_all_proof_reproduces_the_bytes": True, "verify_proof": "Ok(())", "challenges": challenges, "tampered": tampered}


def min_poseidon_nonce(oracle, h, bits):
    """the smallest i with Poseidon.hash_no_pad(h || i)[0] below 2^(64 - bits) (fri/prover.rs:126-148 over PoseidonHash)"""
    x = np.zeros(5, dtype=np.uint64)
    x[:4] = h
    for i in range(1 << 40):
        x[4] = i
        if int(oracle.hash_no_pad(x)[0]) >> (64 - bits) == 0:
            return i


def part_config2(raw):
    from tests import oracle_lib
    V, CD = _setup()
    rv = V.RefVerifier("/root/reference", hasher="poseidon2_pow_poseidon")
    rv.challenges(V.decode_all_proof(raw, "poseidon2_pow_poseidon"))
    inputs = rv.it.pow_inputs
    assert len(inputs) == 12 and all(len(x) == 5 for x in inputs)
    bits = int(rv.config["fri_config"]["proof_of_work_bits"])
    oracle = oracle_lib.load()
    pows = [(a, b) for n, a, b in CD.parse_all_proof(raw) if n.endswith("pow_witness")]
    out = bytearray(raw)
    witnesses = []
    for (a, b), x in zip(pows, inputs):
        w = min_poseidon_nonce(oracle, np.array(x[:4], dtype=np.uint64), bits)
        witnesses.append(w)
        out[a:b] = int(w).to_bytes(8, "little")
    raw3 = bytes(out)
    rv.it.pow_inputs = []
    proof = V.decode_all_proof(raw3, "poseidon2_pow_poseidon")
    assert rv.encode(proof) == raw3
    ok, where = rv.verify(proof)
    print("reference verify_proof (Poseidon2GoldilocksConfig2):", "Ok(())" if ok else "Err at " + where, flush=True)
    assert ok
    return {"config2": {"config": "Poseidon2GoldilocksConfig2", "proof_bytes": len(raw3), "proof_sha256": hashlib.sha256(raw3).hexdigest(),
                        "verify_proof": "Ok(())", "pow_inputs": [[int(v) for v in x[:4]] for x in inputs], "pow_witnesses": witnesses}}


def part_prover(raw, tables):
    from tests.make_ref_verdict import instance
    V, _ = _setup()
    traces, _, _ = instance()
    rp = V.RefProver("/root/reference", hasher="poseidon2")
    out = []
    for k in tables:
        t = time.time()
        got, state_ok = rp.prove_table(raw, traces, k)
        a, b = V.table_span(raw, k)
        out.append({"table": k, "rows": int(traces[k].shape[1]), "columns": int(traces[k].shape[0]), "bytes": b - a, "equal": got == raw[a:b],
                    "transcript_after_equal": bool(state_ok), "sha256": hashlib.sha256(got).hexdigest()})
        print("prove_single_table of table %d: equal %s, transcript after equal %s (%.0f s)" % (k, got == raw[a:b], state_ok, time.time() - t), flush=True)
    return {"prove_single_table": out}


def merge(raw):
    from tests.make_ref_verdict import PROVE_TABLES, instance
    traces, _, _ = instance()
    record = {"generated_by": "python -m tests.make_ref_verdict_poseidon2",
              "instance": "miniexec.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True; ola_stark(); standard_fast_config",
              "config": "Poseidon2GoldilocksConfig", "prover": "ola_prove_with_traces (GPU)",
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
    assert "verify_proof" in record and "config2" in record
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
    elif name == "config2":
        data = part_config2(raw)
    elif name.startswith("prover"):
        tables = [int(x) for x in name.split("=", 1)[1].split(",")] if "=" in name else PROVE_TABLES
        data = part_prover(raw, tables)
    else:
        raise SystemExit("unknown part " + name)
    data["proof_sha256"] = hashlib.sha256(raw).hexdigest()
    open(os.path.join(PARTS, name.replace("=", "_").replace(",", "-") + ".json"), "w").write(json.dumps(data) + "\n")


if __name__ == "__main__":
    main()
