"""tests/golden/ref_verified/wide_program_nch3.{proof,json} (tests/make_ref_verdict_nch.py): the GPU prover's proof of the full-size
instance under standard_fast_config with num_challenges = 3, and what the reference's verifier and prover, interpreted from their
source with that field set, said of it and of nineteen corruptions.

  * everywhere: the record belongs to the proof; the library's verifier host stage, built with g++ alone (tests/host_verify_check_nch.cpp
    over olavm_amd/csrc/verify_host.h), accepts the proof under three challenges, re-derives every challenge the reference recorded with
    the library's host challenger, refuses the proof under two, and resolves each corruption to the reference's reason and place;
  * where the reference tree is present: the interpreter's configuration carries the field, and encode and the challenges are repeated;
  * with -m gpu: ola_prove_with_traces returns the committed bytes and ola_verify_all_proof gives the recorded verdicts."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests.make_ref_verdict_nch import NOT_RUN, NUM_CHALLENGES, PROVE_TABLES_NCH
from tests.test_verify_host import expected

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")
STEM = "wide_program_nch3"
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}
reference = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def record():
    return json.load(open(os.path.join(DIR, STEM + ".json")))


@pytest.fixture(scope="module")
def raw():
    return open(os.path.join(DIR, STEM + ".proof"), "rb").read()


def test_record_belongs_to_the_proof_and_says_accepted(record, raw):
    import compare_with_dump as CD
    from olavm_amd.air import ola_tables as T
    from tests.make_ref_verdict import TAMPER
    assert len(raw) == record["proof_bytes"] < 1 << 20 and hashlib.sha256(raw).hexdigest() == record["proof_sha256"]
    assert record["config"] == "PoseidonGoldilocksConfig" and record["num_challenges"] == NUM_CHALLENGES == 3
    assert record["verify_proof"] == "Ok(())" and record["write_all_proof_reproduces_the_bytes"] is True
    assert record["verify_proof_under_standard_fast_config"].startswith("Err ")
    default = json.load(open(os.path.join(DIR, "wide_program.json")))
    assert record["trace_shapes"] == default["trace_shapes"]                           # the same instance as the two-challenge proof
    spans = {n.split(" (")[0]: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    s = T.ola_stark()
    for t, tab in enumerate(s.tables):                                                 # the widths three challenges give
        a, b = spans["table %d: openings.quotient_polys" % t]
        assert b - a == 16 * 3 * tab.quotient_degree_factor
        a, b = spans["table %d: openings.permutation_ctl_zs" % t]
        assert b - a == 16 * (tab.num_permutation_batches(3) + s.num_ctl_zs(t, 3))
    ch = record["challenges"]
    assert len(ch["ctl_challenges"]["challenges"]) == 3 and all(len(sc["stark_alphas"]) == 3 for sc in ch["stark_challenges"])
    for tab, sc in zip(s.tables, ch["stark_challenges"]):
        sets = sc["permutation_challenge_sets"] or []
        assert len(sets) == (tab.quotient_degree_factor if tab.permutation_pairs else 0) and all(len(cs["challenges"]) == 3 for cs in sets)
    assert [t["span"] for t in record["tampered"]] == list(TAMPER) and len(record["tampered"]) == 19
    stops = {t["reference"] for t in record["tampered"]}
    assert {"Err verifier.rs:295", "Err verifier.rs:52", "Err merkle_proofs.rs:71"} <= stops and "Ok(())" not in stops
    proved = record["prove_single_table"]
    assert [p["table"] for p in proved] == PROVE_TABLES_NCH and record["prove_single_table_not_run"] == NOT_RUN
    assert all(p["equal"] and p["transcript_after_equal"] for p in proved)


def test_host_stage_accepts_derives_the_challenges_and_places_the_corruptions(record, tmp_path):
    from olavm_amd.air import ola_tables as T
    blob = [int(x) for x in T.ola_stark().blob()]
    w = ["hasher", 0, "challenges", NUM_CHALLENGES, "proof", os.path.join(DIR, STEM + ".proof"), "blob", len(blob)] + blob
    ch = record["challenges"]
    w += ["ctl"] + [c[k] for c in ch["ctl_challenges"]["challenges"] for k in ("beta", "gamma")]
    w += ["tables", len(ch["stark_challenges"])]
    for s in ch["stark_challenges"]:
        perm = [c[k] for cs in (s["permutation_challenge_sets"] or []) for c in cs["challenges"] for k in ("beta", "gamma")]
        f = s["fri_challenges"]
        w += [len(perm)] + perm + s["stark_alphas"] + s["stark_zeta"] + f["fri_alpha"] + [len(f["fri_betas"])] + [x for b in f["fri_betas"] for x in b]
        w += [f["fri_pow_response"], len(f["fri_query_indices"])] + f["fri_query_indices"]
    w += ["cases", len(record["tampered"])]
    for t in record["tampered"]:
        w += [t["byte"], t["bit"]] + list(expected(t))
    cases = tmp_path / "cases.txt"
    cases.write_text(" ".join(str(x) for x in w) + "\n")
    exe = str(tmp_path / "host_verify_check_nch")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "host_verify_check_nch.cpp")])
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "19 cases, 0 failed" in r.stdout, r.stdout + r.stderr


@reference
def test_the_references_configuration_and_challenges_today(record, raw):
    import ref_verifier as V
    rv = V.RefVerifier("/root/reference", hasher="poseidon", num_challenges=NUM_CHALLENGES)
    plain = V.RefVerifier("/root/reference", hasher="poseidon")
    assert rv.config["num_challenges"] == 3 and plain.config["num_challenges"] == 2
    for f in plain.config["fri_config"]:
        if isinstance(plain.config["fri_config"][f], int):
            assert rv.config["fri_config"][f] == plain.config["fri_config"][f], f
    assert V.RefProver("/root/reference", num_challenges=NUM_CHALLENGES).config["num_challenges"] == 3
    proof = V.decode_all_proof(raw, "poseidon")
    assert rv.encode(proof) == raw
    assert rv.challenges(proof) == record["challenges"]


def span_place(span):
    import re
    m = re.match(r"table (\d+): ", span)
    table = int(m.group(1)) if m else int(re.match(r"compress_challenges\[(\d+)\]", span).group(1))
    q = re.search(r"fri\.query\[(\d+)\]\.(?:initial_trees_proof|step)\[(\d+)\]", span)
    return (table, int(q.group(1)), int(q.group(2))) if q else (table, None, None)


@pytest.mark.gpu
def test_gpu_returns_the_committed_bytes_and_the_recorded_verdicts(record, raw):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    blob = T.ola_stark().blob()
    traces, params, compress = instance()
    be, default = Backend(device=0, num_challenges=3), Backend(device=0)
    try:
        assert all(be.air_kernels_available(blob, 12))
        assert bytes(be.prove_with_traces(blob, traces, params, compress)) == raw, "ola_prove_with_traces at three challenges does not return the committed proof"
        res = be.verify_all_proof(blob, raw)
        assert res and res.reason == "OK" and (res.table, res.query, res.oracle_or_layer) == (None, None, None), res
        assert res.query_jobs == 28 * 12 and res.merkle_jobs == 28 * sum(3 + l for l in record["fri_layers"])
        for t in record["tampered"]:
            bad = bytearray(raw)
            bad[t["byte"]] ^= 1 << t["bit"]
            res = be.verify_all_proof(blob, bytes(bad))
            table, query, which = span_place(t["span"])
            assert not res and res.reason in REFERENCE[t["reference"]] and res.table == table, (t, res)      # where the reference's verifier stopped
            assert (res.query, res.oracle_or_layer) == (query, which), (t, res)
        res = default.verify_all_proof(blob, raw)                                        # standard_fast_config: a shape refusal at the first table
        assert not res and res.reason.startswith("SHAPE") and res.table == 0, res
    finally:
        be.close()
        default.close()
