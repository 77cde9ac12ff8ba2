"""tests/golden/ref_verified/wide_program_cfg.{proof,json} (tests/make_ref_verdict_config.py): the GPU prover's proof of the full-size
instance under rate_bits 4, cap_height 2, 12-bit proof of work and 20 query rounds, and what the reference's verifier, interpreted from its
source with those four fields of `StarkConfig::standard_fast_config().fri_config` changed, said of it and of nineteen corruptions.

  * everywhere: the record belongs to the proof; the ORACLE's verifier under cfg = (4, 2, 12, 4, 5, 20) accepts the proof, gives the
    reference's verdict on every corruption at the reference's place, and refuses the proof under the default configuration as the
    reference did -- outside the default configuration this is what ties the oracle, the checker of tests/test_gpu_configs.py, to the
    reference;
  * where the reference tree is present: the interpretation is repeated (the overrides, encode, challenges, verify, one corruption);
  * the GPU side is tests/test_gpu_configs.py::test_committed_configuration_proof_and_its_nineteen_corruptions."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests.make_ref_verdict_config import CFG, CONFIG, MOVED, tamper_list
from tests.verdicts import oracle_says

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}
reference = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def record():
    return json.load(open(os.path.join(DIR, "wide_program_cfg.json")))


@pytest.fixture(scope="module")
def raw():
    return open(os.path.join(DIR, "wide_program_cfg.proof"), "rb").read()


def test_record_belongs_to_the_proof_and_says_accepted(record, raw):
    import compare_with_dump as CD
    assert len(raw) == record["proof_bytes"] and hashlib.sha256(raw).hexdigest() == record["proof_sha256"]
    assert record["config"] == "PoseidonGoldilocksConfig" and record["config_overrides"] == CONFIG and tuple(record["oracle_cfg"]) == CFG
    assert record["verify_proof"] == "Ok(())" and record["write_all_proof_reproduces_the_bytes"] is True
    assert record["verify_proof_under_standard_fast_config"].startswith("Err ")
    default = json.load(open(os.path.join(DIR, "wide_program.json")))
    assert record["trace_shapes"] == default["trace_shapes"]                           # the same instance as the default configuration's proof
    spans = {n.split(" (")[0]: (a, b) for n, a, b in CD.parse_all_proof(raw)}
    assert sum(n.endswith("trace_cap") for n in spans) == 12
    a, b = spans["table 0: trace_cap"]
    assert b - a == 32 * (1 << CFG[1])                                                 # a cap of 2^2 digests
    assert "table 0: fri.query[19].initial_trees_proof[0].leaf" in spans and not any("fri.query[20]" in n for n in spans)   # twenty queries
    assert [t["span"] for t in record["tampered"]] == tamper_list() and len(record["tampered"]) == 19
    assert all(new in [t["span"] for t in record["tampered"]] for new in MOVED.values())
    stops = {t["reference"] for t in record["tampered"]}
    assert {"Err verifier.rs:295", "Err verifier.rs:52", "Err merkle_proofs.rs:71"} <= stops and "Ok(())" not in stops


def test_oracle_verifier_under_the_configuration_agrees_with_the_reference(record, raw, oracle):
    from olavm_amd.air import ola_tables as T
    blob = T.ola_stark().blob()
    compress = np.frombuffer(raw[-96:], dtype="<u8")
    params = [int(compress[2]), int(compress[10])]
    assert oracle.verify_all_proof(blob, raw, params, cfg=CFG) == (0, "")
    for t in record["tampered"]:
        bad = bytearray(raw)
        bad[t["byte"]] ^= 1 << t["bit"]
        c = np.frombuffer(bytes(bad[-96:]), dtype="<u8")                                # a corrupted compress challenge is the AIR parameter it is
        rc, msg = oracle.verify_all_proof(blob, bytes(bad), [int(c[2]), int(c[10])], cfg=CFG)
        ok, reason, table = oracle_says(rc, msg)
        assert not ok and reason in REFERENCE[t["reference"]], (t["span"], msg)         # where the reference's verifier stopped
        named = t["span"].split(":")[0]
        assert table == (int(named[len("table "):]) if named.startswith("table ") else int(t["span"][len("compress_challenges["):-1])), (t["span"], msg)
    rc, msg = oracle.verify_all_proof(blob, raw, params)                                # standard_fast_config: a shape refusal, as the reference's
    # `ensure!(trace_cap.height() == cap_height)` of the first table's validate_proof_shape (verifier.rs:363)
    assert record["verify_proof_under_standard_fast_config"] == "Err verifier.rs:363"
    assert oracle_says(rc, msg) == (False, "SHAPE_CAP_HEIGHT", 0), msg


@reference
def test_the_references_verifier_under_the_configuration_today(record, raw):
    import ref_verifier as V
    rv = V.RefVerifier("/root/reference", hasher="poseidon", config_overrides=CONFIG)
    plain = V.RefVerifier("/root/reference", hasher="poseidon")
    for field, value in CONFIG.items():
        assert rv.config["fri_config"][field] == value != plain.config["fri_config"][field]
    for field in plain.config["fri_config"]:
        if field not in CONFIG and isinstance(plain.config["fri_config"][field], int):
            assert rv.config["fri_config"][field] == plain.config["fri_config"][field], field
    with pytest.raises(ValueError):
        V.RefVerifier("/root/reference", config_overrides={"num_challenges": 3})
    proof = V.decode_all_proof(raw, "poseidon")
    assert rv.encode(proof) == raw
    assert rv.challenges(proof) == record["challenges"]
    assert rv.verify(proof) == (True, None)
    t = record["tampered"][0]
    bad = bytearray(raw)
    bad[t["byte"]] ^= 1 << t["bit"]
    ok, where = rv.verify(bytes(bad))
    assert ("Ok(())" if ok else "Err " + where) == t["reference"]
