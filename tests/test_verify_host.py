"""The verifier's host stage without a device (olavm_amd/csrc/verify_host.h, PARITY.md "verification").

tests/host_verify_check.cpp is a stand-alone program over the header: built here with g++ alone -- no HIP, no library -- and run on
the three committed proofs of tests/golden/ref_verified/ with what the REFERENCE's verifier, interpreted from its source, recorded
of them (the .json beside each proof):
  * the host stage accepts each proof and derives the challenges of the record's `challenges` block;
  * each of the 19 one-bit corruptions that the reference rejects at verifier.rs:295 (the quotient identity) or verifier.rs:52 (the
    proof of work) is rejected by the host stage with that reason at the span's table -- a corrupted compress_challenges[2] / [10]
    at tables 2 / 10, whose constraint parameter it is;
  * those the reference rejects at merkle_proofs.rs:71 or verifier.rs:218 pass the host stage and leave their job in the list, and
    that job's flag alone resolves to the reference's reason and place;
  * truncation at 2 000 seeded lengths and every length prefix set to all ones are refused as malformed.
The same program is built a second time with -fsanitize=address,undefined and run again (every eighth truncation and prefix)."""
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")

STEMS = {"poseidon": ("wide_program", 0), "blake3": ("wide_program_blake3", 1), "poseidon2": ("wide_program_poseidon2", 2)}
# include/ola_gpu.h OLA_VERIFY_*
QUOTIENT_IDENTITY, POW, MERKLE_INITIAL, FRI_CONSISTENCY, MERKLE_COMMIT = 7, 17, 18, 19, 20


def expected(t):
    """(where, reason, table, query, kind, which) of a record's corruption: where the reference stopped, in the report's terms"""
    span, ref = t["span"], t["reference"]
    m = re.match(r"table (\d+): ", span)
    table = int(m.group(1)) if m else int(re.match(r"compress_challenges\[(\d+)\]", span).group(1))
    if ref == "Err verifier.rs:295":
        return 0, QUOTIENT_IDENTITY, table, -1, 0, -1
    if ref == "Err verifier.rs:52":
        return 0, POW, table, -1, 0, -1
    q = re.search(r"fri\.query\[(\d+)\]\.(initial_trees_proof|step)\[(\d+)\]", span)
    query, kind, which = int(q.group(1)), 0 if q.group(2) == "initial_trees_proof" else 1, int(q.group(3))
    if ref == "Err merkle_proofs.rs:71":
        return 1, MERKLE_COMMIT if kind else MERKLE_INITIAL, table, query, kind, which
    assert ref == "Err verifier.rs:218" and kind == 1, t          # the flipped bit is in the value the consistency check reads
    return 2, FRI_CONSISTENCY, table, query, kind, which


def case_file(path, config):
    from olavm_amd.air import ola_tables as T
    stem, hasher = STEMS[config]
    rec = json.load(open(os.path.join(DIR, stem + ".json")))
    blob = [int(x) for x in T.ola_stark().blob()]
    w = ["hasher", hasher, "proof", os.path.join(DIR, stem + ".proof"), "blob", len(blob)] + blob
    ch = rec["challenges"]
    w += ["ctl"] + [c[k] for c in ch["ctl_challenges"]["challenges"] for k in ("beta", "gamma")]
    w += ["tables", len(ch["stark_challenges"])]
    for s in ch["stark_challenges"]:
        perm = [c[k] for cs in (s["permutation_challenge_sets"] or []) for c in cs["challenges"] for k in ("beta", "gamma")]
        f = s["fri_challenges"]
        w += [len(perm)] + perm + s["stark_alphas"] + s["stark_zeta"] + f["fri_alpha"] + [len(f["fri_betas"])] + [x for b in f["fri_betas"] for x in b]
        w += [f["fri_pow_response"], len(f["fri_query_indices"])] + f["fri_query_indices"]
    assert len(rec["tampered"]) == 19 and all(t["reference"] != "Ok(())" for t in rec["tampered"])
    w += ["cases", len(rec["tampered"])]
    for t in rec["tampered"]:
        w += [t["byte"], t["bit"]] + list(expected(t))
    open(path, "w").write(" ".join(str(x) for x in w) + "\n")
    return rec


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + extra +
                          ["-o", exe, os.path.join(HERE, "host_verify_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_verify")
    return {"plain": build(d, "host_verify_check", ["-O2"]),
            "sanitized": build(d, "host_verify_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


@pytest.mark.parametrize("config", ["poseidon", "blake3", "poseidon2"])
def test_host_stage_on_the_committed_proofs(programs, tmp_path, config):
    cases = str(tmp_path / "cases.txt")
    rec = case_file(cases, config)
    kinds = [expected(t)[0] for t in rec["tampered"]]
    assert kinds.count(0) == 14 and kinds.count(1) + kinds.count(2) == 5        # 14 for the host stage, 5 only the device can see
    r = subprocess.run([programs["plain"], cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "19 cases, 0 failed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("config", ["poseidon", "blake3", "poseidon2"])
def test_host_stage_is_clean_under_the_sanitizers(programs, tmp_path, config):
    cases = str(tmp_path / "cases.txt")
    case_file(cases, config)
    r = subprocess.run([programs["sanitized"], cases, "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "19 cases, 0 failed" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr


def test_usage_without_arguments(programs):
    r = subprocess.run([programs["plain"]], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
