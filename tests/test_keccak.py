"""KeccakGoldilocksConfig (plonky2/plonky2/src/plonk/config.rs:145-151), CPU side.  Nothing on a test machine computes Keccak-256, so the chain
of evidence starts at hashlib: tests/keccak_ref.py's permutation and sponge with the domain byte 0x06 are SHA3-256, and with 0x01 give the
two published Keccak-256 digests.  From there: the committed vectors are a fresh derivation; the reference's own hash/keccak.rs, interpreted
from source with only `keccak_hash::keccak` under it restated a third time, gives them; the library's host code (the header the kernels are
compiled from) gives them, stand-alone under the sanitizers too; the committed proof belongs to the record of the reference's verdict on it,
and the library's host stage accepts it under Keccak only and re-derives every challenge of that record."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import keccak_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "olavm_amd", "csrc")
DIR = os.path.join(HERE, "golden", "ref_verified")
VECTORS = os.path.join(HERE, "golden", "keccak_vectors.json")
PROOF = os.path.join(DIR, "wide_program_keccak.proof")
RECORD = os.path.join(DIR, "wide_program_keccak.json")
REFERENCE = os.environ.get("OLA_REFERENCE", "/root/reference")
U64P = C.POINTER(C.c_uint64)
OLA_HASH_KECCAK = 5


def _p(a):
    return a.ctypes.data_as(U64P)


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(VECTORS))


@pytest.fixture(scope="module")
def lib():
    from olavm_amd.backend import load_library
    return load_library()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_is_sha3_with_the_other_domain_byte_and_gives_the_published_digests():
    for n in list(range(0, 301)) + [271, 272]:          # 135, 136, 137 and 271, 272: one byte short of a block, a block, a block and a byte
        d = bytes((i * 7 + n) % 256 for i in range(n))
        assert K.sha3_256(d) == hashlib.sha3_256(d).digest(), n
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert K.keccak256(b"abc") != hashlib.sha3_256(b"abc").digest()


def test_vectorised_sponge_and_tree_equal_the_integer_form():
    rng = np.random.default_rng(1)
    for n in (0, 1, 8, 50, 135, 136, 137, 272, 752):
        m = rng.integers(0, 256, (5, n), dtype=np.uint8)
        got = K.sponge256_np(m)
        assert [g.tobytes() for g in got] == [K.keccak256(r.tobytes()) for r in m], n
        assert [g.tobytes() for g in K.sponge256_np(m, 0x06)] == [hashlib.sha3_256(r.tobytes()).digest() for r in m], n
    leaves = rng.integers(0, 2**64, (32, 19), dtype=np.uint64)
    for cap_h in (0, 2, 5):
        tree = K.MerkleTree(leaves, cap_h)
        level = [K.hash_no_pad(r.tolist()) for r in leaves]
        while len(level) > (1 << cap_h):
            level = [K.two_to_one(level[i], level[i + 1]) for i in range(0, len(level), 2)]
        assert [K.digest_bytes(d) for d in tree.cap()] == level
        for j in (0, 13, 31):
            assert K.verify_to_cap(leaves[j].tolist(), j, tree.prove(j), tree.cap())
            assert not K.verify_to_cap(leaves[j].tolist(), j ^ 1, tree.prove(j), tree.cap())


def test_vectors_file_is_a_fresh_derivation(vectors):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_keccak_vectors as mk
    assert mk.derive() == vectors
    assert sorted(len(v["input"]) for v in vectors["hash_no_pad"]) == [0, 1, 2, 15, 16, 17, 18, 33, 34, 35, 94, 134, 135, 136, 137]
    assert len(vectors["permutation"]) == 8 and len(vectors["challenger"]) == 6
    r = vectors["rejecting_state"]
    assert r["input"][1:] == [0] * 11 and len(r["rejected"]) >= 1 and all(w >= K.P for w in r["rejected"])
    assert any(w >> 32 == 0xFFFFFFFF and w & 0xFFFFFFFF for w in r["h1_words"])


# ---------------------------------------------------------------------------------------------------------------- the reference's source
@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference tree is not on this machine")
def test_interpreted_keccak_rs_gives_the_vectors(vectors):
    """hash/keccak.rs (hash_no_pad, two_to_one, KeccakPermutation::permute) interpreted from the reference's source; under it only
    `keccak_hash::keccak`, a crate outside the tree, is tools/ref_verifier.py's own Keccak-256"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_verifier as V
    from rust_air_eval import Fe
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    it = V.verifier_interp(REFERENCE, True, "keccak")
    rs = os.path.join(it.plonky2, "hash", "keccak.rs")

    def words(h):
        return K.digest_words(bytes(int(x) for x in h[0]))
    for v in vectors["hash_no_pad"]:
        assert words(it.call_assoc("KeccakHash", "hash_no_pad", [[Fe(x) for x in v["input"]]], rs)) == v["digest"], len(v["input"])
    for v in vectors["two_to_one"]:
        l, r = (V.bytes_hash(K.digest_bytes(v[k])) for k in ("left", "right"))
        assert words(it.call_assoc("KeccakHash", "two_to_one", [l, r], rs)) == v["digest"]
    for v in vectors["permutation"] + [vectors["rejecting_state"]]:
        assert [x.v for x in it.call_assoc("KeccakPermutation", "permute", [[Fe(x) for x in v["input"]]], rs)] == v["output"]
    hs = os.path.join(it.plonky2, "hash", "hash_types.rs")
    for v in vectors["digest_elements"]:
        got = it.call_assoc("BytesHash", "to_vec", [], hs, self_val=V.bytes_hash(K.digest_bytes(v["digest"])), has_self=True)
        assert [x.v for x in got] == v["elements"]


# ---------------------------------------------------------------------------------------------------------------- the library's host code
def replay(script, ch):
    outs = []
    for op in script["ops"]:
        if op[0] == "observe":
            ch.observe(np.array(op[1], dtype=np.uint64))
        elif op[0] == "observe_cap":
            ch.observe_cap(np.array(op[1], dtype=np.uint64).reshape(-1, 4))
        elif op[0] == "get":
            outs.append([int(x) for x in ch.get(op[1])])
        else:
            ch.compact()
            outs.append([int(x) for x in ch.state()])
    return outs, [int(x) for x in ch.state()]


def test_library_host_hash_and_challenger_equal_the_vectors(lib, vectors):
    from olavm_amd.backend import Challenger, HASHERS
    assert HASHERS["keccak"] == OLA_HASH_KECCAK
    out = np.zeros(4, dtype=np.uint64)
    for v in vectors["hash_no_pad"]:
        x = np.array(v["input"], dtype=np.uint64)
        if x.size == 0:
            continue
        assert lib.ola_keccak_hash_elements(_p(x), x.size, _p(out)) == 0
        assert out.tolist() == v["digest"], x.size
        if int(x[-1]) == 0:                                                      # a word >= p hashes as its canonical value
            x[-1] = np.uint64(K.P)
            assert lib.ola_keccak_hash_elements(_p(x), x.size, _p(out)) == 0 and out.tolist() == v["digest"]
    x = np.zeros(4097, dtype=np.uint64)
    assert lib.ola_keccak_hash_elements(_p(x), 0, _p(out)) != 0 and lib.ola_keccak_hash_elements(_p(x), 4097, _p(out)) != 0
    for script in vectors["challenger"]:
        outs, state = replay(script, Challenger(lib, "keccak"))
        assert outs == script["outputs"] and state == script["state"]
    # the permutation alone: eight observed elements over a zero state are one duplexing of (e0 .. e7, 0, 0, 0, 0)
    for v in vectors["permutation"] + [vectors["rejecting_state"]]:
        if v["input"][8:] != [0] * 4:
            continue
        ch = Challenger(lib, "keccak")
        ch.observe(np.array(v["input"][:8], dtype=np.uint64))
        assert [int(s) for s in ch.state()] == v["output"]
    assert sum(1 for v in vectors["permutation"] if v["input"][8:] == [0] * 4) >= 1
    for v in vectors["digest_elements"]:                                         # a digest is observed as its four elements
        a, b = Challenger(lib, "keccak"), Challenger(lib, "keccak")
        a.observe_cap(np.array(v["digest"], dtype=np.uint64).reshape(1, 4))
        b.observe(np.array(v["elements"], dtype=np.uint64))
        assert [int(x) for x in a.get(8)] == [int(x) for x in b.get(8)]
    import ctypes
    from olavm_amd.backend import OlaChallenger
    ch = OlaChallenger()
    assert lib.ola_challenger_init_keccak(ctypes.byref(ch)) == 0 and ch.hasher == OLA_HASH_KECCAK
    # ola_challenger_init_hasher keeps the range it was published with (tests/test_poseidon2.py pins 4 and 5 as refused there)
    assert all(lib.ola_challenger_init_hasher(ctypes.byref(ch), h) != 0 for h in (4, 5, 6))


def test_config_validation_takes_hasher_5_and_refuses_4_and_6(lib):
    """ola_gpu_init reads the configuration before it looks for a device: hasher 5 passes the validation and gets as far as the device --
    OLA_E_NO_DEVICE (-2) on a machine without one, never OLA_E_INVALID_ARG (-1); a context where there is one -- while 4 and 6 are
    OLA_E_INVALID_ARG on either machine"""
    from olavm_amd.backend import OlaGpuConfig
    for hasher, allowed in ((5, (0, -2)), (0, (0, -2)), (4, (-1,)), (6, (-1,))):
        cfg = OlaGpuConfig(0, None, 3, 4, 16, 4, 5, 28, 2, hasher)
        ctx = C.c_void_p()
        rc = lib.ola_gpu_init(C.byref(cfg), C.byref(ctx))
        assert rc in allowed, (hasher, rc)
        if rc == 0:
            lib.ola_gpu_free(ctx)


def hx(xs):
    return " ".join("%x" % int(x) for x in xs)


def keccak_cases(path, vectors):
    """the case file of tests/host_keccak_check.cpp: the vectors, widths 0..300 afresh, and word streams that reject 1, 2 and 12 words in a row"""
    rng = random.Random(300)
    lines = []
    for v in vectors["hash_no_pad"]:
        lines.append("hash %x %s %s" % (len(v["input"]), hx(v["input"]), hx(v["digest"])))
    for n in range(0, 301):
        xs = [rng.randrange(K.P) for _ in range(n)]
        lines.append("hash %x %s %s" % (n, hx(xs), hx(K.digest_words(K.hash_no_pad(xs)))))
        if n in (0, 4, 12, 17, 34):
            full = K.keccak256(K.words_bytes(xs))
            lines.append("full %x %s %s" % (n, hx(xs), hx(int.from_bytes(full[8 * i:8 * i + 8], "little") for i in range(4))))
    for v in vectors["two_to_one"]:
        lines.append("node %s %s %s" % (hx(v["left"]), hx(v["right"]), hx(v["digest"])))
    for v in vectors["permutation"] + [vectors["rejecting_state"]]:
        lines.append("perm %s %s" % (hx(v["input"]), hx(v["output"])))
    for v in vectors["digest_elements"]:
        lines.append("elems %s %s" % (hx(v["digest"]), hx(v["elements"])))
    for rejects, at in ((1, 0), (2, 3), (12, 5), (1, 11)):
        keep = [rng.randrange(K.P) for _ in range(12)]
        stream = keep[:at] + [K.P + rng.randrange(2**32 - 1) for _ in range(rejects)] + keep[at:]
        assert K.onion_select(stream) == keep
        lines.append("onion %x %s %s" % (len(stream), hx(stream), hx(keep)))
    lines.append("onion c %s %s" % (hx([K.P - 1] * 12), hx([K.P - 1] * 12)))                   # p - 1 is kept, p itself is not
    lines.append("onion d %s %s" % (hx([K.P] + [0] * 12), hx([0] * 12)))
    open(path, "w").write("\n".join(lines) + "\n")
    return len(lines)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_standalone_host_program_over_the_header(tmp_path, vectors, build):
    """tests/host_keccak_check.cpp with g++ alone, and again with -fsanitize=address,undefined, run as a program"""
    exe = str(tmp_path / "host_keccak_check")
    extra = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I" + CSRC] + extra +
                          ["-o", exe, os.path.join(HERE, "host_keccak_check.cpp")])
    cases = str(tmp_path / "cases.txt")
    count = keccak_cases(cases, vectors)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "%d cases, 0 failures" % count in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- the proof and its record
@pytest.fixture(scope="module")
def record():
    return json.load(open(RECORD))          # a missing fixture is a failure


def test_record_and_proof_belong_together(record):
    from tests.make_ref_verdict import PROVE_TABLES, TAMPER, instance
    raw = open(PROOF, "rb").read()
    assert record["config"] == "KeccakGoldilocksConfig"
    assert record["proof_bytes"] == len(raw) and record["proof_sha256"] == hashlib.sha256(raw).hexdigest()
    assert record["verify_proof"] == "Ok(())" and record["write_all_proof_reproduces_the_bytes"] is True
    traces, _, _ = instance()
    assert record["trace_shapes"] == [[int(x) for x in t.shape] for t in traces]
    assert [t["span"] for t in record["tampered"]] == TAMPER and all(t["reference"].startswith("Err ") for t in record["tampered"])
    ran = [r["table"] for r in record["prove_single_table"]]
    assert sorted(ran + record["prove_single_table_tables_not_run"]) == PROVE_TABLES and len(ran) >= 3
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_verifier as V
    for r in record["prove_single_table"]:
        assert r["equal"] and r["transcript_after_equal"], r["table"]
        a, b = V.table_span(raw, r["table"], 25)
        assert b - a == r["bytes"] and hashlib.sha256(raw[a:b]).hexdigest() == r["sha256"]
        assert [r["columns"], r["rows"]] == record["trace_shapes"][r["table"]]
    # 25-byte digests: the proof is shorter than the Blake3 proof of the same instance by 7 bytes a digest, and by nothing else
    b3 = open(os.path.join(DIR, "wide_program_blake3.proof"), "rb").read()
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as CD
    k_spans, b_spans = CD.parse_all_proof(raw, digest_bytes=25), CD.parse_all_proof(b3)
    assert [n for n, _, _ in k_spans] == [n for n, _, _ in b_spans]
    for (n, a, b), (_, a3, b3_) in zip(k_spans, b_spans):
        digests = "cap" in n or n.endswith(".path")
        assert (b - a) * (32 if digests else 1) == (b3_ - a3) * (25 if digests else 1), n


@pytest.fixture(scope="module")
def host_stage_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_keccak_verify")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        out[name] = str(d / ("host_keccak_verify_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + extra +
                              ["-o", out[name], os.path.join(HERE, "host_keccak_verify_check.cpp")])
    return out


def write_stage_cases(path, monkeypatch):
    from tests import test_verify_host as TV
    monkeypatch.setitem(TV.STEMS, "keccak", ("wide_program_keccak", OLA_HASH_KECCAK))
    return TV.case_file(path, "keccak")


def test_host_stage_accepts_the_proof_and_rederives_every_challenge(host_stage_programs, tmp_path, monkeypatch):
    """verify_host.h alone: the committed proof is accepted, the product's host challenger gives every challenge of the record
    (`AllProof::get_challenges` as the reference derived them), each corruption resolves to the reference's reason and place, truncations
    and length prefixes of all ones are malformed"""
    cases = str(tmp_path / "cases.txt")
    write_stage_cases(cases, monkeypatch)
    r = subprocess.run([host_stage_programs["plain"], cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "19 cases, 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    r = subprocess.run([host_stage_programs["sanitized"], cases, "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "19 cases, 0 failed" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]


def test_host_stage_refuses_the_proof_under_the_other_hashers(host_stage_programs, tmp_path, monkeypatch):
    cases = str(tmp_path / "cases.txt")
    write_stage_cases(cases, monkeypatch)
    r = subprocess.run([host_stage_programs["plain"], cases, "as", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hasher 5: accepted" in r.stdout, r.stdout + r.stderr
    for other in (0, 1, 2, 3):
        r = subprocess.run([host_stage_programs["plain"], cases, "as", str(other)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "hasher %d: rejected" % other in r.stdout, r.stdout + r.stderr
