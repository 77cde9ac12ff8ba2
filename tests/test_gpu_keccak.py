"""GPU parity under the reference's KeccakGoldilocksConfig (plonky2/plonky2/src/plonk/config.rs:145-151): Merkle trees and the challenger
on Keccak-256 truncated to 25 bytes (hash/keccak.rs), proof of work on Poseidon.  Every call goes through the C ABI of a context
created with hasher = OLA_HASH_KECCAK.  The checker is tests/keccak_ref.py -- Python integers, pinned to hashlib.sha3_256 and the
published Keccak-256 digests by tests/test_keccak.py -- over the oracle's transforms (which do not depend on the hasher) and
tests/opening_reference.py's folded polynomials; whole proofs are pinned by tests/golden/ref_verified/wide_program_keccak.proof,
which the reference's own verifier, run from source, accepted (wide_program_keccak.json).

Size thresholds of the launch code (olavm_amd/csrc/merkle.hip), both sides of each are among the cases:
  * launch_merkle_build fuses levels (merkle_levels_bytes_kernel) while a level has more than 256 nodes: trees of 512 leaves
    (commit log_n 6) have none, of 1024 leaves (log_n 7) one fused launch of one level, of 2048 and more two levels per launch;
    levels of 256 nodes and fewer go to merkle_top_bytes_kernel.
  * launch_leaf_hash_ext stages arity-16 leaves through LDS (leaf_bytes_ext_tile_kernel<H, 4>) from 1024 leaves: the first FRI layer of a
    2^10-row opening has 512 leaves (direct kernel), of a 2^11-row opening 1024 (staged).
  * two FRI layers start at 2^10 rows (ConstantArityBits(4, 5), rate 3, cap height 4)."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from olavm_amd.air import miniexec as M, ola_tables as T
from tests import keccak_ref as K, opening_reference as R, tracegen
from tests.oracle_lib import P, rand_field

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")
PROOF = os.path.join(DIR, "wide_program_keccak.proof")
RECORD = os.path.join(DIR, "wide_program_keccak.json")
MINI = dict(range_bits=4, limb_bits=2)
DB = K.DIGEST_BYTES


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0, hasher="keccak")
    yield b
    b.close()


def test_config_validation_takes_hasher_5_and_refuses_4_and_6():
    import ctypes as C
    from olavm_amd.backend import OlaGpuConfig, load_library
    L = load_library()
    for hasher, want in ((5, 0), (4, -1), (6, -1)):
        cfg = OlaGpuConfig(0, None, 3, 4, 16, 4, 5, 28, 2, hasher)
        ctx = C.c_void_p()
        assert L.ola_gpu_init(C.byref(cfg), C.byref(ctx)) == want, hasher
        if want == 0:
            L.ola_gpu_free(ctx)


def well_formed(d):
    """digests in device memory: 4 words, word 3 holds byte 24 only"""
    d = np.asarray(d, dtype=np.uint64).reshape(-1, 4)
    return bool(np.all(d[:, 3] < np.uint64(256)))


# ---------------------------------------------------------------------------------------------------------------- hashing
@pytest.mark.parametrize("row_len", [1, 2, 15, 16, 17, 18, 33, 34, 35, 94, 134, 135, 136, 137, 300])
def test_hash_rows(be, row_len):
    """KeccakHash<25>::hash_no_pad of every row: the two pad bytes in one word (16 mod 17), in two words, the extra all-padding block
    (0 mod 17), one to eighteen blocks; words >= p hash as their canonical value"""
    rng = np.random.default_rng(row_len)
    for nrows in (1, 63, 300):
        rows = rng.integers(0, 2**64, (nrows, row_len), dtype=np.uint64)
        rows[0, 0] = np.uint64(P + 1)
        rows[nrows - 1, row_len - 1] = np.uint64(2**64 - 1)
        got = be.hash_rows(rows)
        assert well_formed(got)
        assert np.array_equal(got, K.hash_rows(rows)), nrows
        reduced = np.where(rows >= np.uint64(P), rows - np.uint64(P), rows)
        assert np.any(reduced != rows)
        assert np.array_equal(be.hash_rows(reduced), got), nrows
    one = rng.integers(0, P, row_len, dtype=np.uint64)                       # and one row against the integer form of the restatement
    assert be.hash_rows(one.reshape(1, -1))[0].tolist() == K.digest_words(K.hash_no_pad(one.tolist()))


@pytest.mark.parametrize("log_leaves,width,cap_h", [(4, 5, 4), (5, 3, 4), (9, 12, 4), (8, 33, 0), (6, 2, 2), (13, 7, 4), (10, 134, 3),
                                                    (3, 2, 3), (10, 3, 0), (11, 2, 4)])
def test_merkle_cap(be, log_leaves, width, cap_h):
    """the cap is the leaf level (cap_height = log_leaves), the root (0), and levels between; trees below, at and above the fused levels"""
    rng = np.random.default_rng(log_leaves + width)
    leaves = rand_field(rng, (1 << log_leaves, width))
    got = be.merkle_cap(leaves, cap_h)
    assert well_formed(got)
    assert np.array_equal(got, K.MerkleTree(leaves, cap_h).cap())


@pytest.mark.parametrize("log_n,ncols", [(1, 1), (3, 2), (5, 3), (6, 2), (7, 2), (8, 12), (10, 9), (12, 29), (9, 134), (14, 6)])
def test_commit_values_cap_leaves_and_paths(be, oracle, log_n, ncols):
    """PolynomialBatch::from_values under the configuration: the cap, eight leaves and their sibling paths are those of the restatement's
    MerkleTree::new_v2 over the oracle's LDE"""
    rng = np.random.default_rng(log_n * 100 + ncols)
    vals = rand_field(rng, (ncols, 1 << log_n))
    b = be.commit(vals)
    ob = oracle.batch(vals)
    leaves = ob.leaves()
    N = 8 << log_n
    assert leaves.shape == (N, ncols)
    tree = K.MerkleTree(leaves, min(be.cap_height, log_n + 3))
    assert np.array_equal(b.cap(), tree.cap()) and well_formed(b.cap())
    assert np.array_equal(b.coeffs(), ob.coeffs())
    picks = sorted(set([0, 1, N - 1, N // 2, N // 2 - 1] + [int(x) for x in rng.integers(0, N, 3)]))
    for j in picks:
        row, sib = b.leaf(j)
        assert np.array_equal(row, leaves[j])
        assert well_formed(sib) and np.array_equal(np.asarray(sib).reshape(-1, 4), tree.prove(j)), j
        assert K.verify_to_cap(row.tolist(), j, np.asarray(sib).reshape(-1, 4), tree.cap())
    b.free()


# ---------------------------------------------------------------------------------------------------------------- the opening proof
def ext_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=2 * k, offset=at + 4).reshape(k, 2), at + 4 + 16 * k


def field_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=k, offset=at + 4), at + 4 + 8 * k


def path_at(buf, at):
    """a MerkleProof of 25-byte siblings -> (list of 25-byte digests, offset of the first sibling, next offset)"""
    depth = buf[at]
    return [bytes(buf[at + 1 + DB * i:at + 1 + DB * (i + 1)]) for i in range(depth)], at + 1, at + 1 + DB * depth


def parse_queries(buf):
    """the query rounds of a FriProof (serialization.rs:255-303) with 25-byte digests"""
    (nq,) = struct.unpack_from("<I", buf, 0)
    at, out = 4, []
    for _ in range(nq):
        (ni,) = struct.unpack_from("<I", buf, at)
        at += 4
        initial, steps = [], []
        for _ in range(ni):
            row, at = field_vec(buf, at)
            sib, sib_at, at = path_at(buf, at)
            initial.append((row, sib, sib_at))
        (ns,) = struct.unpack_from("<I", buf, at)
        at += 4
        for _ in range(ns):
            ev, at = ext_vec(buf, at)
            sib, sib_at, at = path_at(buf, at)
            steps.append((ev, sib, sib_at))
        out.append((initial, steps))
    assert at == len(buf)
    return out


def layer_trees(oracle, layers, cap_height=4):
    """the restatement's trees over the layers that fri_committed_trees commits: the polynomial's values on shift * H in bit-reversed
    order, 16 extension elements to a leaf (the leaf building of opening_reference.layer_caps; the transform is the oracle's)"""
    trees, shift = [], 7
    for c, length in layers[:-1]:
        planes = np.zeros((2, length), dtype=np.uint64)
        planes[:, :len(c)] = np.array(c, dtype=np.uint64).T
        va, vb = (oracle.evaluate_poly_with_offset(pl, shift, 1) for pl in planes)
        bits = length.bit_length() - 1
        j = np.arange(length, dtype=np.uint64)
        rev = np.zeros(length, dtype=np.uint64)
        for b in range(bits):
            rev |= ((j >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
        leaves = np.stack([va[rev], vb[rev]], axis=1).reshape(length // 16, 32)
        trees.append((leaves, K.MerkleTree(leaves, cap_height)))
        shift = pow(shift, 16, P)
    return trees


def cap_bytes(cap):
    return b"".join(K.digest_bytes(d) for d in np.asarray(cap, dtype=np.uint64).reshape(-1, 4))


@pytest.mark.parametrize("log_n,cols,nperm", [(3, (3, 2, 2), 0), (7, (5, 4, 4), 1), (10, (4, 3, 2), 0), (11, (3, 2, 2), 1), (12, (9, 5, 4), 2)])
def test_opening_proof_step_by_step_with_the_python_challenger(be, oracle, log_n, cols, nperm):
    """ola_open, ola_fri_commit_begin / next_layer / finish, ola_pow, ola_fri_query with the transcript held by the PYTHON Keccak challenger
    (the onion permutation, digests observed as 4 elements): layer caps, query leaves and 25-byte sibling paths against the restatement's
    trees over opening_reference's folded polynomials; the pieces are ola_open_and_prove's bytes; ola_verify_opening accepts them and
    refuses a flipped sibling byte, a flipped cap byte and a witness one too small.  No layer (2^3), one (2^7), two (2^10: direct
    layer-leaf kernel; 2^11 and 2^12: staged)."""
    from olavm_amd.backend import Challenger, OlaGpuError
    rng = np.random.default_rng(7000 + log_n)
    n = 1 << log_n
    N = n << 3
    tv, zv, qc = rand_field(rng, (cols[0], n)), rand_field(rng, (cols[1], n)), rand_field(rng, (cols[2], n))
    gt, gz, gq = be.commit(tv), be.commit(zv), be.commit(qc, from_coeffs=True)
    obs = [oracle.batch(tv), oracle.batch(zv), oracle.batch(qc, from_coeffs=True)]
    initial = [(ob.leaves(), K.MerkleTree(ob.leaves(), min(4, log_n + 3))) for ob in obs]
    ch, mine = Challenger(hasher="keccak"), K.Challenger()
    for b, (_, tree) in zip((gt, gz, gq), initial):
        assert np.array_equal(b.cap(), tree.cap())
        ch.observe_cap(b.cap())
        mine.observe_cap(b.cap())
    before = ch.clone()
    want_open, want_fri = be.open_and_prove(gt, gz, gq, nperm, ch)

    zeta = mine.get_n(2)
    got_open, fri = be.open(gt, gz, gq, nperm, zeta)
    assert got_open == want_open
    local, at = ext_vec(got_open, 0)
    nxt, at = ext_vec(got_open, at)
    zs_local, at = ext_vec(got_open, at)
    zs_next, at = ext_vec(got_open, at)
    ctl_last, at = field_vec(got_open, at)
    q_local, at = ext_vec(got_open, at)
    assert at == len(got_open)
    for v in (local, zs_local, q_local, nxt, zs_next):
        mine.observe(v.reshape(-1).tolist())
    mine.observe(np.stack([ctl_last, np.zeros_like(ctl_last)], axis=1).reshape(-1).tolist())
    alpha = mine.get_n(2)
    fri.begin(alpha)
    caps, betas, beta = [], [], None
    for _ in fri.arity_bits:
        cap = fri.next_layer(beta)
        assert well_formed(cap)
        caps.append(cap)
        mine.observe_cap(cap)
        beta = mine.get_n(2)
        betas.append(beta)
    assert len(caps) == {3: 0, 7: 1, 10: 2, 11: 2, 12: 2}[log_n]
    final_poly = fri.finish(beta)
    mine.observe(final_poly.reshape(-1).tolist())
    witness = be.pow(np.array(mine.get_n(4), dtype=np.uint64), bits=16)
    xs = np.array([mine.get() % N for _ in range(28)], dtype=np.uint64)
    queries = fri.query(xs)
    fri.free()

    # ---- against the restatement: the folded polynomials' trees
    coeffs = [[c.tolist() for c in ob.coeffs()] for ob in obs[:2]] + [[c.tolist() for c in qc]]
    layers = R.fri_layers(coeffs[0], coeffs[1], coeffs[2], nperm, zeta, alpha, betas)
    trees = layer_trees(oracle, layers)
    assert len(trees) == len(caps)
    for cap, (_, tree) in zip(caps, trees):
        assert np.array_equal(cap, tree.cap())
    assert [tuple(int(v) for v in e) for e in final_poly] == R.final_poly(coeffs[0], coeffs[1], coeffs[2], nperm, zeta, alpha, betas, layers=layers)
    parsed = parse_queries(queries)
    assert len(parsed) == 28
    for x, (ini, steps) in zip(xs.tolist(), parsed):
        assert len(ini) == 3 and len(steps) == len(trees)
        for (row, sib, _), (leaves, tree) in zip(ini, initial):
            assert np.array_equal(row, leaves[x])
            assert sib == [K.digest_bytes(d) for d in tree.prove(x)]
            assert K.verify_to_cap(row.tolist(), x, sib, tree.cap())
        for (ev, sib, _), (leaves, tree) in zip(steps, trees):
            x >>= 4
            assert np.array_equal(ev.reshape(-1), leaves[x])
            assert sib == [K.digest_bytes(d) for d in tree.prove(x)]
            assert K.verify_to_cap(ev.reshape(-1).tolist(), x, sib, tree.cap())

    # ---- the pieces are the fused call's bytes, and the two transcripts end in the same state
    head = struct.pack("<I", len(caps)) + b"".join(struct.pack("<I", cap.shape[0]) + cap_bytes(cap) for cap in caps)
    out = head + queries + struct.pack("<I", final_poly.shape[0]) + final_poly.astype("<u8").tobytes() + struct.pack("<Q", int(witness))
    assert out == want_fri
    assert mine.get() == ch.get()

    # ---- the verifier
    all_caps = np.stack([gt.cap(), gz.cap(), gq.cap()])
    proof = want_open + want_fri
    res = be.verify_opening(all_caps, cols, log_n, nperm, proof, before.clone())
    assert res, res

    def refused(bad, caps3=all_caps):
        r = be.verify_opening(caps3, cols, log_n, nperm, bytes(bad), before.clone())
        assert not r, r
        return r

    sib_at = next((s[2] for s in parsed[3][0] if s[1]), None)                  # a sibling of query 3's first initial path that has one
    if sib_at is not None:
        bad = bytearray(proof)
        bad[len(want_open) + len(head) + sib_at + DB - 1] ^= 0x10              # byte 24 of the first sibling
        assert refused(bad).reason == "MERKLE_INITIAL"
    bad = bytearray(proof)
    if caps:
        bad[len(want_open) + 8 + DB - 1] ^= 1                                  # byte 24 of the first digest of the first layer's cap
        refused(bad)
    flipped = all_caps.copy()
    flipped[0, int(xs[0]) >> (log_n + 3 - min(4, log_n + 3)), 3] ^= np.uint64(1)   # byte 24 of the trace cap entry query 0 ends in
    assert refused(proof, flipped).reason == "MERKLE_INITIAL"
    assert witness > 0
    bad = bytearray(proof)
    bad[-8:] = struct.pack("<Q", int(witness) - 1)
    assert refused(bad).reason == "POW"
    overflow = all_caps.copy()
    overflow[1, 0, 3] |= np.uint64(256)                                        # word 3 above one byte: not a digest
    with pytest.raises(OlaGpuError):
        be.verify_opening(overflow, cols, log_n, nperm, proof, before.clone())
    # a Poseidon challenger handed to a Keccak context is refused
    with pytest.raises(OlaGpuError):
        be.open_and_prove(gt, gz, gq, nperm, Challenger())
    for b in (gt, gz, gq):
        b.free()


# ---------------------------------------------------------------------------------------------------------------- whole proofs
@pytest.fixture(scope="module")
def committed():
    return open(PROOF, "rb").read(), json.load(open(RECORD))       # a missing fixture is a failure


@pytest.fixture(scope="module")
def wide():
    from tests.make_ref_verdict import instance
    return T.ola_stark().blob(), instance()


def test_prove_with_traces_gives_the_committed_proof(be, wide, committed):
    blob, (traces, params, compress) = wide
    raw, rec = committed
    assert hashlib.sha256(raw).hexdigest() == rec["proof_sha256"] and rec["verify_proof"] == "Ok(())"
    assert bytes(be.prove_with_traces(blob, traces, params, compress)) == raw
    by_cols = [[np.array(c) for c in t] for t in traces]            # every column its own allocation: ola_prove_with_traces_cols
    assert bytes(be.prove_with_traces(blob, by_cols, params, compress)) == raw


def test_interpreter_kernels_give_the_committed_proof(committed):
    code = r"""
import os, sys
sys.path.insert(0, %r)
os.environ["OLA_AIR_KERNELS"] = "interpreter"
from olavm_amd.air import ola_tables as T
from olavm_amd.backend import Backend
from tests.make_ref_verdict import instance
traces, params, compress = instance()
be = Backend(device=0, hasher="keccak")
raw = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
be.close()
print("same" if raw == open(%r, "rb").read() else "different", len(raw))
""" % (ROOT, PROOF)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "same" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_memory_lean_mode_gives_the_committed_proof(be, wide, committed, monkeypatch):
    blob, (traces, params, compress) = wide
    monkeypatch.setenv("OLA_LEAN", "1")
    assert bytes(be.prove_with_traces(blob, traces, params, compress)) == committed[0]


def test_two_rank_aliased_context_gives_the_committed_proof(wide, committed):
    from olavm_amd.backend import Backend
    blob, (traces, params, compress) = wide
    b = Backend(devices=[0, 0], hasher="keccak")
    try:
        assert bytes(b.prove_with_traces(blob, traces, params, compress)) == committed[0]
    finally:
        b.close()


# where the reference's verifier stops (the record's `reference` field) -> the reason of the report
REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}


def test_verify_all_proof_gives_the_records_verdicts(be, wide, committed):
    """the honest proof and the nineteen one-bit corruptions: the verdict, the table and the place the reference's verifier gave"""
    from tests.test_gpu_verify import span_place
    blob = wide[0]
    raw, rec = committed
    res = be.verify_all_proof(blob, raw)
    assert res and res.reason == "OK" and (res.table, res.query, res.oracle_or_layer) == (None, None, None), res
    layers = [len(s["fri_challenges"]["fri_betas"]) for s in rec["challenges"]["stark_challenges"]]
    assert res.query_jobs == 28 * 12 and res.merkle_jobs == 28 * sum(3 + l for l in layers) and res.kernel_launches == 2
    assert len(rec["tampered"]) == 19
    for t in rec["tampered"]:
        bad = bytearray(raw)
        bad[t["byte"]] ^= 1 << t["bit"]
        res = be.verify_all_proof(blob, bytes(bad))
        table, query, which = span_place(t["span"])
        assert not res and res.reason in REFERENCE[t["reference"]], (t, res)
        assert res.table == table, (t, res)
        if query is not None:
            assert (res.query, res.oracle_or_layer) == (query, which), (t, res)
            assert res.reason == ("FRI_CONSISTENCY" if t["reference"] == "Err verifier.rs:218" else "MERKLE_COMMIT" if ".step[" in t["span"] else "MERKLE_INITIAL")
        else:
            assert (res.query, res.oracle_or_layer) == (None, None), (t, res)


def test_executed_programs_and_the_padding_instance_are_proven_and_accepted(be):
    blob = T.ola_stark(**MINI).blob()
    instances = {name: M.instance(make(), **MINI, **kw) for name, (make, kw) in M.EXAMPLES.items()}
    instances["padding"] = tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(3))
    assert len(instances) == 10
    for name, (traces, params, compress) in instances.items():
        proof = bytes(be.prove_with_traces(blob, traces, params, compress))
        res = be.verify_all_proof(blob, proof, params)
        assert res and res.kernel_launches == 2, (name, res)
        assert be.verify_all_proof(blob, proof), name
        bad = bytearray(proof)
        bad[len(bad) // 2] ^= 4
        assert not be.verify_all_proof(blob, bytes(bad), params), name


def test_configurations_refuse_each_others_proofs(be, wide, committed):
    from olavm_amd.backend import Backend
    blob = wide[0]
    raw = committed[0]
    for other, stem in (("blake3", "wide_program_blake3"), ("poseidon", "wide_program")):
        theirs = open(os.path.join(DIR, stem + ".proof"), "rb").read()
        b = Backend(device=0, hasher=other)
        try:
            assert b.verify_all_proof(blob, theirs)
            assert not b.verify_all_proof(blob, raw), other
        finally:
            b.close()
        assert not be.verify_all_proof(blob, theirs), other
