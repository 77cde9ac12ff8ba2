"""GPU parity under the reference fork's Poseidon2GoldilocksConfig (OLA_HASH_POSEIDON2: Merkle trees, challenger and proof of work on
Poseidon2, hash/poseidon2.rs:50) and Poseidon2GoldilocksConfig2 (OLA_HASH_POSEIDON2_POW_POSEIDON: the proof of work on Poseidon,
plonk/config.rs:133-141).  The checker is the Python restatement of tools/poseidon2_ref.py, pinned to the interpreted reference by
tests/test_poseidon2.py; the whole proof is pinned by tests/golden/ref_verified/wide_program_poseidon2.proof."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import poseidon2_ref as Q  # noqa: E402

pytestmark = pytest.mark.gpu
P = Q.P
PARAMS = Q.params_from_header()
PROOF = os.path.join(HERE, "golden", "ref_verified", "wide_program_poseidon2.proof")


def perm_many(states):
    """the restatement on an (n, 12) array of u64 states at once (numpy object arrays of Python integers)"""
    a = np.asarray(states, dtype=np.uint64).astype(object) % P
    out = Q.permute_lanes([a[:, i] for i in range(12)], PARAMS)
    return np.stack([np.asarray(o, dtype=object) for o in out], axis=1).astype(np.uint64)


def hash_no_pad(rows):
    """hash_n_to_hash_no_pad (hashing.rs:84-107) of every row: overwrite-mode sponge, rate 8, 4-element digest"""
    rows = np.asarray(rows, dtype=np.uint64)
    n, w = rows.shape
    st = np.zeros((n, 12), dtype=np.uint64)
    for c0 in range(0, w, 8):
        blk = rows[:, c0:c0 + 8]
        st[:, :blk.shape[1]] = blk
        st = perm_many(st)
    return st[:, :4]


def merkle_cap(leaves, cap_height):
    """MerkleTree::new_v2 (merkle_tree/mod.rs:180-226): every leaf hashed, compress (hashing.rs:66-74) up to 2^cap_height nodes"""
    level = hash_no_pad(leaves)
    while level.shape[0] > (1 << cap_height):
        st = np.zeros((level.shape[0] // 2, 12), dtype=np.uint64)
        st[:, :4], st[:, 4:8] = level[0::2], level[1::2]
        level = perm_many(st)[:, :4]
    return level


def rand_u64(rng, shape, noncanonical=True):
    x = rng.integers(0, 2**64, shape, dtype=np.uint64)
    if noncanonical:
        flat = x.reshape(-1)
        flat[::97] = np.uint64(P) + (flat[::97] % np.uint64(2**32 - 1))     # words >= p
    return x


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0, hasher="poseidon2")
    yield b
    b.close()


def test_permutation_equals_the_known_answers_and_the_restatement(be):
    import json
    kats = json.load(open(os.path.join(HERE, "golden", "ref_poseidon2_vectors.json")))["vectors"]
    got = be.poseidon2(np.array([v["input"] for v in kats], dtype=np.uint64))
    assert got.tolist() == [v["output"] for v in kats]
    rng = np.random.default_rng(22)
    for n in (1, 5, 8192, 8193, 1 << 16):           # quad-cooperative form up to 8192 states, one state per thread above
        s = rand_u64(rng, (n, 12))
        s[0] = np.uint64(2**64 - 1)
        assert np.array_equal(be.poseidon2(s), perm_many(s)), n
    # the Poseidon permutation entry is unchanged under this context
    z = np.zeros((1, 12), dtype=np.uint64)
    assert hex(int(be.poseidon(z)[0, 0])) == "0x3c18a9786cb0b359"


@pytest.mark.parametrize("row_len", [1, 4, 8, 9, 16, 94, 135])
def test_hash_rows(be, row_len):
    rng = np.random.default_rng(row_len)
    for nrows in (300, 9000):                       # both sides of the launchers' 8192 switch
        rows = rand_u64(rng, (nrows, row_len))
        got = be.hash_rows(rows)
        idx = sorted(set(list(range(0, nrows, 37)) + [nrows - 1]))
        assert np.array_equal(got[idx], hash_no_pad(rows[idx])), nrows


@pytest.mark.parametrize("log_leaves,width,cap_h", [(4, 5, 4), (5, 3, 2), (9, 12, 4), (8, 33, 0), (13, 7, 4), (14, 2, 3), (10, 135, 3)])
def test_merkle_cap(be, log_leaves, width, cap_h):
    rng = np.random.default_rng(log_leaves * 7 + width)
    leaves = rand_u64(rng, (1 << log_leaves, width))
    assert np.array_equal(be.merkle_cap(leaves, cap_h), merkle_cap(leaves, cap_h))


@pytest.mark.parametrize("log_n,ncols", [(3, 2), (8, 12), (11, 9)])
def test_commit_values_cap_is_the_tree_over_the_lde(be, log_n, ncols):
    from olavm_amd.backend import OLA_NTT_COSET_LDE_LEAF_ORDER, OLA_NTT_INTERPOLATE
    rng = np.random.default_rng(100 + log_n)
    vals = rng.integers(0, P, (ncols, 1 << log_n), dtype=np.uint64)
    coeffs = be.ntt(OLA_NTT_INTERPOLATE, vals)
    lde = be.ntt(OLA_NTT_COSET_LDE_LEAF_ORDER, coeffs, shift=7, blowup_log=be.rate_bits)
    b = be.commit(vals)
    assert np.array_equal(b.cap(), merkle_cap(np.ascontiguousarray(lde.T), be.cap_height))
    b.free()


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_pow_is_the_minimal_witness_of_the_inner_hasher(be, bits):
    """ola_pow searches with C::InnerHasher: Poseidon2 under hasher 2 (fri/prover.rs:133), Poseidon under hasher 3"""
    from olavm_amd.backend import Backend
    rng = np.random.default_rng(bits)
    h = rng.integers(0, P, 4, dtype=np.uint64)
    # Poseidon2: a vectorised scan for the first nonce below 2^bits leading zeros
    want2, start = None, 0
    while want2 is None:
        st = np.zeros((4096, 12), dtype=np.uint64)
        st[:, :4] = h
        st[:, 4] = np.arange(start, start + 4096, dtype=np.uint64)
        hit = np.nonzero((perm_many(st)[:, 0] >> np.uint64(64 - bits)) == 0)[0]
        want2 = start + int(hit[0]) if hit.size else None
        start += 4096
    assert be.pow(h, bits) == want2
    b3 = Backend(device=0, hasher="poseidon2_pow_poseidon")
    try:
        w = b3.pow(h, bits)
        st = np.zeros((w + 1, 12), dtype=np.uint64)
        st[:, :4] = h
        st[:, 4] = np.arange(w + 1, dtype=np.uint64)
        out = b3.poseidon(st)[:, 0] >> np.uint64(64 - bits)     # Poseidon (its own entry, pinned by its KATs)
        assert out[w] == 0 and not np.any(out[:w] == 0)
    finally:
        b3.close()


def _prove(hasher, devices=None):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    traces, params, compress = instance()
    b = Backend(device=0, hasher=hasher) if devices is None else Backend(devices=devices, hasher=hasher)
    try:
        return bytes(b.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
    finally:
        b.close()


@pytest.fixture(scope="module")
def proof2():
    return _prove("poseidon2")


def test_proof_under_poseidon2_is_the_committed_proof(proof2):
    assert proof2 == open(PROOF, "rb").read()


def test_config2_proof_differs_only_in_the_proof_of_work_witnesses(proof2):
    sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
    import compare_with_dump as m
    proof3 = _prove("poseidon2_pow_poseidon")
    assert len(proof3) == len(proof2) and proof3 != proof2
    spans = m.parse_all_proof(proof2)
    pows = [(a, b) for n, a, b in spans if n.endswith("pow_witness")]
    assert len(pows) == 12
    diff = [i for i in range(len(proof2)) if proof2[i] != proof3[i]]
    assert all(any(a <= i < b for a, b in pows) for i in diff)
    assert m.first_difference(proof3, proof2) is None
    # the bytes the reference's verifier accepted under Poseidon2GoldilocksConfig2 (tests/make_ref_verdict_poseidon2.py), and each of the
    # twelve witnesses -- found by the side-stream search inside the proof -- is the minimal Poseidon nonce of its recorded input
    import hashlib
    import json
    c2 = json.load(open(PROOF[:-len(".proof")] + ".json"))["config2"]
    assert hashlib.sha256(proof3).hexdigest() == c2["proof_sha256"] and len(proof3) == c2["proof_bytes"]
    ws = [int.from_bytes(proof3[a:b], "little") for a, b in pows]
    assert ws == c2["pow_witnesses"]
    from olavm_amd.backend import Backend
    be = Backend(device=0, hasher="poseidon2_pow_poseidon")
    try:
        for h, w in zip(c2["pow_inputs"], ws):
            st = np.zeros((w + 1, 12), dtype=np.uint64)
            st[:, :4] = np.array(h, dtype=np.uint64)
            st[:, 4] = np.arange(w + 1, dtype=np.uint64)
            lead = be.poseidon(st)[:, 0] >> np.uint64(64 - 16)
            assert lead[w] == 0 and not np.any(lead[:w] == 0)
    finally:
        be.close()


@pytest.mark.parametrize("hasher", ["poseidon2", "poseidon2_pow_poseidon"])
@pytest.mark.parametrize("log_n,cols,nperm", [(3, (3, 2, 2), 0), (12, (9, 5, 4), 2), (16, (7, 4, 2), 0)])
def test_layer_stepped_abi_reassembles_the_fused_proof(hasher, log_n, cols, nperm):
    """ola_open, ola_fri_plan / commit_begin / next_layer / finish, ola_pow, ola_fri_query with the caller's transcript under both Poseidon2
    configurations: the same steps and checks as tests/test_gpu_fri_steps.py does under Poseidon and Blake3"""
    from tests import test_gpu_fri_steps as steps
    steps.test_steps_with_the_callers_transcript_reassemble_the_fused_proof(hasher, log_n, cols, nperm)


def test_multi_device_context_gives_the_same_bytes(proof2):
    assert _prove("poseidon2", devices=[0, 0]) == proof2


def test_primed_context_taken_over_by_a_poseidon2_init_gives_the_bytes_of_a_fresh_one():
    code = r"""
import sys
sys.path.insert(0, %r)
from olavm_amd import backend as B
from olavm_amd.air import miniexec as M, ola_tables as T
blob = T.ola_stark(range_bits=4, limb_bits=2).blob()
B.warmup(0, airset=blob)
B.warmup_wait()
traces, params, compress = M.instance(M.fibonacci(12))
out = []
for k in range(2):
    be = B.Backend(device=0, hasher="poseidon2")   # the first one takes the primed context over, the second is created afresh
    out.append(be.prove_with_traces(blob, traces, params, compress))
    be.close()
assert out[0] == out[1]
print("same", len(out[0]))
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "same" in r.stdout, r.stderr[-2000:]


def test_hasher_4_is_refused():
    import ctypes as C
    from olavm_amd.backend import OlaGpuConfig, load_library
    L = load_library()
    cfg = OlaGpuConfig(0, None, 3, 4, 16, 4, 5, 28, 2, 4)
    ctx = C.c_void_p()
    assert L.ola_gpu_init(C.byref(cfg), C.byref(ctx)) == -1
