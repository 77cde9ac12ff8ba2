"""Commit, open, prove and verify under StarkConfig values other than standard_fast_config (rate_bits 1..8, cap_height 0..16,
proof_of_work_bits 1..20, fri_arity_bits 1..8, fri_final_poly_bits 0..5, num_query_rounds 1..1024; tests/config_cases.py).  Everything is
exact equality of words or bytes against the CPU oracle run under the same six integers (tests/oracle_lib.py `cfg`), under Poseidon and
Blake3; one full-size proof is held to what the REFERENCE's interpreted verifier recorded (tests/make_ref_verdict_config.py).

  1. commitments: caps, leaves and sibling paths at the first and last index of every coset, depth 0, caps above and below the 256 nodes
     of the tree's last launch; also with OLA_LEAN=1 in the environment; a cap higher than the tree is refused;
  2. opening proofs byte for byte, the transcript afterwards, both verifiers' verdicts on the proof and on one-bit corruptions of every
     part, and the default configuration's refusal; arities 32 .. 256 are prover-only (the verifier supports FRI arities of 2 to 16);
  3. the stepped ABI with the caller's transcript; ola_fri_query refuses n = 0;
  4. whole proofs of the miniature 12-table set (quotients on fewer cosets than the LDE has) and of a two-table set, refusals of rates
     below the constraint degree, corruptions, cross-configuration refusals, Poseidon2 / Keccak self-consistency, two logical ranks;
  5. the proof-of-work search at 1, 8, 12 and 20 bits, and a witness found by its second launch;
  6. the committed proof under rate_bits 4, cap_height 2, 12-bit work and 20 queries, and its nineteen corruptions."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest

from olavm_amd.air import AirSet, miniexec as M, ola_tables as T
from tests import config_cases as CC, fri_plan_reference as FP, tracegen
from tests.oracle_lib import P, rand_field
from tests.verdicts import WORDS, agrees, oracle_says

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "ref_verified")
OLA_E_INVALID_ARG = -1
MINI = dict(range_bits=4, limb_bits=2)
HASHERS = ["poseidon", "blake3"]
ORACLE_REASONS = {r for _, r in WORDS}
REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.fixture(scope="module")
def backends():
    """one context per (hasher, configuration), kept for the module"""
    from olavm_amd.backend import Backend
    made = {}

    def get(hasher, cfg=CC.DEFAULT):
        if (hasher, cfg) not in made:
            made[(hasher, cfg)] = Backend(device=0, hasher=hasher, **CC.kwargs(cfg))
        return made[(hasher, cfg)]
    yield get
    for be in made.values():
        be.close()


@pytest.fixture(scope="module")
def mini():
    stark = T.ola_stark(**MINI)
    assert [t.constraint_degree for t in stark.tables] == CC.MINI_DEGREES
    traces, params, compress = M.instance(M.fibonacci(5), **MINI)
    assert {t.shape[1] for t in traces} >= {2, 64} and max(t.shape[1] for t in traces) == 64
    return stark.blob(), (traces, params, compress)


@pytest.fixture(scope="module")
def two_tables():
    cmp_t, rc_t = tracegen.cmp_rangecheck_instance(np.random.default_rng(11), 6, 4)
    set_ = AirSet([T.cmp_table(), T.rangecheck_table(4)], [T.ctl_cmp_rangecheck(0, 1)])
    assert [t.constraint_degree for t in set_.tables] == [3, 3]
    return set_.blob(), [cmp_t, rc_t]


# ---------------------------------------------------------------------------------------------------------------- 1. commitments
@pytest.mark.parametrize("lean", ["0", "1"], ids=["resident", "OLA_LEAN"])
@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("rc,log_n", CC.COMMIT, ids=["r%d-c%d" % rc for rc, _ in CC.COMMIT])
def test_commitments_caps_leaves_and_paths(backends, oracle, monkeypatch, hasher, rc, log_n, lean):
    """PolynomialBatch::from_values / from_coeffs under (rate_bits, cap_height): the cap, and the row and sibling path at index 0, N - 1
    and the first and last index of every coset (in leaf order coset k is the leaves [k n, (k + 1) n)); ola_batch_get_lde_row reads the
    same rows in natural order"""
    monkeypatch.setenv("OLA_LEAN", lean)
    rate_bits, cap_height = rc
    n, N = 1 << log_n, 1 << (log_n + rate_bits)
    assert N <= 1 << 16 and log_n + rate_bits >= cap_height
    if rc in ((8, 13), (3, 16)):
        assert log_n + rate_bits == cap_height                                       # depth 0: the leaves' digests are the cap
    be = backends(hasher, (rate_bits, cap_height) + CC.DEFAULT[2:])
    cols = rand_field(np.random.default_rng(100 * rate_bits + cap_height), (CC.COMMIT_COLS, n))
    index = sorted({0, N - 1} | {k * n for k in range(1 << rate_bits)} | {k * n + n - 1 for k in range(1 << rate_bits)})
    with oracle.hasher(hasher):
        for from_coeffs in (False, True):
            b, ob = be.commit(cols, from_coeffs=from_coeffs), oracle.batch(cols, rate_bits, cap_height, from_coeffs=from_coeffs)
            assert b.cap().shape == (1 << cap_height, 4) and np.array_equal(b.cap(), ob.cap()), "cap (from_coeffs=%s)" % from_coeffs
            assert (b.ncols, b.log_n, b.rate_bits) == (CC.COMMIT_COLS, log_n, rate_bits)
            for j in index:
                row, sib = b.leaf(j)
                want = ob.leaf(j)
                assert np.array_equal(row, want), ("leaf", j, from_coeffs)
                path = ob.prove(j)
                assert sib.shape == path.shape == (log_n + rate_bits - cap_height, 4) and np.array_equal(sib, path), ("path", j, from_coeffs)
                assert np.array_equal(b.lde_row(bitrev(j, log_n + rate_bits)), want), ("lde row", j, from_coeffs)
            b.free()


@pytest.mark.parametrize("rc,log_n", [((3, 16), 12), ((8, 13), 4), ((1, 4), 2), ((4, 7), 2)])
def test_a_cap_higher_than_the_tree_is_refused(backends, oracle, rc, log_n):
    from olavm_amd.backend import OlaGpuError
    be = backends("poseidon", rc + CC.DEFAULT[2:])
    assert log_n + rc[0] == rc[1] - 1
    cols = rand_field(np.random.default_rng(5), (3, 1 << log_n))
    for from_coeffs in (False, True):
        with pytest.raises(OlaGpuError) as e:
            be.commit(cols, from_coeffs=from_coeffs)
        assert e.value.code == OLA_E_INVALID_ARG
    cols = rand_field(np.random.default_rng(6), (3, 2 << log_n))                      # one bit more: depth 0, and the context works
    b = be.commit(cols)
    assert np.array_equal(b.cap(), oracle.batch(cols, *rc).cap())
    b.free()


# ---------------------------------------------------------------------------------------------------------------- 2. opening proofs
def layer_depths(cfg, log_n, plan):
    """[(arity, sibling path length)] of every FRI layer"""
    out, bits = [], log_n + cfg[0]
    for ab in plan:
        bits -= ab
        out.append((1 << ab, max(bits - cfg[1], 0)))
    return out


class Opening:
    """three committed batches on the device and in the oracle, and the transcript with their caps observed"""

    def __init__(self, be, oracle, hasher, cfg, log_n, seed):
        from olavm_amd.backend import Challenger
        rng = np.random.default_rng(seed)
        n = 1 << log_n
        self.cols, self.nperm, self.log_n, self.cfg, self.hasher, self.oracle = CC.OPENING_COLS, CC.OPENING_NPERM, log_n, cfg, hasher, oracle
        data = [rand_field(rng, (c, n)) for c in self.cols]
        self.gpu = [be.commit(d, from_coeffs=(i == 2)) for i, d in enumerate(data)]
        self.ora = [oracle.batch(d, cfg[0], cfg[1], from_coeffs=(i == 2)) for i, d in enumerate(data)]
        for g, o in zip(self.gpu, self.ora):
            assert np.array_equal(g.cap(), o.cap())
        self.caps = np.stack([b.cap() for b in self.gpu])
        self.start = Challenger(hasher=hasher)
        for b in self.gpu:
            self.start.observe_cap(b.cap())

    def oracle_challenger(self):
        och = self.oracle.challenger()
        for b in self.ora:
            och.observe_cap(b.cap())
        return och

    def default_caps(self):
        """the caps as a default-configuration verifier takes them, 3 x 16 digests: cut or filled with zeros (it refuses the proof either way)"""
        out = np.zeros((3, 16, 4), dtype=np.uint64)
        k = min(16, self.caps.shape[1])
        out[:, :k] = self.caps[:, :k]
        return out

    def free(self):
        for b in self.gpu:
            b.free()


@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("cfg,log_n,plan,verifies", CC.OPENING, ids=[CC.cfg_id(c[0]) for c in CC.OPENING])
def test_opening_proofs_equal_the_oracles_bytes_and_verdicts(backends, oracle, hasher, cfg, log_n, plan, verifies):
    from olavm_amd.backend import OlaGpuError
    assert (1 << (log_n + cfg[0])) <= 1 << 16
    be = backends(hasher, cfg)
    with oracle.hasher(hasher):
        assert oracle.fri_arity_bits(log_n, cfg) == plan == FP.arity_bits(("constant_arity_bits",), log_n, **CC.kwargs(cfg))
        op = Opening(be, oracle, hasher, cfg, log_n, 31000 + log_n)
        prover, och = op.start.clone(), op.oracle_challenger()
        g_open, g_fri = be.open_and_prove(*op.gpu, op.nperm, prover)
        _, o_open, o_fri = oracle.open_and_prove(*op.ora, op.nperm, och, cfg)
        assert g_open == o_open, "opening set bytes differ"
        if g_fri != o_fri:
            first = next(i for i, (a, b) in enumerate(zip(g_fri, o_fri)) if a != b) if len(g_fri) == len(o_fri) else -1
            spans = CC.opening_spans(o_fri, op.cols, log_n + cfg[0] - cfg[1], layer_depths(cfg, log_n, plan))
            raise AssertionError("FRI proof bytes differ: lengths %d / %d, first at %d; parts of the oracle's bytes: %s" % (len(g_fri), len(o_fri), first, spans))
        after = bytes(C.string_at(C.byref(prover.c), C.sizeof(prover.c)))
        assert [prover.get() for _ in range(3)] == [och.get() for _ in range(3)]         # the two transcripts end in the same state
        honest = g_open + g_fri
        assert oracle.verify_opening(op.caps, op.cols, log_n, op.nperm, honest, op.oracle_challenger(), cfg) == (0, "")

        if not verifies:
            # arities 32 .. 256: the prover's bytes are the oracle's and the oracle accepts them; the library's verifier says what it supports
            assert cfg[3] > 4
            with pytest.raises(OlaGpuError) as e:
                be.verify_opening(op.caps, op.cols, log_n, op.nperm, honest, op.start.clone())
            assert e.value.code == OLA_E_INVALID_ARG and "the verifier supports FRI arities of 2 to 16" in str(e.value)
            again = op.start.clone()
            assert b"".join(be.open_and_prove(*op.gpu, op.nperm, again)) == honest       # the context still proves,
            be.set_fri_reduction(("min_size", None))                                     # and, under a plan the verifier takes, verifies
            try:
                ch = op.start.clone()
                proof = b"".join(be.open_and_prove(*op.gpu, op.nperm, ch))
                assert be.verify_opening(op.caps, op.cols, log_n, op.nperm, proof, op.start.clone())
            finally:
                be.set_fri_reduction(None)
        else:
            ch = op.start.clone()
            res = be.verify_opening(op.caps, op.cols, log_n, op.nperm, honest, ch)
            assert res and res.reason == "OK" and res.query_jobs == cfg[5] and res.merkle_jobs == cfg[5] * (3 + len(plan)), res
            assert bytes(C.string_at(C.byref(ch.c), C.sizeof(ch.c))) == after                # advanced to where the prover's stands
            # one flipped bit in every part the proof has: the oracle's verdict
            spans = CC.opening_spans(g_fri, op.cols, log_n + cfg[0] - cfg[1], layer_depths(cfg, log_n, plan))
            base = len(g_open)
            flips = [("row", 0), ("initial_path", 3), ("layer_leaf", 0), ("layer_leaf", 16), ("layer_path", 5), ("final_poly", (spans["final_poly"][1] // 32) * 16), ("witness", 0)]
            verdicts = {}
            for name, at in flips:
                off, length = spans.get(name, (0, 0))
                if length == 0:
                    continue                                                             # a part this case does not have
                assert at < length
                bad = bytearray(honest)
                bad[base + off + at] ^= 1
                res = be.verify_opening(op.caps, op.cols, log_n, op.nperm, bytes(bad), op.start.clone())
                agrees(res, *oracle.verify_opening(op.caps, op.cols, log_n, op.nperm, bytes(bad), op.oracle_challenger(), cfg))
                verdicts.setdefault(name, []).append(res.reason)
            assert verdicts["row"] == ["MERKLE_INITIAL"] and "final_poly" in verdicts and "witness" in verdicts, verdicts
            if spans["initial_path"][1]:
                assert verdicts["initial_path"] == ["MERKLE_INITIAL"]
            if plan:
                # evaluations 0 and 1 of the first layer's leaf: at most one of them is the one the fold is compared with; the other
                # changes nothing but the leaf's digest
                assert "MERKLE_COMMIT" in verdicts["layer_leaf"] and set(verdicts["layer_leaf"]) <= {"MERKLE_COMMIT", "FRI_CONSISTENCY"}, verdicts
            if spans.get("layer_path", (0, 0))[1]:
                assert verdicts["layer_path"] == ["MERKLE_COMMIT"]

        # the default configuration does not take the proof: a reason of the oracle's list from the library, a refusal from the oracle
        if cfg != CC.DEFAULT:
            res = backends(hasher).verify_opening(op.default_caps(), op.cols, log_n, op.nperm, honest, op.start.clone())
            assert not res and res.reason in ORACLE_REASONS, res
            rc, msg = oracle.verify_opening(op.default_caps(), op.cols, log_n, op.nperm, honest, op.oracle_challenger())
            assert rc != 0 and oracle_says(rc, msg)[1] in ORACLE_REASONS
            agrees(res, rc, msg)
        op.free()


# ---------------------------------------------------------------------------------------------------------------- 3. the stepped ABI
def ext_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=2 * k, offset=at + 4).reshape(k, 2), at + 4 + 16 * k


def field_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=k, offset=at + 4), at + 4 + 8 * k


@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("cfg,log_n", CC.STEPPED, ids=[CC.cfg_id(c) for c, _ in CC.STEPPED])
def test_steps_with_the_callers_transcript_reassemble_the_fused_proof(backends, oracle, hasher, cfg, log_n):
    """as tests/test_gpu_fri_steps.py for the default: N from the context's rate_bits, the query count and the work from the configuration;
    ola_fri_query with no index is refused before anything is launched, and the handle goes on answering"""
    from olavm_amd.backend import OlaGpuError
    be = backends(hasher, cfg)
    with oracle.hasher(hasher):
        op = Opening(be, oracle, hasher, cfg, log_n, 32000 + log_n)
    ch, mine = op.start.clone(), op.start.clone()
    want_open, want_fri = be.open_and_prove(*op.gpu, op.nperm, ch)
    zeta = mine.get(2)
    got_open, fri = be.open(*op.gpu, op.nperm, zeta)
    assert got_open == want_open and fri.arity_bits == FP.arity_bits(("constant_arity_bits",), log_n, **CC.kwargs(cfg))
    local, at = ext_vec(got_open, 0)
    nxt, at = ext_vec(got_open, at)
    zs_local, at = ext_vec(got_open, at)
    zs_next, at = ext_vec(got_open, at)
    ctl_last, at = field_vec(got_open, at)
    q_local, at = ext_vec(got_open, at)
    assert at == len(got_open)
    for v in (local, zs_local, q_local, nxt, zs_next):
        mine.observe(v)
    mine.observe(np.stack([ctl_last, np.zeros_like(ctl_last)], axis=1))
    fri.begin(mine.get(2))
    caps, beta = [], None
    for _ in fri.arity_bits:
        cap = fri.next_layer(beta)
        assert cap.shape == (1 << cfg[1], 4)
        caps.append(cap)
        mine.observe_cap(cap)
        beta = mine.get(2)
    final_poly = fri.finish(beta)
    assert final_poly.shape == (fri.final_poly_len, 2) == (1 << (log_n - sum(fri.arity_bits)), 2)
    mine.observe(final_poly)
    witness = be.pow(mine.get(4), bits=cfg[2])
    N, nq = (1 << log_n) << be.rate_bits, cfg[5]
    assert be.rate_bits == cfg[0]
    xs = np.array([int(mine.get()) % N for _ in range(nq)], dtype=np.uint64)
    with pytest.raises(OlaGpuError) as e:
        fri.query(np.zeros(0, dtype=np.uint64))                                          # n = 0
    assert e.value.code == OLA_E_INVALID_ARG
    queries = fri.query(xs)
    assert (len(queries) - 4) % nq == 0
    one = fri.query(xs[:1])                                                              # the handle still answers: query 0 by itself
    assert one == struct.pack("<I", 1) + queries[4:4 + (len(queries) - 4) // nq]
    fri.free()
    out = struct.pack("<I", len(caps))
    for cap in caps:
        out += struct.pack("<I", cap.shape[0]) + cap.astype("<u8").tobytes()
    out += queries + struct.pack("<I", final_poly.shape[0]) + final_poly.astype("<u8").tobytes() + struct.pack("<Q", int(witness))
    assert out == want_fri
    assert mine.get() == ch.get()
    op.free()


# ---------------------------------------------------------------------------------------------------------------- 4. whole proofs
def middle_flip(proof):
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 4
    return bytes(bad)


@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("cfg", CC.MINI_PROVEN, ids=[CC.cfg_id(c) for c in CC.MINI_PROVEN])
def test_miniature_set_whole_proofs_equal_the_oracles(backends, oracle, mini, monkeypatch, hasher, cfg):
    """twelve tables of constraint degrees 1 .. 8 under rates 16, 32 and 256: the quotient lives on fewer cosets than the LDE has"""
    blob, (traces, params, compress) = mini
    be = backends(hasher, cfg)
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    with oracle.hasher(hasher):
        assert proof == oracle.prove_with_traces(blob, traces, params, compress, cfg=cfg), "AllProof bytes differ from the oracle's"
        res = be.verify_all_proof(blob, proof, params)
        assert res and res.query_jobs == 12 * cfg[5] and res.kernel_launches == 2, res
        agrees(res, *oracle.verify_all_proof(blob, proof, params, cfg=cfg))
        assert be.verify_all_proof(blob, proof)
        bad = middle_flip(proof)
        res = be.verify_all_proof(blob, bad, params)
        assert not res
        agrees(res, *oracle.verify_all_proof(blob, bad, params, cfg=cfg))
        # the default configuration's verifiers refuse it
        res = backends(hasher).verify_all_proof(blob, proof, params)
        assert not res and res.reason in ORACLE_REASONS, res
        agrees(res, *oracle.verify_all_proof(blob, proof, params))
        if cfg[1] != CC.DEFAULT[1]:
            assert (res.reason, res.table) == ("SHAPE_CAP_HEIGHT", 0), res                # verifier.rs:363: the caps' height comes first
    monkeypatch.setenv("OLA_LEAN", "1")                                                  # coset-streamed LDEs: the same bytes
    assert bytes(be.prove_with_traces(blob, traces, params, compress)) == proof


@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("cfg", CC.MINI_REFUSED, ids=[CC.cfg_id(c) for c in CC.MINI_REFUSED])
def test_a_rate_below_the_constraint_degree_is_refused_by_both(backends, oracle, mini, two_tables, hasher, cfg):
    from olavm_amd.backend import OlaGpuError
    blob, (traces, params, compress) = mini
    be = backends(hasher, cfg)
    with oracle.hasher(hasher):
        with pytest.raises(RuntimeError) as oe:
            oracle.prove_with_traces(blob, traces, params, compress, cfg=cfg)
        assert CC.DEGREE_WORDS in str(oe.value)
        with pytest.raises(OlaGpuError) as e:
            be.prove_with_traces(blob, traces, params, compress)
        assert e.value.code == OLA_E_INVALID_ARG and CC.DEGREE_WORDS in str(e.value)
        # the context goes on working: the two-table set's degrees fit
        two, tr = two_tables
        proof = bytes(be.prove_with_traces(two, tr))
        assert proof == oracle.prove_with_traces(two, tr, cfg=cfg) and be.verify_all_proof(two, proof)


@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("cfg", CC.TWO_TABLES, ids=[CC.cfg_id(c) for c in CC.TWO_TABLES])
def test_two_table_set_whole_proofs_equal_the_oracles(backends, oracle, two_tables, hasher, cfg):
    two, tr = two_tables
    be = backends(hasher, cfg)
    proof = bytes(be.prove_with_traces(two, tr))
    with oracle.hasher(hasher):
        assert proof == oracle.prove_with_traces(two, tr, cfg=cfg), "AllProof bytes differ from the oracle's"
        res = be.verify_all_proof(two, proof)
        assert res and res.query_jobs == 2 * cfg[5] and res.kernel_launches == 2, res
        agrees(res, *oracle.verify_all_proof(two, proof, cfg=cfg))
        bad = middle_flip(proof)
        res = be.verify_all_proof(two, bad)
        assert not res
        agrees(res, *oracle.verify_all_proof(two, bad, cfg=cfg))
        res = backends(hasher).verify_all_proof(two, proof)
        assert not res and res.reason in ORACLE_REASONS, res
        agrees(res, *oracle.verify_all_proof(two, proof))
        assert (res.reason, res.table) == ("SHAPE_CAP_HEIGHT", 0), res                    # verifier.rs:363: the caps' height comes first


@pytest.mark.parametrize("hasher", ["poseidon2", "keccak"])
def test_hashers_without_an_oracle_accept_their_own_proof(backends, mini, hasher):
    """A CONSISTENCY check only: the oracle has neither Poseidon2 nor Keccak, so under rate_bits 4, cap_height 2, 12-bit work and 20
    queries the library's verifier judges the library's proof; what ties these kernels to a reference is the default configuration's
    tests (tests/test_gpu_poseidon2.py, tests/test_gpu_keccak.py) and the Poseidon / Blake3 cases of this module."""
    blob, (traces, params, compress) = mini
    be = backends(hasher, CC.NO_ORACLE)
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    res = be.verify_all_proof(blob, proof, params)
    assert res and res.query_jobs == 12 * CC.NO_ORACLE[5] and res.kernel_launches == 2, res
    assert not be.verify_all_proof(blob, middle_flip(proof), params)
    res = backends(hasher).verify_all_proof(blob, proof, params)
    assert not res and res.reason in ORACLE_REASONS, res


def test_two_logical_ranks_give_the_single_device_bytes(backends, oracle, two_tables):
    """the shard limits world <= 2^rate_bits, 2^cap_height at their edge: two ranks on two cosets and a cap of two digests; and tables
    large enough to go on the partition under cap_height 1"""
    from olavm_amd.backend import Backend, OlaGpuError
    two, tr = two_tables
    cfg = (1, 1) + CC.DEFAULT[2:]
    multi = Backend(devices=[0, 0], **CC.kwargs(cfg))
    try:
        proof = bytes(multi.prove_with_traces(two, tr))
    finally:
        multi.close()
    assert proof == bytes(backends("poseidon", cfg).prove_with_traces(two, tr)) == oracle.prove_with_traces(two, tr, cfg=cfg)
    blob = T.ola_stark(**MINI).blob()
    traces, params, compress = tracegen.empty_program_instance(log_n=12, live=np.random.default_rng(12))
    for rate_bits in (3, 4):
        cfg = (rate_bits, 1) + CC.DEFAULT[2:]
        multi = Backend(devices=[0, 0], **CC.kwargs(cfg))
        try:
            multi.proof_stats(enable=True)
            proof = bytes(multi.prove_with_traces(blob, traces, params, compress))
            st = multi.proof_stats()
        finally:
            multi.close()
        assert st["peer_exchanges"] > 0, st                                              # tables of the instance are on the partition
        one = backends("poseidon", cfg)
        assert proof == bytes(one.prove_with_traces(blob, traces, params, compress)), "rate_bits %d" % rate_bits
        assert one.verify_all_proof(blob, proof, params)
    for kw in (dict(rate_bits=1), dict(cap_height=1)):
        with pytest.raises(OlaGpuError) as e:
            Backend(devices=[0] * 4, **kw)
        assert e.value.code == OLA_E_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------- 5. proof of work
def test_proof_of_work_witnesses_are_the_oracles(backends, oracle):
    """proof_of_work_bits 37..40 are not searched on a device (minutes to hours each); their launch geometry is tests/test_pow_batch.py's"""
    be = backends("poseidon")
    rng = np.random.default_rng(77)
    for bits in CC.POW_BITS:
        for _ in range(3):
            h = rng.integers(0, P, 4, dtype=np.uint64)
            assert be.pow(h, bits) == oracle.fri_pow(h, bits), bits
    seed, draw, bits, witness = CC.POW_SECOND_LAUNCH
    rng = np.random.default_rng(seed)
    for _ in range(draw):
        h = rng.integers(0, P, 4, dtype=np.uint64)
    want = oracle.fri_pow(h, bits)
    assert want == witness and want >= 1 << 14                                         # beyond the first batch of 2^14 nonces
    assert be.pow(h, bits) == want


# ---------------------------------------------------------------------------------------------------------------- 6. held to the reference
def span_place(span):
    m = re.match(r"table (\d+): ", span)
    table = int(m.group(1)) if m else int(re.match(r"compress_challenges\[(\d+)\]", span).group(1))
    q = re.search(r"fri\.query\[(\d+)\]\.(?:initial_trees_proof|step)\[(\d+)\]", span)
    return (table, int(q.group(1)), int(q.group(2))) if q else (table, None, None)


def test_committed_configuration_proof_and_its_nineteen_corruptions(backends):
    """tests/golden/ref_verified/wide_program_cfg.{proof,json}: the full-size instance under rate_bits 4, cap_height 2, 12-bit work and 20
    queries (an LDE of 2^22 points: the one case of this module above 2^16).  ola_prove_with_traces returns the committed bytes, which the
    reference's verifier accepted under that configuration, and the library's verifier gives the reference's verdict and place on each
    of the nineteen corruptions; the default configuration refuses the proof, as the reference's did."""
    from tests.make_ref_verdict import instance
    raw = open(os.path.join(DIR, "wide_program_cfg.proof"), "rb").read()
    rec = json.load(open(os.path.join(DIR, "wide_program_cfg.json")))
    assert tuple(rec["oracle_cfg"]) == CC.REFERENCE_CFG and rec["verify_proof"] == "Ok(())"
    assert rec["verify_proof_under_standard_fast_config"].startswith("Err ")
    blob = T.ola_stark().blob()
    traces, params, compress = instance()
    be = backends("poseidon", CC.REFERENCE_CFG)
    got = bytes(be.prove_with_traces(blob, traces, params, compress))
    assert got == raw, "ola_prove_with_traces under the configuration does not return the committed proof"
    res = be.verify_all_proof(blob, raw)
    assert res and res.reason == "OK" and (res.table, res.query, res.oracle_or_layer) == (None, None, None), res
    nq = CC.REFERENCE_CFG[5]
    assert res.query_jobs == nq * 12 and res.merkle_jobs == nq * sum(3 + l for l in rec["fri_layers"]) and res.kernel_launches == 2
    assert len(rec["tampered"]) == 19
    for t in rec["tampered"]:
        bad = bytearray(raw)
        bad[t["byte"]] ^= 1 << t["bit"]
        res = be.verify_all_proof(blob, bytes(bad))
        table, query, which = span_place(t["span"])
        assert not res and res.reason in REFERENCE[t["reference"]], (t, res)             # where the reference's verifier stopped
        assert res.table == table, (t, res)
        if query is not None:
            assert (res.query, res.oracle_or_layer) == (query, which), (t, res)
            assert res.reason == ("FRI_CONSISTENCY" if t["reference"] == "Err verifier.rs:218" else "MERKLE_COMMIT" if ".step[" in t["span"] else "MERKLE_INITIAL")
        else:
            assert (res.query, res.oracle_or_layer) == (None, None), (t, res)
    # standard_fast_config: the reference stopped at `ensure!(trace_cap.height() == cap_height)` of the first table (verifier.rs:363)
    assert rec["verify_proof_under_standard_fast_config"] == "Err verifier.rs:363"
    res = backends("poseidon").verify_all_proof(blob, raw)
    assert not res and (res.reason, res.table, res.query) == ("SHAPE_CAP_HEIGHT", 0, None), res
