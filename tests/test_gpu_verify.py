"""ola_verify_all_proof / ola_verify_opening on the device (include/ola_gpu.h "verification", PARITY.md): every verdict and reason is
held to the ORACLE's verifier on the same bytes (its message mapped to the OLA_VERIFY_* reason here), and on the committed proofs to
what the REFERENCE's interpreted verifier recorded beside them (tests/golden/ref_verified/*.json) -- never to the product itself.

  1. the three committed proofs are accepted, their 19 one-bit corruptions each rejected with the oracle's / the reference's reason at
     the table, query and oracle-or-layer the record's span names; the other configuration's verifier refuses each proof; a proof made
     under Poseidon2GoldilocksConfig2 is accepted by its own verifier and refused by Poseidon2GoldilocksConfig's;
  2. the nine executed miniature programs and the padding instance, proven by the library, are accepted (2-row tables: Merkle depth 0
     and no FRI layer; tables with and without permutation arguments; quotient oracles of two and four words; the 134-column
     Poseidon table), with the same two kernel launches for a 2-table and a 12-table set;
  3. at the opening level, proofs assembled through the stepped ABI with the transcript kept by the test, whose Merkle paths all
     verify and whose algebra does not: wrong alpha, wrong betas, a changed final polynomial, a proof-of-work witness one too small;
  4. several faults at once: the one the reference reaches first is reported;
  5. refusals -- non-canonical words, trailing bytes, a multi-rank context -- after each of which the context proves and verifies."""
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

from olavm_amd.air import AirSet, miniexec as M, ola_tables as T
from tests import tracegen
from tests.verdicts import WORDS, agrees, oracle_says  # noqa: F401  (the oracle's words -> the report's reasons)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")
sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
P = 0xFFFFFFFF00000001
OLA_E_INVALID_ARG = -1
STEM = {"poseidon": "wide_program", "blake3": "wide_program_blake3", "poseidon2": "wide_program_poseidon2"}
MINI = dict(range_bits=4, limb_bits=2)

# where the reference's verifier stops (the records' `reference` field) -> the reason
REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}


def span_place(span):
    """(table, query, oracle or layer) a record's span names; None where it names none"""
    m = re.match(r"table (\d+): ", span)
    table = int(m.group(1)) if m else int(re.match(r"compress_challenges\[(\d+)\]", span).group(1))
    q = re.search(r"fri\.query\[(\d+)\]\.(?:initial_trees_proof|step)\[(\d+)\]", span)
    return (table, int(q.group(1)), int(q.group(2))) if q else (table, None, None)


@pytest.fixture(scope="module")
def backends():
    from olavm_amd.backend import Backend
    made = {}

    def get(hasher):
        if hasher not in made:
            made[hasher] = Backend(device=0, hasher=hasher)
        return made[hasher]
    yield get
    for be in made.values():
        be.close()


@pytest.fixture(scope="module")
def full_blob():
    return T.ola_stark().blob()


@pytest.fixture(scope="module")
def mini():
    """the miniature 12-table set and one executed instance of it, for "the context still proves and verifies" """
    return T.ola_stark(**MINI).blob(), M.instance(M.fibonacci(5), **MINI)


def still_works(be, mini, oracle=None):
    blob, (traces, params, compress) = mini
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    res = be.verify_all_proof(blob, proof)
    assert res and res.kernel_launches == 2, res
    if oracle is not None:
        assert oracle.verify_all_proof(blob, proof, params) == (0, "")


# ---------------------------------------------------------------------------------------------------------------- 1. the committed proofs
@pytest.mark.parametrize("config", ["poseidon", "blake3", "poseidon2"])
def test_committed_proof_and_its_nineteen_corruptions(backends, full_blob, oracle, config):
    raw = open(os.path.join(DIR, STEM[config] + ".proof"), "rb").read()
    rec = json.load(open(os.path.join(DIR, STEM[config] + ".json")))
    be = backends(config)
    res = be.verify_all_proof(full_blob, raw)                    # params NULL: from the proof's compress challenges
    assert res and res.reason == "OK" and (res.table, res.query, res.oracle_or_layer) == (None, None, None), res
    layers = [len(s["fri_challenges"]["fri_betas"]) for s in rec["challenges"]["stark_challenges"]]
    assert res.query_jobs == 28 * 12 and res.merkle_jobs == 28 * sum(3 + l for l in layers) and res.kernel_launches == 2
    compress = np.frombuffer(raw[-96:], dtype="<u8")
    assert be.verify_all_proof(full_blob, raw, [int(compress[2]), int(compress[10])])             # and with the caller's parameters
    assert not be.verify_all_proof(full_blob, raw, [int(compress[2]) ^ 1, int(compress[10])])
    assert len(rec["tampered"]) == 19
    for t in rec["tampered"]:
        bad = bytearray(raw)
        bad[t["byte"]] ^= 1 << t["bit"]
        bad = bytes(bad)
        res = be.verify_all_proof(full_blob, bad)
        table, query, which = span_place(t["span"])
        assert not res and res.reason in REFERENCE[t["reference"]], (t, res)         # where the reference's verifier stopped
        assert res.table == table, (t, res)
        if query is not None:
            assert (res.query, res.oracle_or_layer) == (query, which), (t, res)
            assert res.reason == ("FRI_CONSISTENCY" if t["reference"] == "Err verifier.rs:218" else "MERKLE_COMMIT" if ".step[" in t["span"] else "MERKLE_INITIAL")
        else:
            assert (res.query, res.oracle_or_layer) == (None, None), (t, res)
        if config != "poseidon2":                                                      # the oracle has no Poseidon2 configuration
            c = np.frombuffer(bad[-96:], dtype="<u8")
            with oracle.hasher(config):
                agrees(res, *oracle.verify_all_proof(full_blob, bad, [int(c[2]), int(c[10])]))
    # the other configurations' verifiers do not take it
    for other in ("poseidon", "blake3", "poseidon2"):
        if other != config:
            res = backends(other).verify_all_proof(full_blob, raw)
            assert not res, (other, res)
            if other != "poseidon2":
                with oracle.hasher(other):
                    assert oracle.verify_all_proof(full_blob, raw, [int(compress[2]), int(compress[10])])[0] != 0


def test_poseidon2_config2_proof_is_its_own(backends, mini):
    """Poseidon2GoldilocksConfig2 (Poseidon2 trees and transcript, Poseidon proof of work): its verifier accepts its proof,
    Poseidon2GoldilocksConfig's reads the same trees and transcript and stops at the proof of work of the first table"""
    blob, (traces, params, compress) = mini
    be3, be2 = backends("poseidon2_pow_poseidon"), backends("poseidon2")
    proof = bytes(be3.prove_with_traces(blob, traces, params, compress))
    assert be3.verify_all_proof(blob, proof, params)
    res = be2.verify_all_proof(blob, proof, params)
    assert not res and (res.reason, res.table) == ("POW", 0), res
    back = bytes(be2.prove_with_traces(blob, traces, params, compress))
    assert be2.verify_all_proof(blob, back) and not be3.verify_all_proof(blob, back)


# ---------------------------------------------------------------------------------------------------------------- 2. proofs of the library
@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_executed_programs_and_the_padding_instance_are_accepted(backends, oracle, hasher):
    be = backends(hasher)
    stark = T.ola_stark(**MINI)
    blob = stark.blob()
    instances = {name: M.instance(make(), **MINI, **kw) for name, (make, kw) in M.EXAMPLES.items()}
    instances["padding"] = tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(3))
    assert len(instances) == 10
    heights = {t.shape[1] for tr, _, _ in instances.values() for t in tr}
    assert 2 in heights and max(heights) >= 4096                                   # Merkle depth 0 and no FRI layer; three FRI layers
    assert {t.constraint_degree for t in stark.tables} >= {1, 3, 4, 8}             # quotient oracles of 2 and 4 words, and wider ones
    assert any(t.permutation_pairs for t in stark.tables) and any(not t.permutation_pairs for t in stark.tables)
    assert max(t.ncols for t in stark.tables) == 134
    launches = set()
    for name, (traces, params, compress) in instances.items():
        proof = bytes(be.prove_with_traces(blob, traces, params, compress))
        res = be.verify_all_proof(blob, proof, params)
        assert res, (name, res)
        assert be.verify_all_proof(blob, proof), name                              # parameters from the compress challenges
        launches.add(res.kernel_launches)
        if name in ("fibonacci", "storage", "padding"):
            with oracle.hasher(hasher):
                agrees(res, *oracle.verify_all_proof(blob, proof, params))
                bad = bytearray(proof)
                bad[len(bad) // 2] ^= 4                                             # somewhere in the middle: whatever it hits, the same verdict
                agrees(be.verify_all_proof(blob, bytes(bad), params), *oracle.verify_all_proof(blob, bytes(bad), params))
    # a 2-table set: the same two launches
    rng = np.random.default_rng(11)
    cmp_t, rc_t = tracegen.cmp_rangecheck_instance(rng, 6, 4)
    two = AirSet([T.cmp_table(), T.rangecheck_table(4)], [T.ctl_cmp_rangecheck(0, 1)]).blob()
    proof = bytes(be.prove_with_traces(two, [cmp_t, rc_t]))
    res = be.verify_all_proof(two, proof)
    assert res and res.query_jobs == 2 * 28
    launches.add(res.kernel_launches)
    assert launches == {2}
    # a trace that breaks a constraint still yields bytes (test_gpu_stark.py): rejected at the quotient identity of that table, as the oracle says
    cmp_t[T.COL_CMP_GTE, 2] ^= 1
    proof = bytes(be.prove_with_traces(two, [cmp_t, rc_t]))
    res = be.verify_all_proof(two, proof)
    assert (res.reason, res.table) == ("QUOTIENT_IDENTITY", 0)
    with oracle.hasher(hasher):
        agrees(res, *oracle.verify_all_proof(two, proof))


# ---------------------------------------------------------------------------------------------------------------- 3. the opening level
def rand_field(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def ext_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=2 * k, offset=at + 4).reshape(k, 2), at + 4 + 16 * k


def field_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=k, offset=at + 4), at + 4 + 8 * k


def bump(pair):
    return np.array([(int(pair[0]) + 1) % P, int(pair[1])], dtype=np.uint64)


def assemble(be, batches, nperm, start, fault=None):
    """The opening proof through the stepped ABI as tests/test_gpu_fri_steps.py assembles it, the transcript kept here; `fault` hands the
    device something else than the transcript drew, so that every commitment is honest about what was computed and the computation
    is not the protocol's.  -> opening-set bytes + FRI-proof bytes"""
    gt, gz, gq = batches
    mine = start.clone()
    zeta = mine.get(2)
    opening, fri = be.open(gt, gz, gq, nperm, zeta)
    at = 0
    parts = []
    for _ in range(4):
        v, at = ext_vec(opening, at)
        parts.append(v)
    ctl_last, at = field_vec(opening, at)
    q_local, at = ext_vec(opening, at)
    for v in (parts[0], parts[2], q_local, parts[1], parts[3]):
        mine.observe(v)
    mine.observe(np.stack([ctl_last, np.zeros_like(ctl_last)], axis=1))
    alpha = mine.get(2)
    fri.begin(bump(alpha) if fault == "alpha" else alpha)
    caps, beta = [], None
    for layer in range(len(fri.arity_bits)):
        cap = fri.next_layer(bump(beta) if fault == "beta0" and layer == 1 else beta)
        caps.append(cap)
        mine.observe_cap(cap)
        beta = mine.get(2)
    final_poly = fri.finish(bump(beta) if fault == "beta_last" and beta is not None else beta).copy()
    if fault == "final_word":
        final_poly[-1, 0] = (int(final_poly[-1, 0]) + 1) % P                # and observed as changed: the transcript is the verifier's
    mine.observe(final_poly)
    witness = int(be.pow(mine.get(4), bits=16))
    if fault == "pow":
        witness -= 1                                                         # the minimal witness is the first that passes
    n = 1 << (gt.log_n + 3)
    xs = np.array([int(mine.get()) % n for _ in range(28)], dtype=np.uint64)
    queries = fri.query(xs)
    fri.free()
    out = struct.pack("<I", len(caps))
    for cap in caps:
        out += struct.pack("<I", cap.shape[0]) + cap.astype("<u8").tobytes()
    out += queries + struct.pack("<I", final_poly.shape[0]) + final_poly.astype("<u8").tobytes() + struct.pack("<Q", witness)
    return opening + out, len(caps)


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("log_n,cols,nperm,layers", [(3, (3, 2, 2), 0, 0), (7, (5, 4, 4), 2, 1), (12, (9, 5, 4), 0, 2), (16, (7, 4, 2), 2, 3)])
def test_openings_whose_paths_verify_and_whose_algebra_does_not(backends, oracle, hasher, log_n, cols, nperm, layers):
    import ctypes as C
    from olavm_amd.backend import Challenger
    be = backends(hasher)
    rng = np.random.default_rng(9000 + log_n)
    n = 1 << log_n
    batches = (be.commit(rand_field(rng, (cols[0], n))), be.commit(rand_field(rng, (cols[1], n))), be.commit(rand_field(rng, (cols[2], n)), from_coeffs=True))
    caps = np.stack([b.cap() for b in batches])
    start = Challenger(hasher=hasher)
    for b in batches:
        start.observe_cap(b.cap())

    def oracle_verdict(proof):
        with oracle.hasher(hasher):
            och = oracle.challenger()
            for b in batches:
                och.observe_cap(b.cap())
            return oracle.verify_opening(caps, cols, log_n, nperm, proof, och)

    # honest: accepted, and the transcript ends where the prover's does
    prover = start.clone()
    fused = b"".join(be.open_and_prove(*batches, nperm, prover))
    honest, got_layers = assemble(be, batches, nperm, start)
    assert got_layers == layers and honest == fused
    ch = start.clone()
    res = be.verify_opening(caps, cols, log_n, nperm, honest, ch)
    assert res and res.table is None and res.query_jobs == 28 and res.merkle_jobs == 28 * (3 + layers), res
    agrees(res, *oracle_verdict(honest))
    assert bytes(C.string_at(C.byref(ch.c), C.sizeof(ch.c))) == bytes(C.string_at(C.byref(prover.c), C.sizeof(prover.c)))
    want = {"alpha": ("FRI_CONSISTENCY", 0) if layers else ("FINAL_POLY", None), "final_word": ("FINAL_POLY", None), "pow": ("POW", None)}
    if layers >= 2:
        want["beta0"] = ("FRI_CONSISTENCY", 1)
    if layers >= 1:
        want["beta_last"] = ("FINAL_POLY", None)
    for fault, (reason, layer) in want.items():
        proof, _ = assemble(be, batches, nperm, start, fault)
        ch = start.clone()
        res = be.verify_opening(caps, cols, log_n, nperm, proof, ch)
        agrees(res, *oracle_verdict(proof))                                  # the oracle's verify_opening gives the expected reason
        assert (res.reason, res.oracle_or_layer) == (reason, layer), (fault, res)
        assert res.query == (None if reason == "POW" else 0), (fault, res)  # every query fails: the first is named
        assert bytes(C.string_at(C.byref(ch.c), C.sizeof(ch.c))) == bytes(C.string_at(C.byref(start.c), C.sizeof(start.c)))   # a refusal leaves the transcript
    # the caller's transcript one element off: not this proof's
    off = start.clone()
    off.observe(np.array([1], dtype=np.uint64))
    assert not be.verify_opening(caps, cols, log_n, nperm, honest, off)
    for b in batches:
        b.free()


# ---------------------------------------------------------------------------------------------------------------- 4. several faults at once
def test_the_first_failing_check_is_the_one_reported(backends, full_blob, oracle):
    import compare_with_dump as CD
    raw = open(os.path.join(DIR, "wide_program.proof"), "rb").read()
    be = backends("poseidon")
    at = {name.split(" (")[0]: (a, b) for name, a, b in CD.parse_all_proof(raw)}
    compress = np.frombuffer(raw[-96:], dtype="<u8")
    params = [int(compress[2]), int(compress[10])]

    def flipped(*spans):
        bad = bytearray(raw)
        for s in spans:
            bad[at[s][0] + 9] ^= 1
        return bytes(bad)

    # two queries of one table: the lower one; within a query the initial trees before the layers
    bad = flipped("table 2: fri.query[17].initial_trees_proof[0].leaf", "table 2: fri.query[4].initial_trees_proof[2].path")
    res = be.verify_all_proof(full_blob, bad)
    assert (res.reason, res.table, res.query, res.oracle_or_layer) == ("MERKLE_INITIAL", 2, 4, 2), res
    agrees(res, *oracle.verify_all_proof(full_blob, bad, params))
    bad = flipped("table 5: fri.query[6].step[1].path", "table 5: fri.query[6].initial_trees_proof[1].path", "table 5: fri.query[6].step[0].path")
    res = be.verify_all_proof(full_blob, bad)
    assert (res.reason, res.table, res.query, res.oracle_or_layer) == ("MERKLE_INITIAL", 5, 6, 1), res
    bad = flipped("table 5: fri.query[6].step[1].path", "table 5: fri.query[6].step[0].path", "table 5: fri.query[9].initial_trees_proof[0].path")
    res = be.verify_all_proof(full_blob, bad)
    assert (res.reason, res.table, res.query, res.oracle_or_layer) == ("MERKLE_COMMIT", 5, 6, 0), res
    agrees(res, *oracle.verify_all_proof(full_blob, bad, params))
    # a path of table 7 and an opening of table 3: table 3 comes first, at its quotient identity
    bad = flipped("table 7: fri.query[2].initial_trees_proof[0].path", "table 3: openings.local_values")
    res = be.verify_all_proof(full_blob, bad)
    assert (res.reason, res.table, res.query) == ("QUOTIENT_IDENTITY", 3, None), res
    agrees(res, *oracle.verify_all_proof(full_blob, bad, params))
    # the other way round: a path of table 3 comes before the opening of table 7, and the host stage does not hide it
    bad = flipped("table 3: fri.query[2].initial_trees_proof[0].path", "table 7: openings.local_values")
    res = be.verify_all_proof(full_blob, bad)
    assert (res.reason, res.table, res.query, res.oracle_or_layer) == ("MERKLE_INITIAL", 3, 2, 0), res
    agrees(res, *oracle.verify_all_proof(full_blob, bad, params))
    # a changed ctl_zs_last breaks a lookup product, which is checked last of all: table 11's transcript, and with it its proof of
    # work, come first
    bad = flipped("table 11: openings.ctl_zs_last")
    res = be.verify_all_proof(full_blob, bad)
    agrees(res, *oracle.verify_all_proof(full_blob, bad, params))
    assert (res.reason, res.table) == ("POW", 11)


def test_a_lookup_that_does_not_close_is_rejected_after_every_table(backends, oracle):
    """one looked row of the bitwise table no longer selected: every table still satisfies its constraints and proves, every table's
    proof verifies, and the product of the looking tables' last Z values is not the looked table's"""
    be = backends("poseidon")
    stark = T.ola_stark(**MINI)
    blob = stark.blob()
    traces, params, compress = M.instance(M.mixed_program(), **MINI)
    twc = stark.ctls[3].looked_table
    assert twc.table == T.BITWISE and len(twc.filter_column.terms) == 1
    col = twc.filter_column.terms[0][0]
    bad = list(traces)
    bad[T.BITWISE] = traces[T.BITWISE].copy()
    bad[T.BITWISE][col, int(np.nonzero(traces[T.BITWISE][col] == 1)[0][0])] = 0
    assert oracle.check_constraints(blob, T.BITWISE, bad[T.BITWISE], [params[0]]) == -1
    proof = bytes(be.prove_with_traces(blob, bad, params, compress))
    res = be.verify_all_proof(blob, proof, params)
    assert (bool(res), res.reason, res.table, res.query, res.kernel_launches) == (False, "CTL", None, None, 2), res
    agrees(res, *oracle.verify_all_proof(blob, proof, params))
    # a broken path in the last table comes before it
    tampered = bytearray(proof)
    tampered[-96 - 8 - 32 * 2 - 40] ^= 1          # inside the last table's final polynomial: its transcript, hence its proof of work
    res = be.verify_all_proof(blob, bytes(tampered), params)
    agrees(res, *oracle.verify_all_proof(blob, bytes(tampered), params))
    assert res.table == 11 and res.reason != "CTL"


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_context_working(backends, full_blob, mini, oracle):
    import compare_with_dump as CD
    from olavm_amd.backend import Backend, OlaGpuError
    raw = open(os.path.join(DIR, "wide_program.proof"), "rb").read()
    be = backends("poseidon")
    at = {name.split(" (")[0]: (a, b) for name, a, b in CD.parse_all_proof(raw)}
    # a word >= p in an opening, a sibling, the final polynomial: an honest serializer writes none
    for span, skip in (("table 4: openings.next_values", 16), ("table 6: fri.query[3].initial_trees_proof[1].path", 32), ("table 9: fri.final_poly", 8)):
        for word in (P, 2**64 - 1):
            bad = bytearray(raw)
            a = at[span][0] + skip
            bad[a:a + 8] = struct.pack("<Q", word)
            res = be.verify_all_proof(full_blob, bytes(bad))
            assert (bool(res), res.reason, res.table, res.kernel_launches) == (False, "MALFORMED", None, 0), (span, res)
            assert res.message.startswith("malformed proof bytes")
        still_works(be, mini)
    # under Blake3 a digest is bytes: a sibling of all ones is a wrong sibling, not a malformed one
    raw3 = open(os.path.join(DIR, "wide_program_blake3.proof"), "rb").read()
    bad = bytearray(raw3)
    a = at["table 6: fri.query[3].initial_trees_proof[1].path"][0] + 32
    bad[a:a + 8] = b"\xff" * 8
    res = backends("blake3").verify_all_proof(full_blob, bytes(bad))
    assert (res.reason, res.table, res.query, res.oracle_or_layer) == ("MERKLE_INITIAL", 6, 3, 1), res
    # trailing bytes, a truncated proof, no proof
    for bad in (raw + b"\0", raw[:-1], raw[:100000], b""):
        res = be.verify_all_proof(full_blob, bad)
        assert (bool(res), res.reason) == (False, "MALFORMED"), res
        agrees(res, *oracle.verify_all_proof(full_blob, bad, None))
    still_works(be, mini, oracle)
    # the miniature set's verifier on the full set's proof: twelve tables of other shapes
    res = be.verify_all_proof(mini[0], raw)
    assert not res
    # not an AIR set: the caller's error
    with pytest.raises(OlaGpuError) as e:
        be.verify_all_proof(full_blob[:-1], raw)
    assert e.value.code == OLA_E_INVALID_ARG
    still_works(be, mini)
    # a multi-rank context is refused as by the per-phase entry points
    multi = Backend(devices=[0, 0])
    try:
        with pytest.raises(OlaGpuError) as e:
            multi.verify_all_proof(full_blob, raw)
        assert e.value.code == OLA_E_INVALID_ARG and "single-device" in str(e.value)
        blob, (traces, params, compress) = mini
        proof = bytes(multi.prove_with_traces(blob, traces, params, compress))      # and still proves
    finally:
        multi.close()
    assert be.verify_all_proof(blob, proof, params)
