"""Whole multi-table traces that hold words >= p, through the prover: the bytes are those of the canonical trace.

include/ola_gpu.h promises that trace inputs may be non-canonical, and the reference's own generator writes such words
(generation/memory.rs:104-112,137: `p - addr`, the literal word 0xFFFFFFFF00000001 for addr = 0; GoldilocksField compares canonical
values, goldilocks_field.rs:32-37).  The whole-proof path has code of its own for them: olavm_amd/csrc/upload.h judges every staging
piece by itself (bytes, 32-bit words or 64-bit words over the link), TraceUploader::column_is_narrow tells prove_with_traces which
columns may skip canonicalize(), device-resident tables, the 2-rank path, the lean path, ola_prove_single_table and ola_commit_values*
each reduce in their own place, parameters and compress challenges in theirs.

Expected bytes never come from the library: for the full-size instance (tests/make_ref_verdict.instance(): the 2^16-row range-check
table and the 2^18-row bitwise table are the ones that are packed) they are the committed proofs tests/golden/ref_verified/wide_program*.proof,
which the reference's interpreted verify_proof accepted; for the miniature instances the oracle's proof of the CANONICAL trace
(tests/test_noncanonical_cases.py shows that the oracle gives the same bytes for either representative).  upload_stats()["link_bytes"]
equals tests/noncanonical_cases.link_bytes_model() exactly in every staged run: that is what shows that a pattern reached the path it
is named for (a packed first piece in front of a wide second one, a word >= p in the last block pack_low_* inspects, ...)."""
import functools
import os
import struct
import sys

import numpy as np
import pytest

from olavm_amd.air import miniexec as M, ola_tables as T
from tests import make_ref_verdict, noncanonical_cases as NC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "ref_verified")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "integration", "pin"))
P = NC.P
STEM = {"poseidon": "wide_program", "blake3": "wide_program_blake3", "keccak": "wide_program_keccak", "poseidon2": "wide_program_poseidon2"}
ONE_MB_PIECES = {"OLA_UPLOAD_PIECE_MB": "1", "OLA_UPLOAD_SLOTS": "2", "OLA_UPLOAD_THREADS": "4"}      # the bitwise table's columns: two pieces each
PROGRAMS = ["fibonacci", "mixed", "memory", "hash", "call", "tape", "storage", "heap", "storage_heavy"]   # tests/test_gpu_stark.py's list


@pytest.fixture(scope="module")
def backends():
    from olavm_amd.backend import Backend
    made = {}

    def get(hasher, devices=None):
        key = (hasher, None if devices is None else tuple(devices))
        if key not in made:
            made[key] = Backend(device=0, hasher=hasher) if devices is None else Backend(devices=devices, hasher=hasher)
        return made[key]
    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def full_blob():
    return T.ola_stark().blob()


@functools.lru_cache(maxsize=None)
def full_instance():
    return make_ref_verdict.instance()


@functools.lru_cache(maxsize=3)
def full_shifted(pattern):
    """the full-size traces under `pattern` (None: as generated); every pattern from a generator of the same seed"""
    traces = full_instance()[0]
    return traces if pattern is None else NC.shift_words(traces, pattern, np.random.default_rng(NC.SEED))[0]


@functools.lru_cache(maxsize=None)
def full_model(pattern, **kw):
    return NC.link_bytes_model(full_shifted(pattern), **kw)[0]


def committed(hasher):
    return open(os.path.join(DIR, STEM[hasher] + ".proof"), "rb").read()


def prove_under(be, monkeypatch, env, blob, tables, params, compress):
    """one proof with the upload settings of `env` -> (bytes, upload_stats())"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        proof = bytes(be.prove_with_traces(blob, tables, params, compress))
        return proof, be.upload_stats()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def scattered(traces, rng):
    """every column a separate allocation with gaps of odd sizes in between, as in tests/test_gpu_upload.py"""
    out, spacers = [], []
    for t in traces:
        cols = []
        for c in range(t.shape[0]):
            spacers.append(np.empty(int(rng.integers(1, 4096)), dtype=np.uint8))
            cols.append(np.array(t[c], dtype=np.uint64, copy=True))
        out.append(cols)
    return out


def on_device(t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda()


def still_holds(dev, want):
    return np.array_equal(dev.cpu().numpy().view(np.uint64), want)


# ------------------------------------------------------------------------------------------------------------ A: the full-size instance
@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("pattern", [None] + NC.PATTERNS)          # the slower index: a pattern's words are drawn once for both hashers
def test_full_size_trace_with_words_above_p_gives_the_committed_proof(backends, full_blob, monkeypatch, pattern, hasher):
    """Every pattern, one block per table, under the default upload settings and under 1 MB pieces: the committed bytes, and exactly the
    model's bytes over the link -- for the canonical trace (pattern None) too."""
    be = backends(hasher)
    _, params, compress = full_instance()
    shifted = full_shifted(pattern)
    total = sum(t.size * 8 for t in shifted)
    want = committed(hasher)
    for env, kw in (({}, {}), (ONE_MB_PIECES, {"piece_mb": 1})):
        proof, st = prove_under(be, monkeypatch, env, full_blob, shifted, params, compress)
        assert proof == want, (pattern, env)
        assert st["mode"] == "staged" and st["bytes"] == total, st
        assert st["link_bytes"] == full_model(pattern, **kw), (pattern, env, st)
    # second_half really leaves packed first pieces in front of wide second ones, `all` leaves none (1 MB pieces)
    if pattern in ("second_half", "all"):
        assert full_model(None, piece_mb=1) < full_model("second_half", piece_mb=1) < full_model("all", piece_mb=1) == total
        assert full_model(None) < full_model("second_half")


@pytest.mark.parametrize("hasher", ["keccak", "poseidon2"])
@pytest.mark.parametrize("pattern", ["all", "second_half"])
def test_full_size_trace_under_the_other_hashers(backends, full_blob, monkeypatch, pattern, hasher):
    be = backends(hasher)
    _, params, compress = full_instance()
    proof, st = prove_under(be, monkeypatch, {}, full_blob, full_shifted(pattern), params, compress)
    assert proof == committed(hasher)
    assert st["link_bytes"] == full_model(pattern), st


@pytest.mark.parametrize("pattern", ["all", "second_half"])
def test_full_size_trace_under_every_upload_setting(backends, full_blob, monkeypatch, pattern):
    """Bytes off, packing off, no pieces of their own for columns shorter than a slot, the pageable path: the committed proof, and the
    model's link bytes with the matching arguments (for the last three: every word as it is)."""
    be = backends("poseidon")
    _, params, compress = full_instance()
    shifted = full_shifted(pattern)
    total = sum(t.size * 8 for t in shifted)
    want = committed("poseidon")
    for env, kw, whole in (({"OLA_UPLOAD_PACK8": "0"}, {"pack8": False}, None), ({"OLA_UPLOAD_PACK": "0"}, {"pack": False}, True),
                           ({"OLA_UPLOAD_SOLO_KB": "0"}, {"solo_kb": 0}, True), ({"OLA_UPLOAD": "pageable"}, None, True)):
        proof, st = prove_under(be, monkeypatch, env, full_blob, shifted, params, compress)
        assert proof == want, (pattern, env)
        assert st["mode"] == env.get("OLA_UPLOAD", "staged") and st["bytes"] == total, (env, st)
        if kw is not None:
            assert st["link_bytes"] == full_model(pattern, **kw), (pattern, env, st)
        assert whole is None or st["link_bytes"] == total, (pattern, env, st)


@pytest.mark.parametrize("pattern", ["all", "second_half"])
def test_full_size_trace_in_every_input_form(backends, full_blob, monkeypatch, pattern):
    """Separately allocated columns; every table device-resident; even tables resident and odd ones on the host; two logical ranks (the
    tables are all-gathered, then reduced); the memory-lean mode.  The caller's device tables hold the shifted words afterwards, bit
    for bit: the library reduces its copy."""
    import torch
    be = backends("poseidon")
    _, params, compress = full_instance()
    shifted = full_shifted(pattern)
    want = committed("poseidon")
    proof, st = prove_under(be, monkeypatch, {}, full_blob, scattered(shifted, np.random.default_rng(11)), params, compress)
    assert proof == want and st["link_bytes"] == full_model(pattern), st
    dev = [on_device(t) for t in shifted]
    torch.cuda.synchronize()
    proof, st = prove_under(be, monkeypatch, {}, full_blob, dev, params, compress)
    assert proof == want and st["link_bytes"] == 0, st
    mixed = [d if i % 2 == 0 else t for i, (d, t) in enumerate(zip(dev, shifted))]
    proof, st = prove_under(be, monkeypatch, {}, full_blob, mixed, params, compress)
    assert proof == want
    assert st["link_bytes"] == NC.link_bytes_model(shifted[1::2])[0], st
    other = [t if i % 2 == 0 else d for i, (d, t) in enumerate(zip(dev, shifted))]       # the two packed tables on the host, their neighbours resident
    proof, st = prove_under(be, monkeypatch, {}, full_blob, other, params, compress)
    assert proof == want
    assert st["link_bytes"] == NC.link_bytes_model(shifted[0::2])[0], st
    assert all(still_holds(d, t) for d, t in zip(dev, shifted))
    two = backends("poseidon", devices=[0, 0])
    assert bytes(two.prove_with_traces(full_blob, shifted, params, compress)) == want
    assert bytes(two.prove_with_traces(full_blob, mixed, params, compress)) == want
    assert all(still_holds(d, t) for d, t in zip(dev, shifted))
    del dev, mixed, other
    monkeypatch.setenv("OLA_LEAN", "1")
    assert bytes(be.prove_with_traces(full_blob, shifted, params, compress)) == want
    monkeypatch.setenv("OLA_LEAN", "0")
    assert bytes(be.prove_with_traces(full_blob, shifted, params, compress)) == want


# ------------------------------------------------------------------------------------------------------------ B: the miniature instances
@pytest.fixture(scope="module")
def mini_blob():
    return T.ola_stark(range_bits=4, limb_bits=2).blob()


@functools.lru_cache(maxsize=None)
def mini_instance(program):
    factory, kwargs = M.EXAMPLES[program]
    return M.instance(factory(), **kwargs)


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("program", PROGRAMS)
def test_executed_programs_with_words_above_p_give_the_oracles_bytes(backends, oracle, mini_blob, program, hasher):
    be = backends(hasher)
    traces, params, compress = mini_instance(program)
    with oracle.hasher(hasher):
        want = oracle.prove_with_traces(mini_blob, traces, params, compress)
    for pattern in ("all", "zeros_to_p"):
        shifted, _ = NC.shift_words(traces, pattern, np.random.default_rng(NC.SEED))
        assert bytes(be.prove_with_traces(mini_blob, shifted, params, compress)) == want, pattern
        dev = [on_device(t) for t in shifted]
        assert bytes(be.prove_with_traces(mini_blob, dev, params, compress)) == want, pattern
        assert all(still_holds(d, t) for d, t in zip(dev, shifted))


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_per_table_entry_point_takes_words_above_p(backends, oracle, mini_blob, hasher):
    """ola_commit_values + ola_prove_single_table, table by table, on the shifted traces: reassembled as
    tests/test_gpu_stark.py::test_per_table_entry_point_reassembles_the_same_all_proof does, the oracle's proof of the canonical trace."""
    from olavm_amd.backend import Challenger
    be = backends(hasher)
    s = T.ola_stark(range_bits=4, limb_bits=2)
    traces, params, compress = mini_instance("mixed")
    with oracle.hasher(hasher):
        want = oracle.prove_with_traces(mini_blob, traces, params, compress)
    for pattern in ("all", "zeros_to_p"):
        shifted, _ = NC.shift_words(traces, pattern, np.random.default_rng(NC.SEED))
        batches = [be.commit(t) for t in shifted]
        ch = Challenger(hasher=hasher)
        for b in batches:
            ch.observe_cap(b.cap())
        ctl = [(ch.get(), ch.get()) for _ in range(2)]
        out, poff = struct.pack("<I", len(shifted)), 0
        for t, tr in enumerate(shifted):
            k = s.tables[t].n_params
            out += be.prove_single_table(mini_blob, t, tr, batches[t], ctl, params[poff:poff + k], ch)
            poff += k
        out += struct.pack("<I", len(shifted)) + b"".join(struct.pack("<Q", int(c)) for c in compress)
        for b in batches:
            b.free()
        assert out == want, pattern


# ------------------------------------------------------------------------------------------------------------ parameters >= p
@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_parameters_and_compress_words_above_p(backends, oracle, mini_blob, hasher):
    """params / compress challenges with p added: the prover reduces them for the constraint programs and for the proof's last words;
    the verifier accepts the proof with either form and stops at the same place on a damaged one."""
    import compare_with_dump as CD
    be = backends(hasher)
    traces, params, compress = M.instance(M.mixed_program(), bitwise_beta=5, program_beta=9)
    with oracle.hasher(hasher):
        want = oracle.prove_with_traces(mini_blob, traces, params, compress)
        assert oracle.verify_all_proof(mini_blob, want, params) == (0, "")
    params_p, compress_p = NC.shift_parameters(params, compress)
    assert params_p == [5 + P, 9 + P] and sum(a != b for a, b in zip(compress, compress_p)) == len(compress)
    assert bytes(be.prove_with_traces(mini_blob, traces, params_p, compress_p)) == want
    assert bytes(be.prove_with_traces(mini_blob, traces, params_p, compress)) == want
    assert bytes(be.prove_with_traces(mini_blob, traces, params, compress_p)) == want
    shifted, _ = NC.shift_words(traces, "all", np.random.default_rng(NC.SEED))
    assert bytes(be.prove_with_traces(mini_blob, shifted, params_p, compress_p)) == want
    assert be.verify_all_proof(mini_blob, want, params_p) and be.verify_all_proof(mini_blob, want, params)
    at = {name.split(" (")[0]: (a, b) for name, a, b in CD.parse_all_proof(want)}
    # table 10 (program, parameter 9) is reached only past the quotient identity of table 2 (bitwise, parameter 5)
    for span, place in (("table 10: fri.query[3].initial_trees_proof[0].path", ("MERKLE_INITIAL", 10, 3, 0)),
                        ("table 2: openings.local_values", ("QUOTIENT_IDENTITY", 2, None, None))):
        bad = bytearray(want)
        bad[at[span][0] + 9] ^= 1
        bad = bytes(bad)
        res = [be.verify_all_proof(mini_blob, bad, pr) for pr in (params, params_p)]
        assert (res[0].accepted, res[0].reason, res[0].table, res[0].query, res[0].oracle_or_layer) == \
               (res[1].accepted, res[1].reason, res[1].table, res[1].query, res[1].oracle_or_layer) and not res[1].accepted
        assert (res[1].reason, res[1].table, res[1].query, res[1].oracle_or_layer) == place, (span, res[1])
    # a wrong parameter is still a wrong parameter, in either form
    assert not be.verify_all_proof(mini_blob, want, [6 + P, 9 + P]) and not be.verify_all_proof(mini_blob, want, [6, 9])


# ------------------------------------------------------------------------------------------------------------ commitments
def commit_columns(ncols, log_n, seed):
    """canonical columns in which about half of the words are eligible: zeros, bytes, 32-bit words and field-sized words side by side"""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    cols = rng.integers(0, P, (ncols, n), dtype=np.uint64)
    kind = rng.integers(0, 6, (ncols, n))
    cols = np.where(kind == 0, np.uint64(0), np.where(kind == 1, cols & np.uint64(0xFF), np.where(kind == 2, cols >> np.uint64(32), cols)))
    cols[:, -1] = np.arange(ncols, dtype=np.uint64)              # the last word of every column is eligible: single(n-1) sits there
    return np.ascontiguousarray(cols.astype(np.uint64))


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("pattern", ["all", "single(n-1)"])
@pytest.mark.parametrize("ncols,log_n", [(5, 12), (3, 15)])
def test_commitments_of_columns_with_words_above_p(backends, oracle, ncols, log_n, pattern, hasher):
    """ola_commit_values, ola_commit_values_dev and ola_commit_coeffs of shifted columns against the oracle's commitment of the
    canonical ones: the cap, opened rows (canonical words) and their sibling paths at the first, a middle and the last leaf, and
    the coefficients."""
    import torch
    be = backends(hasher)
    cols = commit_columns(ncols, log_n, 100 * ncols + log_n)
    (shifted,), (mask,) = NC.shift_words([cols], pattern, np.random.default_rng(NC.SEED))
    if pattern == "single(n-1)":
        assert mask[:, -1].all() and mask.sum() == ncols and (shifted[:, -1] >= P).all()
    leaves = (0, (5 << log_n) + 77, (8 << log_n) - 1)
    for from_coeffs in (False, True):
        with oracle.hasher(hasher):
            ob = oracle.batch(cols, from_coeffs=from_coeffs)
            want_cap, want_coeffs, want_rows = ob.cap(), ob.coeffs(), ob.leaves()
            want_paths = [ob.prove(i) for i in leaves]
        dev = on_device(shifted)
        torch.cuda.synchronize()
        got = [be.commit(shifted, from_coeffs=from_coeffs), be.commit_dev(dev.data_ptr(), ncols, log_n, from_coeffs=from_coeffs)]
        for b in got:
            assert np.array_equal(b.cap(), want_cap)
            coeffs = b.coeffs()
            assert int(coeffs.max()) < P and np.array_equal(coeffs, want_coeffs)
            for i, path in zip(leaves, want_paths):
                row, sib = b.leaf(i)
                assert int(row.max()) < P and np.array_equal(row, want_rows[i]) and np.array_equal(sib, path), i
            b.free()
        assert still_holds(dev, shifted)
