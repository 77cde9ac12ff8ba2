"""ola_tables_from_records / ola_prove_from_records (include/ola_gpu.h): the executor's records in, twelve resident tables and AllProof
bytes out.  The records are the native generator's (OLA_TRACEGEN_RECORDS_ONLY); the tables are held word for word to
miniexec.instance's and the bytes to Backend.prove_with_traces on them, which the other tests hold to the oracle prover -- for the nine
examples under miniature parameters and both hash configurations, for wide_program at the reference's sizes against the committed
proofs, with records in device memory, with explicit challenges, with nothing crossing the link as tables, and with a refusal that
names its step and leaves the context proving."""
import os

import numpy as np
import pytest

from olavm_amd.air import fastexec as F, miniexec as M, ola_tables as T
from tests.test_gpu_tablegen import to_dev

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OLA_E_INVALID_ARG = -1
MINI = dict(range_bits=4, limb_bits=2)


@pytest.fixture(scope="module")
def backends():
    from olavm_amd.backend import Backend
    b = {"poseidon": Backend(device=0), "blake3": Backend(device=0, hasher="blake3")}
    yield b
    for be in b.values():
        be.close()


@pytest.fixture(scope="module")
def stark():
    return T.ola_stark(**MINI)


@pytest.fixture(scope="module")
def instances():
    """name -> (miniexec.instance's traces, params, compress; the native generator's records; the keyword arguments of the records calls)"""
    out = {}
    for name, (make, kw) in M.EXAMPLES.items():
        prog = make()
        rec = F.instance(prog, records_only=True, **MINI, **kw)[3]
        out[name] = (M.instance(prog, **MINI, **kw), rec, dict(result_line=bool(kw.get("prove_program_hash")), **MINI))
    return out


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("name", sorted(M.EXAMPLES))
def test_bytes_are_prove_with_traces_on_miniexecs_tables(backends, stark, instances, name, hasher):
    (traces, params, compress), rec, kw = instances[name]
    be = backends[hasher]
    want = bytes(be.prove_with_traces(stark.blob(), traces, params, compress))
    table_bytes = 8 * sum(t.size for t in traces)
    up = be.upload_stats()
    assert up["bytes"] == table_bytes and 0 < up["link_bytes"] <= table_bytes          # the host's tables went over the link ...
    assert be.prove_from_records(stark.blob(), rec, **kw) == want
    up = be.upload_stats()
    assert up["bytes"] == table_bytes and up["link_bytes"] == 0                        # ... the resident ones did not: no table byte crossed it
    if name == "fibonacci":                                            # a run without any side record goes through
        for key in ("cells", "cmp_ops", "bitwise_ops", "tape_cells", "psdn_calls", "accesses"):
            assert rec[key].shape[1] == 0, key


@pytest.mark.parametrize("name", sorted(M.EXAMPLES))
def test_every_table_of_the_set_is_miniexecs(backends, stark, instances, name):
    (traces, params, compress), rec, kw = instances[name]
    be = backends["poseidon"]
    ts = be.tables_from_records(rec, **kw)
    try:
        assert ts.params == [int(x) for x in params] and ts.compress == [int(x) for x in compress]
        assert ts.log_n == [t.shape[1].bit_length() - 1 for t in traces] == rec["log_n"]
        for t in range(12):
            got = ts.tables[t].to_host()
            assert got.shape == traces[t].shape, t
            for c in range(got.shape[0]):
                assert np.array_equal(got[c], traces[t][c]), "table %d column %d" % (t, c)
        assert be.check_constraints(stark, ts.tables, ts.params) == []
        assert bytes(be.prove_with_traces(stark.blob(), ts.tables, ts.params, ts.compress)) == bytes(be.prove_with_traces(stark.blob(), traces, params, compress))
    finally:
        ts.free()


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_wide_program_at_full_size_gives_the_committed_bytes(backends, hasher):
    committed = {"poseidon": "wide_program.proof", "blake3": "wide_program_blake3.proof"}[hasher]
    rec = F.instance(M.wide_program(), records_only=True, range_bits=16, limb_bits=8, prove_program_hash=True)[3]
    proof = backends[hasher].prove_from_records(T.ola_stark().blob(), rec, range_bits=16, limb_bits=8, result_line=True)
    assert proof == open(os.path.join(HERE, "golden", "ref_verified", committed), "rb").read()


@pytest.mark.parametrize("name", ["mixed", "storage", "tape", "hash"])
def test_records_in_device_memory_give_the_same_bytes(backends, stark, instances, name):
    (traces, params, compress), rec, kw = instances[name]
    be = backends["poseidon"]
    dev = {k: to_dev(v) if isinstance(v, np.ndarray) else v for k, v in rec.items()}
    assert be.prove_from_records(stark.blob(), dev, **kw) == be.prove_from_records(stark.blob(), rec, **kw)
    half = {k: (to_dev(v) if isinstance(v, np.ndarray) and i % 2 else v) for i, (k, v) in enumerate(sorted(rec.items()))}
    assert be.prove_from_records(stark.blob(), half, **kw) == bytes(be.prove_with_traces(stark.blob(), traces, params, compress))


@pytest.mark.parametrize("name", ["mixed", "storage"])
def test_explicit_betas_are_honoured(backends, stark, instances, name):
    make, ekw = M.EXAMPLES[name]
    _, rec, kw = instances[name]
    be = backends["poseidon"]
    traces, params, compress = M.instance(make(), bitwise_beta=5, program_beta=6, **MINI, **ekw)
    assert params == [5, 6]
    got = be.prove_from_records(stark.blob(), rec, bitwise_beta=5, program_beta=6, **kw)
    assert got == bytes(be.prove_with_traces(stark.blob(), traces, params, compress))
    assert got != be.prove_from_records(stark.blob(), rec, **kw)
    ts = be.tables_from_records(rec, bitwise_beta=5, program_beta=6, **kw)
    assert ts.params == [5, 6] and ts.compress[T.BITWISE] == 5 and ts.compress[T.PROGRAM] == 6
    ts.free()


def test_a_cpu_table_too_small_for_the_steps_is_refused_by_name(backends, stark, instances):
    from olavm_amd.backend import OlaGpuError
    (traces, params, compress), rec, kw = instances["memory"]
    be = backends["poseidon"]
    small = dict(rec)
    small["cpu_log_n"] = (rec["steps"].shape[1] - 1).bit_length() - 1                  # half the rows the steps need
    assert rec["steps"].shape[1] > 1 << small["cpu_log_n"]
    for call in (lambda: be.prove_from_records(stark.blob(), small, **kw), lambda: be.tables_from_records(small, **kw)):
        with pytest.raises(OlaGpuError) as e:
            call()
        assert e.value.code == OLA_E_INVALID_ARG and "CPU table" in str(e.value) and "more steps than 2^log_n rows" in str(e.value)
    unknown = dict(rec)
    unknown["psdn_calls"] = np.array([[1], [2], [12], [3], [0]], dtype=np.uint64)       # a length that is no whole number of blocks
    with pytest.raises(OlaGpuError) as e:
        be.prove_from_records(stark.blob(), unknown, **kw)
    assert "Poseidon-chunk table" in str(e.value)
    assert be.prove_from_records(stark.blob(), rec, **kw) == bytes(be.prove_with_traces(stark.blob(), traces, params, compress))


def refused_then_builds(be, instance, bad, message, table):
    """`bad` is refused with exactly `message` behind the name of its step; the untouched records then give miniexec's `table` on the
    same context"""
    from olavm_amd.backend import OlaGpuError
    (traces, params, compress), rec, kw = instance
    with pytest.raises(OlaGpuError) as e:
        be.tables_from_records(bad, **kw)
    assert e.value.code == OLA_E_INVALID_ARG and str(e.value) == "ola_gpu error -1: " + message
    ts = be.tables_from_records(rec, **kw)
    try:
        assert np.array_equal(ts.tables[table].to_host(), traces[table])
    finally:
        ts.free()


def test_an_unknown_flag_in_an_access_record_is_refused_by_the_storage_step(backends, instances):
    rec = instances["storage"][1]
    bad = dict(rec)
    bad["accesses"] = rec["accesses"].copy()
    assert bad["accesses"].shape[1] > 1
    bad["accesses"][12, 1] |= np.uint64(8)                                              # bit 3 of the flags word: not a flag
    refused_then_builds(backends["poseidon"], instances["storage"], bad,
                        "storage-access table: invalid argument: unknown flag in an access record", T.STORAGE_ACCESS)


def test_a_poseidon_call_of_length_0_is_refused_by_the_chunk_step(backends, instances):
    rec = instances["hash"][1]
    bad = dict(rec)
    bad["psdn_calls"] = rec["psdn_calls"].copy()
    assert bad["psdn_calls"].shape[1] > 0
    bad["psdn_calls"][2, 0] = 0                                                         # len
    refused_then_builds(backends["poseidon"], instances["hash"], bad,
                        "Poseidon-chunk table: invalid argument: a POSEIDON call of length 0", T.POSEIDON_CHUNK)


def test_a_program_table_too_small_for_the_executed_rows_is_refused_by_the_program_step(backends, instances):
    (traces, _, _), rec, _ = instances["mixed"]
    exec_rows = int(traces[T.PROGRAM][T.COL_PROG_FILTER_EXEC].sum())
    bad = dict(rec)
    bad["prog_log_n"] = (exec_rows - 1).bit_length() - 1                                # one below what the executed rows need
    assert 1 <= bad["prog_log_n"] < rec["prog_log_n"] and exec_rows > 1 << bad["prog_log_n"]
    bad["listing"] = np.ascontiguousarray(rec["listing"][:, :1 << bad["prog_log_n"]])
    refused_then_builds(backends["poseidon"], instances["mixed"], bad,
                        "program table: invalid argument: the steps give more executed rows than 2^log_n (the count is in *exec_rows_out)",
                        T.PROGRAM)
