"""ola_generate_cpu_trace / ola_generate_prog_trace_steps (include/ola_gpu.h): the CPU table and the program table generated in HBM from
step records, word for word against
  - the Python tables of nine executed programs of olavm_amd/air/miniexec.py (all 94 / all 18 columns),
  - tests/cpu_steps_rules.py (generation/cpu.rs and prog.rs restated) at the heights where the kernels take another path,
  - whole proofs: the two tables passed as resident tables give the committed AllProof bytes."""
import os

import numpy as np
import pytest

from olavm_amd.air import cpu_steps as S, ola_tables as T
from olavm_amd.air.dsl import P
from tests import cpu_steps_rules as R
from tests.test_gpu_tablegen import dev_table, to_dev, to_host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PROGRAMS = ("fibonacci", "mixed_program", "memory_program", "hash_program", "call_program", "tape_program", "storage_program", "heap_program",
            "wide_program")


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def instances():
    """name -> (traces, params, compress): eight programs with miniature fixed tables, wide_program at the reference's sizes"""
    from olavm_amd.air import miniexec as M
    out = {}
    for name in PROGRAMS:
        if name == "wide_program":
            out[name] = M.instance(M.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True)
        else:
            out[name] = M.instance(M.fibonacci(20) if name == "fibonacci" else getattr(M, name)())
    return out


def log2(n):
    return int(n).bit_length() - 1


def records(traces):
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    return S.from_table(cpu, S.live_rows(cpu)), S.prog_listing(pg)


def plus_p(a):
    """p added to every word that leaves room for it"""
    a = np.array(a, dtype=np.uint64)
    return np.where(a < np.uint64((1 << 32) - 1), a + np.uint64(P), a)


@pytest.mark.parametrize("name", PROGRAMS)
def test_tables_of_an_executed_program_word_for_word(be, instances, name):
    traces, params, _ = instances[name]
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    steps, listing = records(traces)
    got = be.generate_cpu_trace(steps, log2(cpu.shape[1]))
    assert got.shape == cpu.shape and np.array_equal(got, cpu)
    got, rows = be.generate_prog_trace_steps(steps, listing, params[1])
    assert got.shape == pg.shape and np.array_equal(got, pg)
    assert rows == int(pg[T.COL_PROG_FILTER_EXEC].sum())
    if name in ("tape_program", "storage_program"):          # extension lines: selector columns that carry data
        assert (cpu[T.COL_S_OP0.start:T.COL_S_DST.stop] > 1).any()


def synthetic(k, imm_rows=()):
    """k ADD steps of one program, pc = 2 i; the rows named carry an immediate word"""
    s = np.zeros((S.STEP_WORDS, k), dtype=np.uint64)
    w = lambda col: col - S.STEP_FIRST_COL
    s[w(T.COL_ADDR_CODE_RANGE.start):w(T.COL_ADDR_CODE_RANGE.stop)] = np.array([[5], [6], [7], [8]], dtype=np.uint64)
    s[w(T.COL_PC)] = 2 * np.arange(k, dtype=np.uint64)
    s[w(T.COL_CLK)] = np.arange(k, dtype=np.uint64)
    s[w(T.COL_OPCODE)] = T.op_mask("ADD")
    s[w(T.COL_INST)] = 1000 + np.arange(k, dtype=np.uint64)
    for i in imm_rows:
        s[w(T.COL_OP1_IMM), i], s[w(T.COL_IMM_VAL), i] = 1, 77 + i
    return s


def synthetic_listing(steps, log_n):
    """every word the steps execute, listed once"""
    n = 1 << log_n
    pr = np.zeros((7, n), dtype=np.uint64)
    words = sorted(set((pc, w) for _, pc, w in R.executed_rows(steps))) or [(0, 0)]
    assert len(words) <= n
    for i, (pc, word) in enumerate(words):
        pr[:4, i], pr[4, i], pr[5, i], pr[6, i] = [5, 6, 7, 8], pc, word, 1
    return pr


@pytest.mark.parametrize("n_steps", [0, 1, 7, 8])
def test_short_runs_at_eight_rows(be, instances, n_steps):
    steps, _ = records(instances["tape_program"][0])
    steps = np.ascontiguousarray(steps[:, :n_steps])
    got = be.generate_cpu_trace(steps, 3)
    assert np.array_equal(got, R.cpu_table(steps, 3))
    if n_steps == 0:
        from olavm_amd.air import tracegen as TG
        assert np.array_equal(got, TG.cpu_padding_trace(8)) and np.array_equal(be.generate_cpu_trace(None, 3), got)
    s = synthetic(n_steps)
    listing = synthetic_listing(s, 3)
    for zero_filler in (False, True):
        want, count = R.prog_table(s, listing, 3, 0xABCDEF, zero_filler)
        got, rows = be.generate_prog_trace_steps(s, listing, 0xABCDEF, zero_filler=zero_filler)
        assert rows == count == n_steps and np.array_equal(got, want)
    if n_steps == 0:        # nothing executed: zero rows whatever the flag says
        assert not got[T.COL_PROG_EXEC_CODE_ADDR_RANGE.start:T.COL_PROG_FILTER_EXEC + 1].any()


@pytest.fixture(scope="module")
def long_run():
    """one native run of more than 2^16 + 3 rows: scan and scatter cross many workgroups"""
    from olavm_amd.air import fastexec as F, miniexec as M
    traces, params, _ = F.instance(M.fibonacci_loop(47, 500), max_steps=1 << 20)
    live = S.live_rows(traces[T.CPU])
    assert live >= (1 << 16) + 3
    return traces, params, live


def cut(steps, k):
    """the first k - 1 records and the run's END record: a run of k rows"""
    return np.ascontiguousarray(np.concatenate([steps[:, :k - 1], steps[:, -1:]], axis=1))


@pytest.mark.parametrize("rows,log_n", [(65, 7), (257, 9), ((1 << 12) + 1, 13), (100, 12)])
def test_runs_cut_from_a_longer_one(be, long_run, rows, log_n):
    """65 and 257: one row past a workgroup, two workgroups; 2^12 + 1 at 2^13; 100 rows at 2^12: a padding majority"""
    traces, params, live = long_run
    steps = cut(S.from_table(traces[T.CPU], live), rows)
    want = R.cpu_table(steps, log_n)
    assert np.array_equal(be.generate_cpu_trace(steps, log_n), want)
    assert want[T.COL_IS_PADDING].sum() == (1 << log_n) - rows
    count = len(R.executed_rows(steps))
    prog_log_n = max(log_n, log2(count - 1) + 1)
    listing = np.zeros((7, 1 << prog_log_n), dtype=np.uint64)
    full = S.prog_listing(traces[T.PROGRAM])
    listed = int(full[6].sum())
    listing[:, :listed] = full[:, :listed]
    ex, _ = R.exec_side(steps, prog_log_n)
    got, n_exec = be.generate_prog_trace_steps(steps, listing, params[1])
    assert n_exec == count
    assert np.array_equal(got, be.generate_prog_trace(ex, listing, params[1]))          # the existing path, from a host-built side
    if prog_log_n <= 9:
        assert np.array_equal(got, R.prog_table(steps, listing, prog_log_n, params[1])[0])


def test_a_run_of_more_than_2_to_16_rows(be, long_run):
    traces, params, live = long_run
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    steps, listing = S.from_table(cpu, live), S.prog_listing(pg)
    d_steps = to_dev(steps)
    out = dev_table(T.NUM_CPU_COLS, log2(cpu.shape[1]))
    assert be.generate_cpu_trace(d_steps, log2(cpu.shape[1]), out=out) == log2(cpu.shape[1])
    assert np.array_equal(to_host(out), cpu)
    out = dev_table(T.NUM_PROG_COLS, log2(pg.shape[1]))
    _, rows = be.generate_prog_trace_steps(d_steps, to_dev(listing), params[1], out=out)
    assert rows == int(pg[T.COL_PROG_FILTER_EXEC].sum()) and rows > 1 << 16
    assert np.array_equal(to_host(out), pg)


def test_executed_rows_that_fill_the_table_exactly_and_one_more(be):
    from olavm_amd.backend import OlaGpuError
    s = synthetic(6, imm_rows=(1, 4))                     # 6 + 2 = 8 executed rows
    listing = synthetic_listing(s, 3)
    want, count = R.prog_table(s, listing, 3, 12345)
    assert count == 8 and want[T.COL_PROG_FILTER_EXEC].all()
    got, rows = be.generate_prog_trace_steps(s, listing, 12345)
    assert rows == 8 and np.array_equal(got, want)
    s = synthetic(6, imm_rows=(1, 4, 5))                  # 9: refused, the count returned, nothing written
    for out in (np.full((T.NUM_PROG_COLS, 8), 7, dtype=np.uint64), dev_table(T.NUM_PROG_COLS, 3, fill=7)):
        with pytest.raises(OlaGpuError) as e:
            be.generate_prog_trace_steps(s, listing, 12345, out=out)
        assert e.value.code == -1 and e.value.exec_rows == 9
        assert (to_host(out) == 7).all() if hasattr(out, "data_ptr") else (out == 7).all()
    with pytest.raises(OlaGpuError) as e:                 # more steps than rows
        be.generate_cpu_trace(synthetic(9), 3)
    assert e.value.code == -1


def test_words_not_below_p_give_the_same_tables(be, instances):
    for name in ("tape_program", "storage_program", "memory_program"):
        traces, params, _ = instances[name]
        steps, listing = records(traces)
        assert (plus_p(steps) >= np.uint64(P)).any()
        assert np.array_equal(be.generate_cpu_trace(plus_p(steps), log2(traces[T.CPU].shape[1])), traces[T.CPU])
        beta = params[1] + P if params[1] + P < 1 << 64 else params[1]
        got, _ = be.generate_prog_trace_steps(plus_p(steps), plus_p(listing), beta)
        assert np.array_equal(got, traces[T.PROGRAM])


@pytest.mark.parametrize("dev_in,dev_out", [(False, False), (False, True), (True, False), (True, True)])
def test_host_and_device_memory(be, instances, dev_in, dev_out):
    traces, params, _ = instances["storage_program"]
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    steps, listing = records(traces)
    before = steps.copy()
    s, l = (to_dev(steps), to_dev(listing)) if dev_in else (steps, listing)
    out = dev_table(T.NUM_CPU_COLS, log2(cpu.shape[1])) if dev_out else np.full(cpu.shape, 7, dtype=np.uint64)
    be.generate_cpu_trace(s, log2(cpu.shape[1]), out=out)
    assert np.array_equal(to_host(out) if dev_out else out, cpu)
    out = dev_table(T.NUM_PROG_COLS, log2(pg.shape[1])) if dev_out else np.full(pg.shape, 7, dtype=np.uint64)
    be.generate_prog_trace_steps(s, l, params[1], out=out)
    assert np.array_equal(to_host(out) if dev_out else out, pg)
    assert np.array_equal(to_host(s) if dev_in else s, before)               # the caller's records are not modified


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_generated_tables_prove_the_committed_bytes(hasher, instances):
    """wide_program: CPU and program table generated resident, constraint check clean, then the committed proof from the same context"""
    from olavm_amd.backend import Backend
    full = T.ola_stark()
    blob = full.blob()
    committed = {"poseidon": "wide_program.proof", "blake3": "wide_program_blake3.proof"}[hasher]
    traces, params, compress = instances["wide_program"]
    steps, listing = records(traces)
    b = Backend(device=0, hasher=hasher)
    try:
        d_cpu = dev_table(T.NUM_CPU_COLS, log2(traces[T.CPU].shape[1]))
        d_pg = dev_table(T.NUM_PROG_COLS, log2(traces[T.PROGRAM].shape[1]))
        b.generate_cpu_trace(to_dev(steps), log2(traces[T.CPU].shape[1]), out=d_cpu)
        b.generate_prog_trace_steps(to_dev(steps), to_dev(listing), params[1], out=d_pg)
        mixed = list(traces)
        mixed[T.CPU], mixed[T.PROGRAM] = d_cpu, d_pg
        assert b.check_constraints(full, mixed, params) == []
        proof = bytes(b.prove_with_traces(blob, mixed, params, compress))
        assert proof == bytes(b.prove_with_traces(blob, traces, params, compress))
        assert proof == open(os.path.join(HERE, "golden", "ref_verified", committed), "rb").read()
    finally:
        b.close()
