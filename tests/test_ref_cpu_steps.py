"""generation/cpu.rs generate_cpu_trace and generation/prog.rs generate_prog_trace of the reference, run by tools/rust_air_eval.py
--tracegen cpu_steps on 37 synthetic steps that reach the branches no program of olavm_amd/air/miniexec.py reaches (cross-contract calls,
END inside a callee, an opcode word of 0, ...): tests/golden/ref_cpu_steps.json holds the step records, the two-program listing and the
reference's tables at 37, 32 and 0 steps.  On the CPU the plain restatement of the rules (tests/cpu_steps_rules.py) must give the fixture
and the tables of executed programs; on the GPU ola_generate_cpu_trace / ola_generate_prog_trace_steps must give the fixture."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from olavm_amd.air import cpu_steps as S, ola_tables as T
from tests import cpu_steps_rules as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "ref_cpu_steps.json")
REF = "/root/reference"


@pytest.fixture(scope="module")
def ref():
    return json.load(open(FIXTURE))


def run_inputs(ref, k):
    """-> (records of the first k steps, the reference's CPU table, its program table, the listing side at that height, beta)"""
    run = ref["runs"][str(k)]
    steps = np.ascontiguousarray(np.array(ref["steps"], dtype=np.uint64).T[:, :k]).reshape(S.STEP_WORDS, k)
    cpu, pg = np.array(run["cpu"], dtype=np.uint64), np.array(run["prog"], dtype=np.uint64)
    listing = np.zeros((7, pg.shape[1]), dtype=np.uint64)
    i = 0
    for addr, words in ref["listing"]:
        for pc, w in enumerate(words):
            listing[:4, i], listing[4, i], listing[5, i], listing[6, i] = addr, pc, w, 1
            i += 1
    return steps, cpu, pg, listing, run["beta"]


def test_fixture_covers_the_branches(ref):
    steps = np.array(ref["steps"], dtype=np.uint64).T
    assert steps.shape == (S.STEP_WORDS, 37) and sorted(int(k) for k in ref["runs"]) == [0, 32, 37]
    col = lambda c: steps[c - S.STEP_FIRST_COL]
    main = col(T.COL_IS_EXT_LINE) == 0
    assert set(int(x) for x in col(T.COL_OPCODE)[main]) == set(R.MASK.values()) | {0}
    for name in ("SLOAD", "SSTORE", "SCCALL", "TLOAD", "TSTORE", "END"):
        assert ((col(T.COL_OPCODE) == R.MASK[name]) & ~main).any(), name
    end = col(T.COL_OPCODE) == R.MASK["END"]
    assert {(int(e), int(x)) for e, x in zip(col(T.COL_ENV_IDX)[end], col(T.COL_IS_EXT_LINE)[end])} == {(0, 0), (0, 1), (2, 0), (2, 1)}
    tload = (col(T.COL_OPCODE) == R.MASK["TLOAD"]) & ~main
    assert {(int(a), int(b)) for a, b in zip(col(T.COL_OP0)[tload], col(T.COL_OP1)[tload])} == {(0, 1), (0, 3), (1, 1), (1, 3)}
    for name in ("MLOAD", "MSTORE"):
        assert col(T.COL_OP1_IMM)[col(T.COL_OPCODE) == R.MASK[name]].tolist() == [0]
    assert set(col(T.COL_OP1_IMM).tolist()) == {0, 1} and steps[S.STEP_COPIED_COLS].any()
    assert (steps[T.COL_S_OP0.start - S.STEP_FIRST_COL:T.COL_S_DST.stop - S.STEP_FIRST_COL] > 1).any()        # selector columns as data carriers
    # both outcomes of ext_length == ext_cnt on extension lines
    want = np.array(ref["runs"]["37"]["cpu"], dtype=np.uint64)
    assert set(want[T.COL_IS_NEXT_LINE_DIFF_INST, :37][~main].tolist()) == {0, 1}


@pytest.mark.parametrize("k", [37, 32, 0])
def test_the_restated_rules_give_the_references_tables(ref, k):
    steps, cpu, pg, listing, beta = run_inputs(ref, k)
    assert cpu.shape == (T.NUM_CPU_COLS, {37: 64, 32: 32, 0: 1}[k]) and pg.shape == (T.NUM_PROG_COLS, {37: 64, 32: 32, 0: 32}[k])
    assert np.array_equal(R.cpu_table(steps, cpu.shape[1].bit_length() - 1), cpu)
    got, count = R.prog_table(steps, listing, pg.shape[1].bit_length() - 1, beta, zero_filler=True)
    assert np.array_equal(got, pg) and count == int(pg[T.COL_PROG_FILTER_EXEC].sum())


@pytest.mark.parametrize("name", ["mixed_program", "memory_program", "call_program", "tape_program"])
def test_the_restated_rules_give_the_tables_of_executed_programs(name):
    from olavm_amd.air import miniexec as M
    traces, params, _ = M.instance(getattr(M, name)())
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    steps = S.from_table(cpu, S.live_rows(cpu))
    assert np.array_equal(R.cpu_table(steps, cpu.shape[1].bit_length() - 1), cpu)
    got, count = R.prog_table(steps, S.prog_listing(pg), pg.shape[1].bit_length() - 1, params[1])
    assert np.array_equal(got, pg) and count == int(pg[T.COL_PROG_FILTER_EXEC].sum())


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_what_the_reference_computes_today():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rust_air_eval.py"), "--tracegen", "cpu_steps", "--check", "--reference", REF],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "up to date" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("k", [37, 32, 0])
def test_device_tables_equal_the_references(ref, k):
    from olavm_amd.backend import Backend
    steps, cpu, pg, listing, beta = run_inputs(ref, k)
    b = Backend(device=0)
    try:
        log_n = max(1, cpu.shape[1].bit_length() - 1)               # the reference's table of no steps has one row, the smallest here has two
        got = b.generate_cpu_trace(steps, log_n)
        assert np.array_equal(got[:, :cpu.shape[1]], cpu) and (got == got[:, -1:]).all() if k == 0 else np.array_equal(got, cpu)
        got, rows = b.generate_prog_trace_steps(steps, listing, beta, zero_filler=True)
        assert np.array_equal(got, pg) and rows == int(pg[T.COL_PROG_FILTER_EXEC].sum())
    finally:
        b.close()
