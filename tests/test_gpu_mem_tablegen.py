"""ola_generate_memory_trace / ola_generate_cmp_trace (include/ola_gpu.h): the memory table generated in HBM from raw cells -- sorted on the
device -- and the comparison table from operand pairs, word for word against miniexec.memory_trace / tracegen.generate_cmp_trace and
their value lists: hand-made cell sets at the sizes where a height or a branch changes, ties, shuffles, words >= p, more than one
workgroup, host and device memory, the quirks flag, nine executed programs with the range-check table made from the lists the two calls
leave in HBM, and whole proofs from five generated tables."""
import os

import numpy as np
import pytest

from olavm_amd.air import dump, miniexec as M, ola_tables as T, tracegen as TG
from olavm_amd.air.dsl import P
from tests import mem_cells_rules as R
from tests.test_gpu_tablegen import add_p, dev_table, to_dev, to_host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HAND_MADE = R.hand_made()


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


def log2(n):
    return int(n).bit_length() - 1


def check_memory(got, want):
    """(table, value list, counts) of Backend.generate_memory_trace against (table, sort values, region values) of memory_trace"""
    table, rc, counts = got
    t, sort_vals, region_vals = want
    assert counts == (len(sort_vals), len(region_vals))
    assert [int(x) for x in rc] == [int(x) for x in sort_vals] + [int(x) for x in region_vals]
    assert table.shape == t.shape and np.array_equal(table, t)


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_cells_word_for_word(be, name):
    cells = HAND_MADE[name]
    want = M.memory_trace(cells)
    assert want[0].shape[1] == TG.next_pow2(max(len(cells) + 1, 8))
    check_memory(be.generate_memory_trace(R.words(cells[::-1])), want)
    if name == "stack_7":
        assert want[0].shape[1] == 8 and want[0][T.COL_MEM_REGION_PROPHET].sum() == 1          # one padding row
    if name == "stack_8":
        assert want[0].shape[1] == 16
    if name == "stack_then_heap":                   # the boundary row: a difference and its inverse, no range check
        i = 4
        assert want[0][T.COL_MEM_REGION_HEAP, i] == 1 and want[0][T.COL_MEM_FILTER_LOOKING_RC, i] == 0 and want[0][T.COL_MEM_DIFF_ADDR_INV, i] > 1
        assert len(want[1]) == len(cells) - 2 and len(want[2]) == 3
    if name == "last_cell_low":                     # the first padding row's difference is a large field element
        assert want[0][T.COL_MEM_DIFF_ADDR, 1] == P - (2**32 - 1)
    if name == "stack_0":                           # no cells: None and an empty array are the same call
        check_memory(be.generate_memory_trace(None), want)
        assert np.array_equal(want[0], TG.memory_padding_trace(8))


def test_ties_and_op_words_without_a_name(be):
    cells = R.ties()
    want = R.table(cells)
    check_memory(be.generate_memory_trace(cells), want)
    check_memory(be.generate_memory_trace(np.ascontiguousarray(cells[:, ::-1])), want)
    named = cells[:, np.isin(cells[2], list(R.RANK))]             # the cells memory_trace has names for: against memory_trace itself
    name = {T.op_mask(op): op for op in dump.MEM_OPS}
    check_memory(be.generate_memory_trace(named), M.memory_trace([(int(a), int(c), name[int(o)], int(v), int(w)) for a, c, o, v, w in named.T]))


def test_order_independence(be):
    cells = R.words(HAND_MADE["stack_then_heap"] + R.pattern(40, base=50) + HAND_MADE["one_address"])
    want = R.table(np.concatenate([cells, R.ties()], axis=1))
    cells = np.concatenate([cells, R.ties()], axis=1)
    for seed in (1, 2, 3):
        order = np.random.default_rng(seed).permutation(cells.shape[1])
        check_memory(be.generate_memory_trace(np.ascontiguousarray(cells[:, order])), want)


def test_words_not_below_p_give_the_same_tables(be):
    rng = np.random.default_rng(7)
    named = HAND_MADE["stack_then_heap"] + R.pattern(30, base=40) + [(5, 3, "MLOAD", 9, 0)]
    cells = R.words(named)
    lifted = add_p(rng, cells, share=1 / 3)
    for row in range(5):                                # addresses, clocks, op words, values and is_write words: each kind has lifted words
        assert (lifted[row] >= np.uint64(P)).any(), row
    want = M.memory_trace(named)
    check_memory(be.generate_memory_trace(lifted), want)
    # an address of p + 5 sorts as 5: in front of 6, behind 4
    few = [(4, 1, "MSTORE", 1, 1), (5, 3, "MLOAD", 9, 0), (6, 2, "MSTORE", 2, 1)]
    w = R.words(few)
    w[0, 1] += np.uint64(P)
    got = be.generate_memory_trace(w)
    check_memory(got, M.memory_trace(few))
    assert got[0][T.COL_MEM_ADDR, :3].tolist() == [4, 5, 6]
    ops = np.array([[3, 9, 7, 0, 2**32 - 5, 11], [9, 3, 7, 5, 1, 2**32 - 2]], dtype=np.uint64)
    lifted = ops + np.uint64(P)
    table, diffs = be.generate_cmp_trace(lifted)
    want, want_diffs = R.cmp_table(ops)
    assert np.array_equal(table, want) and diffs.tolist() == want_diffs


def test_more_than_one_workgroup(be):
    cells = R.big()
    want = M.memory_trace(cells)
    assert want[0].shape[1] == 1 << 13 and len(want[1]) > 4000 and len(want[2]) == 99         # 33 workgroups; heap rows in the last one
    order = np.random.default_rng(5).permutation(len(cells))
    check_memory(be.generate_memory_trace(np.ascontiguousarray(R.words(cells)[:, order])), want)


@pytest.mark.parametrize("dev_in,dev_out", [(False, False), (False, True), (True, False), (True, True)])
def test_host_and_device_memory(be, dev_in, dev_out):
    import torch
    named = HAND_MADE["stack_then_heap"] + R.pattern(20, base=30)
    cells = R.words(named)
    before = cells.copy()
    t, sort_vals, region_vals = M.memory_trace(named)
    total, n = len(sort_vals) + len(region_vals), len(named)
    c = to_dev(cells) if dev_in else cells
    out = dev_table(T.NUM_MEM_COLS, log2(t.shape[1])) if dev_out else np.full(t.shape, 7, dtype=np.uint64)
    # the value list goes into the middle of a larger buffer: what lies around the values must come back untouched
    room = 3 + 2 * n + 3
    if dev_out:
        buf = torch.full((room,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc_out = buf.data_ptr() + 3 * 8
    else:
        buf = np.full(room, 7, dtype=np.uint64)
        rc_out = buf[3:3 + 2 * n]
    _, _, counts = be.generate_memory_trace(c, out=out, rc_out=rc_out)
    assert counts == (len(sort_vals), len(region_vals))
    assert np.array_equal(to_host(out) if dev_out else out, t)
    got = to_host(buf) if dev_out else buf
    assert got[3:3 + total].tolist() == sort_vals + region_vals
    assert (got[:3] == 7).all() and (got[3 + total:] == 7).all()
    assert np.array_equal(to_host(c) if dev_in else c, before)               # the caller's cells are not modified
    # without a value list the counts are still right
    _, none, counts = be.generate_memory_trace(c, out=out, rc_out=False)
    assert none is None and counts == (len(sort_vals), len(region_vals))
    assert np.array_equal(to_host(out) if dev_out else out, t)
    # the comparison table
    ops = np.array([[3, 9, 7, 200, 0], [9, 3, 7, 1, 0]], dtype=np.uint64)
    want, want_diffs = R.cmp_table(ops)
    o = to_dev(ops) if dev_in else ops
    out = dev_table(T.COL_NUM_CMP, 3) if dev_out else np.full(want.shape, 7, dtype=np.uint64)
    diffs = dev_table(1, 3, fill=7).reshape(-1) if dev_out else np.full(8, 7, dtype=np.uint64)
    be.generate_cmp_trace(o, out=out, abs_diff_out=diffs)
    assert np.array_equal(to_host(out) if dev_out else out, want)
    got = to_host(diffs) if dev_out else diffs
    assert got[:5].tolist() == want_diffs and (got[5:] == 7).all()
    be.generate_cmp_trace(o, out=out, abs_diff_out=False)
    assert np.array_equal(to_host(out) if dev_out else out, want)


def test_the_quirks_flag(be):
    table, rc, counts = be.generate_memory_trace(None, reference_quirks=True)
    assert np.array_equal(table, TG.memory_padding_trace(8, reference_quirks=True)) and len(rc) == 0 and counts == (0, 0)
    assert np.array_equal(table, M.memory_trace([], reference_quirks=True)[0])
    out = dev_table(T.NUM_MEM_COLS, 3)
    be.generate_memory_trace(None, reference_quirks=True, out=out)
    assert np.array_equal(to_host(out), table)
    cells = HAND_MADE["stack_then_heap"]                    # with cells the flag changes nothing
    check_memory(be.generate_memory_trace(R.words(cells), reference_quirks=True), M.memory_trace(cells, reference_quirks=True))
    check_memory(be.generate_memory_trace(R.words(cells), reference_quirks=True), M.memory_trace(cells))


@pytest.mark.parametrize("n_ops", [0, 1, 2, 3, 5, (1 << 10) + 1])
def test_comparison_table_word_for_word(be, n_ops):
    rng = np.random.default_rng(n_ops)
    ops = rng.integers(0, 1 << 32, (2, n_ops), dtype=np.uint64)
    if n_ops >= 3:
        ops[:, 0], ops[:, 1], ops[:, 2] = (3, 9), (7, 7), (9, 3)        # op0 < op1, op0 == op1 (the inverse of 0), op0 > op1
    if n_ops >= 5:
        ops[:, 3], ops[:, 4] = (8, 7), (P - 1, 0)                       # a difference of 1 (its own inverse), the largest one
    want, want_diffs = R.cmp_table(ops)
    assert want.shape == (T.COL_NUM_CMP, max(2, TG.next_pow2(n_ops)))
    table, diffs = be.generate_cmp_trace(ops)
    assert np.array_equal(table, want) and diffs.tolist() == want_diffs
    if n_ops == 0:
        assert np.array_equal(be.generate_cmp_trace(None)[0], want)


@pytest.mark.parametrize("name", sorted(M.EXAMPLES))
def test_three_tables_of_an_executed_program(be, name):
    """memory and comparison tables from miniexec.execute's side lists, then the range-check table from a `vals` buffer assembled on the
    device: the CPU's values, abs_diff_out, rc_out -- filters from the returned counts"""
    import torch
    make, kw = M.EXAMPLES[name]
    prog = make()
    tree = M.StorageTree()
    if kw.get("prove_program_hash"):
        listing = prog.words()[0]
        tree.set(prog.code_addr, M.program_hash(listing + [0] * (-len(listing) % 8)))
    _, side, _ = M.execute(prog, tree=tree)
    traces, _, _ = M.instance(prog, **kw)
    cells, ops, cpu_rc = R.words(side["mem"]), np.array(side["cmp"], dtype=np.uint64).reshape(-1, 2).T, np.array(side["rc"], dtype=np.uint64)
    n_cpu, n_cmp, n_cells = len(cpu_rc), ops.shape[1], cells.shape[1]
    vals = torch.full((n_cpu + n_cmp + 2 * n_cells + 1,), -1, dtype=torch.int64, device="cuda")
    vals[:n_cpu] = torch.from_numpy(cpu_rc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    at = lambda k: vals.data_ptr() + 8 * k
    d_cmp = dev_table(T.COL_NUM_CMP, log2(traces[T.CMP].shape[1]))
    d_mem = dev_table(T.NUM_MEM_COLS, log2(traces[T.MEMORY].shape[1]))
    assert be.generate_cmp_trace(np.ascontiguousarray(ops), out=d_cmp, abs_diff_out=at(n_cpu))[0] == log2(traces[T.CMP].shape[1])
    log_n, _, (n_sort, n_region) = be.generate_memory_trace(to_dev(cells), out=d_mem, rc_out=at(n_cpu + n_cmp))
    assert log_n == log2(traces[T.MEMORY].shape[1])
    assert np.array_equal(to_host(d_cmp), traces[T.CMP]) and np.array_equal(to_host(d_mem), traces[T.MEMORY])
    n_rows = n_cpu + n_cmp + n_sort + n_region
    filters = np.zeros((4, n_rows), dtype=np.uint64)
    filters[0, :n_cpu] = 1
    filters[3, n_cpu:n_cpu + n_cmp] = 1
    filters[1, n_cpu + n_cmp:n_cpu + n_cmp + n_sort] = 1
    filters[2, n_cpu + n_cmp + n_sort:] = 1
    rc = be.generate_rc_trace(vals.data_ptr(), filters, range_bits=4, n_rows=n_rows)
    assert np.array_equal(rc, traces[T.RANGECHECK])
    assert to_host(vals)[n_rows:].tolist() == [2**64 - 1] * (2 * n_cells + 1 - n_sort - n_region)       # nothing behind the values was written


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_generated_tables_prove_the_committed_bytes(hasher):
    """wide_program at the reference's sizes: the CPU, program, memory, comparison and range-check tables generated resident, constraint check
    clean, then the committed proof from the same context"""
    import torch
    from olavm_amd.air import cpu_steps as S
    from olavm_amd.backend import Backend
    full = T.ola_stark()
    blob = full.blob()
    committed = {"poseidon": "wide_program.proof", "blake3": "wide_program_blake3.proof"}[hasher]
    prog = M.wide_program()
    listing = prog.words()[0]
    tree = M.StorageTree()
    tree.set(prog.code_addr, M.program_hash(listing + [0] * (-len(listing) % 8)))
    _, side, _ = M.execute(prog, tree=tree)
    traces, params, compress = M.instance(prog, range_bits=16, limb_bits=8, prove_program_hash=True)
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    steps = S.from_table(cpu, S.live_rows(cpu))
    cells, ops, cpu_rc = R.words(side["mem"]), np.array(side["cmp"], dtype=np.uint64).reshape(-1, 2).T, np.array(side["rc"], dtype=np.uint64)
    n_cpu, n_cmp, n_cells = len(cpu_rc), ops.shape[1], cells.shape[1]
    assert n_cpu and n_cmp and n_cells
    b = Backend(device=0, hasher=hasher)
    try:
        d = {t: dev_table(traces[t].shape[0], log2(traces[t].shape[1])) for t in (T.CPU, T.PROGRAM, T.MEMORY, T.CMP, T.RANGECHECK)}
        vals = torch.zeros((n_cpu + n_cmp + 2 * n_cells,), dtype=torch.int64, device="cuda")
        vals[:n_cpu] = torch.from_numpy(cpu_rc.view(np.int64)).cuda()
        torch.cuda.synchronize()
        b.generate_cpu_trace(to_dev(steps), log2(cpu.shape[1]), out=d[T.CPU])
        b.generate_prog_trace_steps(to_dev(steps), to_dev(S.prog_listing(pg)), params[1], out=d[T.PROGRAM])
        b.generate_cmp_trace(to_dev(ops), out=d[T.CMP], abs_diff_out=vals.data_ptr() + 8 * n_cpu)
        _, _, (n_sort, n_region) = b.generate_memory_trace(to_dev(cells), out=d[T.MEMORY], rc_out=vals.data_ptr() + 8 * (n_cpu + n_cmp))
        n_rows = n_cpu + n_cmp + n_sort + n_region
        filters = np.zeros((4, n_rows), dtype=np.uint64)
        for col, lo, hi in ((0, 0, n_cpu), (3, n_cpu, n_cpu + n_cmp), (1, n_cpu + n_cmp, n_cpu + n_cmp + n_sort), (2, n_cpu + n_cmp + n_sort, n_rows)):
            filters[col, lo:hi] = 1
        b.generate_rc_trace(vals.data_ptr(), to_dev(filters), range_bits=16, out=d[T.RANGECHECK], n_rows=n_rows)
        mixed = list(traces)
        for t, table in d.items():
            mixed[t] = table
        assert b.check_constraints(full, mixed, params) == []
        proof = bytes(b.prove_with_traces(blob, mixed, params, compress))
        assert proof == open(os.path.join(HERE, "golden", "ref_verified", committed), "rb").read()
    finally:
        b.close()
