"""ola_generate_storage_trace / ola_generate_poseidon_table (include/ola_gpu.h): the account-storage tree hashed on the device, the
storage-access table and the Poseidon table's inputs, word for word against miniexec's StorageTree and storage_trace -- hand-made batches
at the bit positions where a limb ends, a sibling sits at the root or at the leaf pair, reads, overwrites, a silent write, words >= p,
host and device memory, the caller's siblings -- a batch of more than one workgroup against the native generator's tables, the Poseidon
table at its padded height, and execution to proof bytes through the native
generator's hashes-only mode."""
import json
import os

import numpy as np
import pytest

from olavm_amd.air import fastexec, miniexec as M, ola_tables as T
from olavm_amd.air.dsl import P
from tests import storage_rules as R
from tests.test_gpu_tablegen import dev_table, to_dev, to_host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


def log2(n):
    return int(n).bit_length() - 1


def run(be, name, recs=None, siblings=None):
    """one call on host buffers -> (table, Poseidon inputs, filters, roots)"""
    batch = R.BATCHES[name]
    stride = R.psdn_rows(batch)[1]
    inputs, filters = R.psdn_buffers(stride)
    table, roots = be.generate_storage_trace(R.records(batch) if recs is None else recs, siblings=siblings, psdn_inputs=inputs, psdn_filters=filters)
    return table, inputs, filters, roots


def check(got, name):
    table, inputs, filters, roots = got
    ref = R.reference(name)
    want_inputs, want_filters = R.expected_psdn(ref, inputs.shape[1])
    assert table.shape == ref["table"].shape
    for c in range(T.NUM_COL_ST):
        assert np.array_equal(table[c], ref["table"][c]), "column %d" % c
    assert np.array_equal(inputs, want_inputs) and np.array_equal(filters, want_filters)
    assert np.array_equal(roots, ref["roots"])


@pytest.mark.parametrize("name", ["one_write", "bit_patterns", "write_read_overwrite", "split_bits", "silent_then_for_prog"])
def test_hand_made_batches_word_for_word(be, name):
    got = run(be, name)
    check(got, name)
    table, ref = got[0], R.reference(name)
    m = len(ref["live"])
    assert table.shape[1] == max(8, 1 << log2(2 * 256 * m - 1)) and (table[T.COL_ST_IS_PADDING] == 0).sum() == 256 * m
    if name == "one_write":                      # an empty tree before: every sibling is the empty tree's node, the old root its root
        empty = M.StorageTree()
        assert [int(x) for x in got[3][:4]] == list(empty.root())
        assert [int(table[c, 255]) for c in T.COL_ST_SIB_RANGE] == [0, 0, 0, 0] and table[T.COL_ST_HASH_TYPE, 255] == 1
    if name == "split_bits":                     # the last access: its siblings at layers 1, 64, 65 and 256 are the other keys' nodes
        empty = M.StorageTree()
        base = 256 * 4
        for layer in (1, 64, 65, 256):
            assert tuple(int(table[c, base + layer - 1]) for c in T.COL_ST_SIB_RANGE) != tuple(empty.default[layer]), layer
        assert tuple(int(table[c, base + 1]) for c in T.COL_ST_SIB_RANGE) == tuple(empty.default[2])
    if name == "silent_then_for_prog":           # no rows for the silent write, but its leaf is what the read finds
        assert m == 1 and table[T.COL_ST_FILTER_IS_FOR_PROG].sum() == 1 and table[T.COL_ST_FILTER_IS_FOR_PROG, 255] == 1
        assert [int(table[c, 255]) for c in T.COL_ST_PATH_RANGE] == [901, 902, 903, 904]
        assert np.array_equal(got[3][:4], got[3][4:])


def test_no_access_at_all(be):
    for recs in (None, np.zeros((R.WORDS, 0), dtype=np.uint64)):
        table, roots = be.generate_storage_trace(recs)
        want = M.storage_trace([])
        assert table.shape == want.shape == (48, 8) and np.array_equal(table, want)
        assert [int(x) for x in roots] == list(M.StorageTree().root()) * 2
    # only a silent write: the all-padding table with zero roots, and the tree's root twice
    batch = R.BATCHES["silent_then_for_prog"][:1]
    table, roots = be.generate_storage_trace(R.records(batch))
    assert np.array_equal(table, M.storage_trace([]))
    tree = M.StorageTree()
    tree.set(*batch[0][:2])
    assert [int(x) for x in roots] == list(tree.root()) * 2


def test_words_not_below_p_give_the_same_table(be):
    name = "write_read_overwrite"
    recs = R.records(R.BATCHES[name])
    lifted = recs.copy()
    lifted[0:12] += np.uint64(P)                  # keys, values and pre-values of this batch are small: every word has room for p
    lifted[12, 1] += np.uint64(P)                 # the flags and row words of one record as well
    lifted[13, 2] += np.uint64(P)
    assert (lifted[0:12] >= np.uint64(P)).all()
    check(run(be, name, recs=lifted), name)
    recs, sib = R.sibling_mode_records(name)
    small = sib < np.uint64((1 << 64) - P)
    check(run(be, name, recs=recs + np.where(np.arange(R.WORDS)[:, None] < 12, np.uint64(P), np.uint64(0)), siblings=np.where(small, sib + np.uint64(P), sib)),
          name)


@pytest.mark.parametrize("dev_in,dev_out", [(False, False), (False, True), (True, False), (True, True)])
def test_host_and_device_memory(be, dev_in, dev_out):
    import torch
    name = "write_read_overwrite"
    batch, ref = R.BATCHES[name], R.reference(name)
    recs = R.records(batch)
    before = recs.copy()
    stride = R.psdn_rows(batch)[1]
    inputs, filters = R.psdn_buffers(stride)
    if dev_out:
        out = dev_table(48, log2(ref["table"].shape[1]))
        d_in, d_f = to_dev(inputs), to_dev(filters)
        roots = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        log_n, got_roots = be.generate_storage_trace(to_dev(recs) if dev_in else recs, out=out, psdn_inputs=d_in, psdn_filters=d_f, roots_out=roots)
        assert log_n == log2(ref["table"].shape[1]) and got_roots is roots
        got = to_host(out), to_host(d_in), to_host(d_f), to_host(roots)
    else:
        table, roots = be.generate_storage_trace(to_dev(recs) if dev_in else recs, psdn_inputs=inputs, psdn_filters=filters)
        got = table, inputs, filters, roots
    check(got, name)
    assert np.array_equal(recs, before)


@pytest.mark.parametrize("name", ["one_write", "bit_patterns", "write_read_overwrite", "split_bits", "silent_then_for_prog"])
def test_the_callers_siblings_give_the_same_table(be, name):
    recs, sib = R.sibling_mode_records(name)
    assert sib.shape == (1024, recs.shape[1])
    got = run(be, name, recs=recs, siblings=sib)
    check(got, name)
    # one access alone is complete with its siblings: the accesses are independent of each other
    last = recs.shape[1] - 1
    table, _ = be.generate_storage_trace(np.ascontiguousarray(recs[:, last:]), siblings=np.ascontiguousarray(sib[:, last:]))
    want = R.reference(name)["table"]
    for c in set(range(T.NUM_COL_ST)) - {T.COL_ST_ACCESS_IDX}:
        assert np.array_equal(table[c, :256], want[c, 256 * last:256 * (last + 1)]), c


def test_more_than_one_workgroup(be):
    """storage_heavy_program(70, 0): 141 accesses with rows and the program hash's silent write, 282 states per level, against the native
    generator's table path in every column of both tables"""
    prog = M.storage_heavy_program(70, 0)
    traces, params, _ = fastexec.instance(prog, range_bits=4, limb_bits=2, prove_program_hash=True)
    rec = fastexec.instance(prog, range_bits=4, limb_bits=2, prove_program_hash=True, hashes_only=True)[3]
    recs, inputs, filters = rec["accesses"], rec["psdn_inputs"], rec["psdn_filters"]
    assert recs.shape[1] == 142 and ((recs[12] & np.uint64(R.SILENT)) != 0).sum() == 1
    table, roots = be.generate_storage_trace(recs, psdn_inputs=inputs, psdn_filters=filters)
    for t, got in ((T.STORAGE_ACCESS, table), (T.POSEIDON, be.generate_poseidon_table(inputs, filters))):
        assert got.shape == traces[t].shape
        for c in range(got.shape[0]):
            assert np.array_equal(got[c], traces[t][c]), (t, c)
    assert M.derive_program_beta(roots[:4], roots[4:]) == params[1]


def test_poseidon_table_golden_rows_and_padding(be):
    g = json.load(open(os.path.join(HERE, "golden", "poseidon_air_rows.json")))["rows"]
    rng = np.random.default_rng(11)
    for n_rows, stride in ((0, 0), (0, 4), (5, 9), (8, 11), (300, 301), (300, 300)):
        inputs = rng.integers(0, P, size=(12, stride), dtype=np.uint64)
        filters = rng.integers(0, 2, size=(4, stride), dtype=np.uint64)
        if n_rows:
            inputs[:, 0] = 0
            inputs[:, 1] = np.array(g["1000"][4:16], dtype=np.uint64)
            filters[:, :2] = 0
        n = max(8, 1 << log2(max(2 * n_rows - 1, 1)))
        for f in (filters, None):
            table = be.generate_poseidon_table(inputs, f, n_rows=n_rows)
            assert table.shape == (134, n)
            for i in range(n_rows, n):                                                       # the padding: ZERO-hash rows
                assert [int(x) for x in table[:, i]] == g["ZERO"], i
            if n_rows:
                assert [int(x) for x in table[:, 0]] == g["ZERO"] and [int(x) for x in table[:, 1]] == g["1000"]
                want = be.generate_poseidon_trace(np.ascontiguousarray(inputs[:, :n_rows]), None if f is None else np.ascontiguousarray(f[:, :n_rows]))
                assert np.array_equal(table[:, :n_rows], want)
    # words >= p, device buffers
    inputs = rng.integers(0, 1 << 32, size=(12, 70), dtype=np.uint64)
    want = be.generate_poseidon_table(inputs, n_rows=65)
    out = dev_table(134, 7)
    assert be.generate_poseidon_table(to_dev(inputs + np.uint64(P)), n_rows=65, out=out) == 7
    assert np.array_equal(to_host(out), want)


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("example", ["storage", "storage_heavy"])
def test_hashes_path_proves_the_table_paths_bytes(example, hasher):
    """execution to proof bytes with the native generator in its hashes-only mode: the storage and Poseidon tables from the records, the
    program table's challenge from the roots the device returns, and the CPU, program, memory, comparison and range-check tables from
    steps and cells -- seven tables generated resident next to the five small host-filled ones"""
    import torch
    from olavm_amd.backend import Backend
    make, kw = M.EXAMPLES[example]
    prog = make()
    traces, params, compress = fastexec.instance(prog, **kw)
    lean, lean_params, lean_compress, rec = fastexec.instance(prog, hashes_only=True, **kw)
    full = T.ola_stark(range_bits=4, limb_bits=2)
    b = Backend(device=0, hasher=hasher)
    try:
        want = bytes(b.prove_with_traces(full.blob(), traces, params, compress))
        d = {t: dev_table(traces[t].shape[0], log2(traces[t].shape[1])) for t in (T.CPU, T.PROGRAM, T.MEMORY, T.CMP, T.RANGECHECK, T.STORAGE_ACCESS, T.POSEIDON)}
        assert [rec["storage_log_n"], rec["poseidon_log_n"]] == [log2(traces[t].shape[1]) for t in (T.STORAGE_ACCESS, T.POSEIDON)]
        d_in, d_f = to_dev(rec["psdn_inputs"]), to_dev(rec["psdn_filters"])
        _, roots = b.generate_storage_trace(to_dev(rec["accesses"]), out=d[T.STORAGE_ACCESS], psdn_inputs=d_in, psdn_filters=d_f)
        b.generate_poseidon_table(d_in, d_f, out=d[T.POSEIDON])
        beta = fastexec.program_beta(roots)
        assert lean_params[1] is None and beta == params[1]
        lean_params[1] = lean_compress[T.PROGRAM] = beta
        assert lean_params == params and lean_compress == compress
        n_cpu, n_cmp, n_cells = len(rec["cpu_rc"]), rec["cmp_ops"].shape[1], rec["cells"].shape[1]
        vals = torch.zeros((n_cpu + n_cmp + 2 * n_cells + 1,), dtype=torch.int64, device="cuda")
        vals[:n_cpu] = torch.from_numpy(rec["cpu_rc"].view(np.int64)).cuda()
        torch.cuda.synchronize()
        b.generate_cpu_trace(to_dev(rec["steps"]), rec["cpu_log_n"], out=d[T.CPU])
        b.generate_prog_trace_steps(to_dev(rec["steps"]), rec["listing"], beta, out=d[T.PROGRAM])
        b.generate_cmp_trace(rec["cmp_ops"], out=d[T.CMP], abs_diff_out=vals.data_ptr() + 8 * n_cpu)
        _, _, (n_sort, n_region) = b.generate_memory_trace(rec["cells"], out=d[T.MEMORY], rc_out=vals.data_ptr() + 8 * (n_cpu + n_cmp))
        n_rows = n_cpu + n_cmp + n_sort + n_region
        filters = np.zeros((4, n_rows), dtype=np.uint64)
        for col, lo, hi in ((0, 0, n_cpu), (3, n_cpu, n_cpu + n_cmp), (1, n_cpu + n_cmp, n_cpu + n_cmp + n_sort), (2, n_cpu + n_cmp + n_sort, n_rows)):
            filters[col, lo:hi] = 1
        b.generate_rc_trace(vals.data_ptr(), filters, range_bits=4, out=d[T.RANGECHECK], n_rows=n_rows)
        for t, table in d.items():
            assert lean[t] is None
            lean[t] = table
        for t in (T.STORAGE_ACCESS, T.POSEIDON):
            assert np.array_equal(to_host(d[t]), traces[t]), t
        assert b.check_constraints(full, lean, params) == []
        assert bytes(b.prove_with_traces(full.blob(), lean, params, compress)) == want
    finally:
        b.close()
