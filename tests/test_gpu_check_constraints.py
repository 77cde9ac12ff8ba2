"""ola_check_constraints on the GPU: which constraint of which table fails at which row.

What the report must say comes from two sources that share nothing with the code under test:
  * `failing_rows` below: the table's node DAG and `emits` (olavm_amd/air/dsl.py AirTable) evaluated with Python integers mod p on
    (row i, row i + 1 mod n), in the style of tests/test_codegen_host.py::reference_point; an emit fails at a row iff its value is
    non-zero and its kind applies there (every row / every row but the last / row 0 / row n - 1);
  * the oracle's row-by-row check (oracle/stark.cpp oracle_check_constraints), which returns the first failing row of a table.
An emit's value at row i reads rows i and i + 1 only, so a single changed cell at row r can only change the verdict of rows r - 1 and
r: for tables of more than 256 rows the evaluator looks at those two rows, and the oracle's verdict on the unchanged trace (no
failing row) stands for all the others.  The permutation and lookup sections are predicted from multisets of rows."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest

from olavm_amd.air import ola_tables as T
from olavm_amd.air.dsl import (KIND_ALL, KIND_FIRST, KIND_LAST, KIND_TRANSITION, OP_ADD, OP_CONST, OP_ISZERO, OP_LOCAL, OP_MUL, OP_NEXT, OP_PARAM,
                               OP_SUB, P)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_NAMES = {KIND_ALL: "constraint", KIND_TRANSITION: "constraint_transition", KIND_FIRST: "constraint_first_row", KIND_LAST: "constraint_last_row"}
NCH = 2
HASHERS = ["poseidon", "blake3", "poseidon2", "poseidon2_pow_poseidon"]
PROGRAMS = ["fibonacci", "mixed", "memory", "hash", "call", "tape", "storage", "heap", "storage_heavy"]
# single-cell corruptions: seeds per table, the same for the miniature and the full-size instance (checked on the CPU: for every
# table at least one of them is flagged by the evaluator in either instance; most cells of the range-check and sccall tables are
# read by no constraint, seeds 0..2 hit none that is: these two tables have seeds of their own)
SEEDS = (0, 1, 2)
TABLE_SEEDS = {4: (0, 7, 8), 9: (0, 11, 21)}
SUPPLIED = [(0x1234567890ABCDEF, 0x0FEDCBA987654321), (0xFFFFFFFF00000000, 3)]          # (beta, gamma) x 2, one word >= p


# ------------------------------------------------------------------------------------------------ the independent evaluator
_sched = {}


def failing_rows(tab, trace, params, rows=None):
    """-> per emit of `tab` (AirTable.emits order) the sorted rows, among `rows` (default: all), at which it fails."""
    n = trace.shape[1]
    if id(tab) not in _sched:
        _sched[id(tab)] = tab.schedule()
    out = [[] for _ in tab.emits]
    for i in (range(n) if rows is None else sorted({r % n for r in rows})):
        loc = [int(x) % P for x in trace[:, i]]
        nxt = [int(x) % P for x in trace[:, (i + 1) % n]]
        val, e = {}, 0
        for it in _sched[id(tab)]:
            if it[0] == "emit":
                kind, v = it[1], val[it[2]]
                applies = kind == KIND_ALL or (kind == KIND_TRANSITION and i != n - 1) or (kind == KIND_FIRST and i == 0) or (kind == KIND_LAST and i == n - 1)
                if v != 0 and applies:
                    out[e].append(i)
                e += 1
                continue
            j = it[1]
            op, a, b = tab.nodes[j]
            if op == OP_LOCAL:
                v = loc[a]
            elif op == OP_NEXT:
                v = nxt[a]
            elif op == OP_CONST:
                v = int(a) % P
            elif op == OP_PARAM:
                v = int(params[a]) % P
            elif op == OP_ADD:
                v = (val[a] + val[b]) % P
            elif op == OP_SUB:
                v = (val[a] - val[b]) % P
            elif op == OP_MUL:
                v = val[a] * val[b] % P
            elif op == OP_ISZERO:
                v = 1 if val[a] == 0 else 0
            else:
                raise ValueError(op)
            val[j] = v
    return out


def table_params(airset, params, t):
    off = sum(x.n_params for x in airset.tables[:t])
    return [int(x) for x in (params or [])[off:off + airset.tables[t].n_params]]


def expected_air(airset, t, trace, params, rows=None):
    tab = airset.tables[t]
    fr = failing_rows(tab, trace, table_params(airset, params, t), rows)
    return [{"table": t, "section": "AIR", "index": e, "kind": KIND_NAMES[tab.emits[e][0]], "first_row": r[0], "rows_failing": len(r)}
            for e, r in enumerate(fr) if r]


def strip(report, section=None, table=None):
    keys = ("table", "section", "index", "kind", "first_row", "rows_failing")
    return [{k: d[k] for k in keys} for d in report if (section is None or d["section"] == section) and (table is None or d["table"] == table)]


def col_eval(col, trace, i):
    return (sum(int(trace[c, i]) % P * f for c, f in col.terms) + col.constant) % P


def lookup_sides(airset, traces, li):
    """-> (multiset of looking tuples, multiset of looked tuples) of lookup li over the filter-selected rows"""
    def side(twcs):
        m = Counter()
        for twc in twcs:
            tr = traces[twc.table]
            for i in range(tr.shape[1]):
                if twc.filter_column is None or col_eval(twc.filter_column, tr, i) == 1:
                    m[tuple(col_eval(c, tr, i) for c in twc.columns)] += 1
        return m
    ctl = airset.ctls[li]
    return side(ctl.looking_tables), side([ctl.looked_table])


def expected_lookups(airset, traces):
    out = []
    for li in range(len(airset.ctls)):
        looking, looked = lookup_sides(airset, traces, li)
        if looking != looked:
            for c in range(NCH):
                out.append({"table": airset.ctls[li].looked_table.table, "section": "LOOKUP", "index": li, "kind": c,
                            "first_row": sum(looking.values()), "rows_failing": sum(looked.values())})
    return sorted(out, key=lambda d: (d["table"], d["index"], d["kind"]))


def expected_permutation_batches(tab, trace):
    bad = set()
    for p, pair in enumerate(tab.permutation_pairs):
        lhs = Counter(tuple(int(trace[l, i]) % P for l, _ in pair) for i in range(trace.shape[1]))
        rhs = Counter(tuple(int(trace[r, i]) % P for _, r in pair) for i in range(trace.shape[1]))
        if lhs != rhs:
            for c in range(NCH):
                bad.add((p * NCH + c) // tab.quotient_degree_factor)
    return sorted(bad)


def corrupt(traces, t, seed):
    """a copy of the traces with one seeded cell of table t changed to another value -> (traces, column, row)"""
    rng = np.random.default_rng(1000 * t + seed)
    tr = traces[t].copy()
    c, r = int(rng.integers(0, tr.shape[0])), int(rng.integers(0, tr.shape[1]))
    tr[c, r] = (int(tr[c, r]) % P + 1 + int(rng.integers(0, 1 << 16))) % P
    out = list(traces)
    out[t] = tr
    return out, c, r


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def mini():
    return T.ola_stark(range_bits=4, limb_bits=2)


@pytest.fixture(scope="module")
def full():
    return T.ola_stark()


@pytest.fixture(scope="module")
def mini_instances():
    from olavm_amd.air import miniexec as M
    from tests import tracegen
    inst = {}
    for name in PROGRAMS:
        factory, kwargs = M.EXAMPLES[name]
        inst[name] = M.instance(factory(), **kwargs)
    inst["padding"] = tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(3))
    return inst


@pytest.fixture(scope="module")
def full_instance():
    from tests.make_ref_verdict import instance
    return instance()


# ------------------------------------------------------------------------------------------------ 1. valid traces
@pytest.mark.parametrize("hasher", HASHERS)
def test_valid_traces_report_nothing(hasher, mini, full, mini_instances, full_instance):
    from olavm_amd.backend import Backend
    b = Backend(device=0, hasher=hasher)
    try:
        for name, (traces, params, _) in mini_instances.items():
            for ch in (None, SUPPLIED):
                assert b.check_constraints(mini, traces, params, ctl_challenges=ch) == [], (name, ch)
        traces, params, _ = full_instance
        assert len(traces) == 12
        for ch in (None, SUPPLIED):
            assert b.check_constraints(full, traces, params, ctl_challenges=ch) == []
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ 2. single-cell corruptions
@pytest.mark.parametrize("size", ["miniature", "full"])
@pytest.mark.parametrize("t", range(12))
def test_single_cell_corruptions(be, oracle, mini, full, mini_instances, full_instance, t, size):
    airset = mini if size == "miniature" else full
    traces, params, _ = mini_instances["mixed"] if size == "miniature" else full_instance
    blob = airset.blob()
    pt = table_params(airset, params, t)
    n = traces[t].shape[1]
    assert oracle.check_constraints(blob, t, traces[t], pt or None) == -1          # the unchanged table has no failing row
    flagged = 0
    for seed in TABLE_SEEDS.get(t, SEEDS):
        bad, c, r = corrupt(traces, t, seed)
        want = expected_air(airset, t, bad[t], params, None if n <= 256 else (r - 1, r))
        flagged += bool(want)
        got = be.check_constraints(airset, bad, params, tables=[t])
        print("table %d (%s, %s) seed %d: cell (%d, %d): %d failing emits" % (t, airset.tables[t].name, size, seed, c, r, len(want)))
        assert strip(got, "AIR") == want, (seed, c, r)
        assert all(d["table_name"] == airset.tables[t].name for d in got)
        first = oracle.check_constraints(blob, t, bad[t], pt or None)
        assert first == (min(d["first_row"] for d in want) if want else -1)
        assert (min(d["first_row"] for d in got if d["section"] == "AIR") if want else -1) == first
    assert flagged >= 1, "no seed of this table breaks a constraint: choose other seeds"


def test_next_cells_from_the_neighbouring_lane_give_the_same_report(be, mini, mini_instances, monkeypatch):
    """OLA_CHECK_NEXT=neighbour: the kernel instantiation that takes a `next` cell from the neighbouring lane (the measured
    alternative of DESIGN.md) reports what the evaluator says too, on tables shorter and longer than a wavefront."""
    traces, params, _ = mini_instances["mixed"]
    bad, _, _ = corrupt(traces, 0, 1)            # cpu, 32 rows
    bad, _, _ = corrupt(bad, 2, 0)               # bitwise, 64 rows
    bad, _, _ = corrupt(bad, 10, 0)              # program
    want = [d for t in range(12) for d in expected_air(mini, t, bad[t], params)]
    assert len({d["table"] for d in want}) == 3
    monkeypatch.setenv("OLA_CHECK_NEXT", "neighbour")
    assert strip(be.check_constraints(mini, bad, params), "AIR") == want
    assert be.check_constraints(mini, traces, params) == []
    monkeypatch.delenv("OLA_CHECK_NEXT")
    assert strip(be.check_constraints(mini, bad, params), "AIR") == want


# ------------------------------------------------------------------------------------------------ 3. the reference generators' two quirks
def test_reference_quirks_are_named(be, oracle, mini, full):
    """generation/builtin.rs:66,71,76 drops the fourth limb of a bitwise operand, generation/memory.rs:95-153 writes a memory table
    without cells whose last row does not wrap around to row 0: `reference_quirks` reproduces both, the check names the emits.
    The fixture records the line a `yield_constr.constraint(` statement STARTS on: the two un-gated wrap-around constraints the
    documents cite as memory_stark.rs:265-270 start on lines 263 and 266 (and end on 265 and 268)."""
    from olavm_amd.air import miniexec as M
    fixture = json.load(open(os.path.join(HERE, "golden", "air_emit_kinds.json")))["tables"]
    sites = {d["table"]: d["emit_sites"] for d in fixture}
    cells = {d["table"]: d["emit_direct_cells"] for d in fixture}
    names = [t.name for t in full.tables]
    tb, tm = names.index("bitwise"), names.index("memory")
    # bitwise: "operand = sum of limbs" (bitwise_stark.rs:62,68,74), first at the first live row whose operand needs the fourth limb
    prog = M.wide_program()
    # (a fixed compress challenge: derived from the table as the generator does, it would differ between the two modes and with it every row)
    traces, params, _ = M.instance(prog, range_bits=16, limb_bits=8, bitwise_beta=12345, reference_quirks=True)
    clean, cparams, _ = M.instance(prog, range_bits=16, limb_bits=8, bitwise_beta=12345)
    assert be.check_constraints(full, clean, cparams) == []                     # the default mode reports nothing
    assert oracle.check_constraints(full.blob(), tb, clean[tb], table_params(full, cparams, tb)) == -1
    assert list(params) == list(cparams) and all(np.array_equal(traces[t], clean[t]) for t in range(12) if t != tb)
    changed = np.nonzero((traces[tb] != clean[tb]).any(axis=0))[0]
    assert len(changed)
    want_b = expected_air(full, tb, traces[tb], params, {int(r) + d for r in changed for d in (-1, 0)})
    got = be.check_constraints(full, traces, params)
    assert want_b and strip(got, "AIR") == want_b
    assert sorted(sites["Bitwise"][d["index"]] for d in want_b) == ["builtins/bitwise/bitwise_stark.rs:%d" % k for k in (62, 68, 74)]
    for d in want_b:
        (cell,) = cells["Bitwise"][d["index"]]
        wide = np.nonzero(traces[tb][int(cell[1:])] >= (1 << 24))[0]
        assert d["first_row"] == int(wide[0]) and d["rows_failing"] == len(wide)
    # memory: a run without memory cells gives the no-row table
    traces, params, _ = M.instance(M.fibonacci(5), reference_quirks=True)
    clean, cparams, _ = M.instance(M.fibonacci(5))
    assert be.check_constraints(mini, clean, cparams) == []
    n = traces[tm].shape[1]
    want_m = expected_air(mini, tm, traces[tm], params)
    got = be.check_constraints(mini, traces, params)
    assert strip(got, "AIR") == want_m
    wrap = [d for d in want_m if d["first_row"] == n - 1]
    assert [sites["Memory"][d["index"]] for d in wrap] == ["memory/memory_stark.rs:263", "memory/memory_stark.rs:266"]
    assert all(d["rows_failing"] == 1 and d["kind"] == "constraint" for d in wrap)
    assert oracle.check_constraints(mini.blob(), tm, traces[tm], None) == min(d["first_row"] for d in want_m)


# ------------------------------------------------------------------------------------------------ 4. PERMUTATION
def test_permuted_lookup_column_changed(be, mini, mini_instances):
    traces, params, _ = mini_instances["mixed"]
    names = [t.name for t in mini.tables]
    t = names.index("rangecheck")
    tab = mini.tables[t]
    pair = tab.permutation_pairs[1]
    tr = traces[t].copy()
    col = pair[0][1]                                              # the permuted side
    vals = sorted({int(x) for x in tr[col]})
    assert len(vals) >= 2
    r = 5
    tr[col, r] = next(v for v in vals if v != int(tr[col, r]))   # another in-range value
    bad = list(traces)
    bad[t] = tr
    batches = expected_permutation_batches(tab, tr)
    assert batches and expected_permutation_batches(tab, traces[t]) == []
    got = be.check_constraints(mini, bad, params, tables=[t])
    assert [d["index"] for d in got if d["section"] == "PERMUTATION"] == batches
    assert all(d["first_row"] == tr.shape[1] - 1 and d["rows_failing"] == 1 for d in got if d["section"] == "PERMUTATION")
    assert strip(got, "AIR") == expected_air(mini, t, tr, params)             # the emits of eval_lookups (lookup.rs:13-34)
    # a lookup is only checked when all of its tables are: none here
    assert [d for d in got if d["section"] == "LOOKUP"] == []


# ------------------------------------------------------------------------------------------------ 5. LOOKUP
def test_dropped_looked_row_is_reported_for_both_challenges(be, mini, mini_instances):
    traces, params, _ = mini_instances["mixed"]
    assert expected_lookups(mini, traces) == []
    found = None
    for li, ctl in enumerate(mini.ctls):
        f = ctl.looked_table.filter_column
        if f is None or len(f.terms) != 1 or f.terms[0][1] != 1 or f.constant != 0:
            continue
        t, c = ctl.looked_table.table, f.terms[0][0]
        rows = np.nonzero(traces[t][c] == 1)[0]
        if not len(rows):
            continue
        bad = list(traces)
        bad[t] = traces[t].copy()
        bad[t][c, int(rows[0])] = 0
        want = expected_lookups(mini, bad)
        if {d["index"] for d in want} == {li}:
            found = (li, bad, want)
            break
    assert found, "no lookup whose looked filter can be dropped alone"
    li, bad, want = found
    assert len(want) == 2 and want[0]["first_row"] - want[0]["rows_failing"] == 1
    got = be.check_constraints(mini, bad, params)
    assert strip(got, "LOOKUP") == want
    for d in got:
        if d["section"] == "LOOKUP":
            assert (d["looking_rows"], d["looked_rows"]) == (d["first_row"], d["rows_failing"])
    for t in range(12):
        assert strip(got, "AIR", t) == expected_air(mini, t, bad[t], params)
    # supplied challenges: the same lookups
    assert strip(be.check_constraints(mini, bad, params, ctl_challenges=SUPPLIED), "LOOKUP") == want


# ------------------------------------------------------------------------------------------------ 6. input forms
def test_every_input_form_gives_the_same_report(be, mini, mini_instances):
    import torch
    from olavm_amd.backend import Backend
    traces, params, _ = mini_instances["mixed"]
    bad, _, _ = corrupt(traces, 0, 0)
    bad, _, _ = corrupt(bad, 2, 1)
    bad, _, _ = corrupt(bad, 4, 0)
    base = be.check_constraints(mini, bad, params)
    assert base and strip(base, "AIR", 0) == expected_air(mini, 0, bad[0], params)
    # non-canonical words: p added to a seeded third of the words below 2^32 - 1
    rng = np.random.default_rng(6)
    shifted = []
    for tr in bad:
        tr = tr.copy()
        pick = (tr < (1 << 32) - 1) & (rng.integers(0, 3, size=tr.shape) == 0)
        tr[pick] += np.uint64(P)
        shifted.append(tr)
    assert any((tr >= np.uint64(P)).any() for tr in shifted)
    assert be.check_constraints(mini, shifted, params) == base
    # device-resident tables
    dev = [torch.from_numpy(tr.view(np.int64)).to("cuda:0").contiguous() for tr in bad]
    torch.cuda.synchronize()
    assert be.check_constraints(mini, dev, params) == base
    # separately allocated columns
    cols = [[np.ascontiguousarray(tr[c]).copy() for c in range(tr.shape[0])] for tr in shifted]
    assert be.check_constraints(mini, cols, params) == base
    # a context of two logical ranks on this GPU: the check runs on its first device
    two = Backend(devices=[0, 0])
    try:
        assert two.check_constraints(mini, bad, params) == base
    finally:
        two.close()


# ------------------------------------------------------------------------------------------------ 7. cap smaller than the report
def test_cap_smaller_than_the_number_of_entries(be, mini, mini_instances):
    traces, params, _ = mini_instances["mixed"]
    rng = np.random.default_rng(7)
    bad = [rng.integers(0, P, size=tr.shape, dtype=np.uint64) if t in (3, 8) else tr for t, tr in enumerate(traces)]   # cmp and tape: random rows
    blob = mini.blob()
    everything, total = be.check_constraints_raw(blob, bad, params, cap=4096)
    assert total == len(everything) > 6
    assert everything == sorted(everything, key=lambda e: e[:4])
    for cap in (0, 1, 5, total - 1, total):
        got, n = be.check_constraints_raw(blob, bad, params, cap=cap)
        assert n == total and got == everything[:cap], cap


# ------------------------------------------------------------------------------------------------ 8. a large table
def test_one_cell_of_a_2p20_row_cpu_table(be, oracle, mini):
    from olavm_amd.air import fastexec, miniexec as M
    traces, params, _ = fastexec.instance(M.fibonacci(150000), max_steps=1 << 21)
    cpu = traces[0]
    n = cpu.shape[1]
    assert cpu.shape == (94, 1 << 20)
    only = [cpu] + [None] * 11
    assert be.check_constraints(mini, only, params, tables=[0]) == []
    assert oracle.check_constraints(mini.blob(), 0, cpu, None) == -1
    flagged = 0
    for seed in SEEDS:
        rng = np.random.default_rng(80 + seed)
        c, r = int(rng.integers(0, 94)), int(rng.integers(n // 2, n))
        bad = cpu.copy()
        bad[c, r] ^= np.uint64(1)
        want = expected_air(mini, 0, bad, params, (r - 1, r))
        flagged += bool(want)
        got = be.check_constraints(mini, [bad] + [None] * 11, params, tables=[0])
        print("2^20-row cpu table, cell (%d, %d): %d failing emits" % (c, r, len(want)))
        assert strip(got) == want
        for d in got:
            assert d["first_row"] in (r - 1, r) and d["rows_failing"] <= 2
    assert flagged >= 1


# ------------------------------------------------------------------------------------------------ 9. no side effects
def test_a_failing_check_leaves_the_context_proving_the_committed_bytes(full, full_instance):
    from olavm_amd.backend import Backend
    traces, params, compress = full_instance
    raw = open(os.path.join(HERE, "golden", "ref_verified", "wide_program.proof"), "rb").read()
    b = Backend(device=0)
    try:
        bad, _, _ = corrupt(traces, 0, 0)
        before = b.upload_stats()
        assert b.check_constraints(full, bad, params) != []
        assert b.upload_stats() == before
        assert bytes(b.prove_with_traces(full.blob(), traces, params, compress)) == raw
        assert b.check_constraints(full, bad, params) != []
        assert bytes(b.prove_with_traces(full.blob(), traces, params, compress)) == raw
    finally:
        b.close()
