"""ola_check_lookup on the GPU: which tuples a cross-table lookup is missing.

What the report must say comes from `reference` below, which shares nothing with the code under test: the filter-selected rows of
every looking entry and of the looked table, their data columns evaluated with Python integers mod p (`col_eval`, the arithmetic of
`lookup_sides` in tests/test_gpu_check_constraints.py), counted in two `Counter`s; the first carrier of a tuple is the first one met
when the entries are walked in order and their rows in order.  Every comparison is for equality: the answer is exact."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from olavm_amd.air import ola_tables as T
from olavm_amd.air.dsl import AirSet, AirTable, Col, CrossTableLookup, P, TableWithColumns

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROGRAMS = ["fibonacci", "mixed", "memory", "hash", "call", "tape", "storage", "heap", "storage_heavy"]
KEYS = ("values", "looking_count", "looked_count", "looking_entry", "looking_table", "looking_row", "looked_row")


# ------------------------------------------------------------------------------------------------ the independent evaluator
def col_eval(col, trace, i):
    return (sum(int(trace[c, i]) % P * f for c, f in col.terms) + col.constant) % P


def selected(twc, tr):
    """rows of `tr` the side selects: filter == 1 (canonical), every row without a filter"""
    f = twc.filter_column
    if f is None:
        return range(tr.shape[1])
    if len(f.terms) == 1 and f.terms[0][1] == 1 and f.constant == 0:          # one column: the same comparison, all rows at once
        return [int(i) for i in np.nonzero(tr[f.terms[0][0]] % np.uint64(P) == 1)[0]]
    return [i for i in range(tr.shape[1]) if col_eval(f, tr, i) == 1]


def reference(airset, traces, li):
    """-> {"width", "totals", "mismatches"} as Backend.check_lookup reports them (KEYS of every mismatch)"""
    ctl = airset.ctls[li]

    def side(twcs):
        count, first, rows = Counter(), {}, 0
        for e, twc in enumerate(twcs):
            tr = np.asarray(traces[twc.table])
            cache = {}

            def cell(c, i):
                if c not in cache:
                    cache[c] = (tr[c] % np.uint64(P)).tolist()
                return cache[c][i]
            for i in selected(twc, tr):
                v = tuple((sum(cell(c, i) * f for c, f in col.terms) + col.constant) % P for col in twc.columns)
                count[v] += 1
                first.setdefault(v, (e, twc.table, i))
                rows += 1
        return count, first, rows

    looking, first_lk, n_lk = side(ctl.looking_tables)
    looked, first_ld, n_ld = side([ctl.looked_table])
    mism = []
    for v in sorted(set(looking) | set(looked)):
        if looking[v] != looked[v]:
            e, t, r = first_lk.get(v, (None, None, None))
            mism.append({"values": v, "looking_count": looking[v], "looked_count": looked[v], "looking_entry": e, "looking_table": t,
                         "looking_row": r, "looked_row": first_ld.get(v, (None, None, None))[2]})
    return {"width": len(ctl.looked_table.columns),
            "totals": [n_lk, n_ld, len(mism), sum(abs(m["looking_count"] - m["looked_count"]) for m in mism)], "mismatches": mism}


def strip(rep):
    return {"width": rep["width"], "totals": list(rep["totals"]), "mismatches": [{k: m[k] for k in KEYS} for m in rep["mismatches"]]}


def agree(be, airset, traces, li, what=""):
    """the library's report of lookup li == the evaluator's; -> the report"""
    want = reference(airset, traces, li)
    got = strip(be.check_lookup(airset, traces, li))
    print("%s lookup %d: width %d, totals %s" % (what, li, want["width"], want["totals"]))
    assert got == want, (what, li)
    return want


def set_filter(tr, twc, row, want):
    """make the side select (want) / not select row `row` by changing one cell of a filter column, in place"""
    f = twc.filter_column
    if f is None:
        return False
    for c, _ in f.terms:
        old = tr[c, row]
        for v in (0, 1):
            tr[c, row] = v
            if (col_eval(f, tr, row) == 1) == want:
                return True
        tr[c, row] = old
    return False


def with_table(traces, t, tr):
    out = list(traces)
    out[t] = tr
    return out


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
def mini_instances():
    from olavm_amd.air import miniexec as M
    from tests import tracegen
    inst = {}
    for name in PROGRAMS:
        factory, kwargs = M.EXAMPLES[name]
        inst[name] = M.instance(factory(), **kwargs)[0]
    inst["padding"] = tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(3))[0]
    return inst


@pytest.fixture(scope="module")
def full_instance():
    from tests.make_ref_verdict import instance
    return instance()


def executed(count):
    """memory_program(count) executed, with the reference's range-check width and a miniature bitwise table -> (AIR set, traces)"""
    from olavm_amd.air import fastexec, miniexec as M
    traces = fastexec.instance(M.memory_program(count), range_bits=16, limb_bits=2, max_steps=1 << 20)[0]
    return T.ola_stark(range_bits=16, limb_bits=2), traces


def synthetic(width, n_looking, n_looked, seed, looking_filter="column", looked_filter="column", spread=3):
    """Two tables without constraints and one lookup of `width` data columns between them: table 0 looks (two entries, the second
    with linear combinations), table 1 is looked.  Cells are drawn from `spread` values per column, so tuples repeat; some words
    are field-sized.  Column 0 of either table is the filter column ("column"), or the side has no filter ("none")."""
    rng = np.random.default_rng(seed)
    pool = np.array([5, P - 1, 1 << 32, 0, 1, (1 << 32) - 1, P - 2, 12345678901234567], dtype=np.uint64)
    a = pool[rng.integers(0, spread, size=(width + 2, n_looking))]
    b = pool[rng.integers(0, spread, size=(width + 1, n_looked))]
    a[0] = rng.integers(0, 2, size=n_looking)
    a[width + 1] = rng.integers(0, 3, size=n_looking)                         # a second filter column with a non-binary value
    b[0] = rng.integers(0, 2, size=n_looked)
    plain = [Col.single(1 + k) for k in range(width)]
    # the same tuple written as linear combinations: 2 c - c in the odd positions
    combos = [Col.linear_combination([(1 + k, 2), (1 + k, P - 1)]) if k % 2 else Col.linear_combination([(1 + k, 1)], 0) for k in range(width)]
    f0 = None if looking_filter == "none" else Col.single(0)
    f1 = None if looked_filter == "none" else Col.single(0)
    ctl = CrossTableLookup([TableWithColumns(0, plain, f0), TableWithColumns(0, combos, Col.single(width + 1))], TableWithColumns(1, plain, f1))
    return AirSet([AirTable("looking", width + 2, 3), AirTable("looked", width + 1, 3)], [ctl]), [a, b]


# ------------------------------------------------------------------------------------------------ 1. valid traces
def test_valid_traces_report_nothing(be, mini, mini_instances, full_instance):
    for name, traces in mini_instances.items():
        for li in range(len(mini.ctls)):
            want = agree(be, mini, traces, li, name)
            assert want["mismatches"] == [] and want["totals"][0] == want["totals"][1]
    full = T.ola_stark()
    traces = full_instance[0]
    for li in range(len(full.ctls)):
        got, n, totals, width = be.check_lookup_raw(full.blob(), traces, li)
        ctl = full.ctls[li]
        rows = [sum(len(selected(twc, traces[twc.table])) for twc in ctl.looking_tables), len(selected(ctl.looked_table, traces[ctl.looked_table.table]))]
        assert (got, n, totals, width) == ([], 0, rows + [0, 0], len(ctl.looked_table.columns)) and rows[0] == rows[1], li


# ------------------------------------------------------------------------------------------------ 2. single corruptions
def test_single_corruptions_entry_for_entry(be, mini, mini_instances):
    """For every lookup that selects rows in one of the miniature instances: one looked row dropped, one looking tuple duplicated into
    a filler row, and one data cell changed on the looking side -- the FIRST tuple word in one case, the LAST in another."""
    covered = Counter()
    for li, ctl in enumerate(mini.ctls):
        looked = ctl.looked_table
        for name, traces in mini_instances.items():
            if selected(looked, traces[looked.table]) and any(selected(twc, traces[twc.table]) for twc in ctl.looking_tables):
                break
        else:
            continue
        e, twc = next((e, twc) for e, twc in enumerate(ctl.looking_tables) if selected(twc, traces[twc.table]))
        rows = selected(twc, traces[twc.table])
        # drop one looked row
        tr = traces[looked.table].copy()
        r = selected(looked, tr)[-1]
        if set_filter(tr, looked, r, False):
            want = agree(be, mini, with_table(traces, looked.table, tr), li, "%s, looked row %d dropped:" % (name, r))
            if len({t.table for t in ctl.looking_tables} | {looked.table}) == len(ctl.looking_tables) + 1:    # no table on both sides, none twice
                assert len(want["mismatches"]) == 1 and want["totals"][2:] == [1, 1]
                m = want["mismatches"][0]
                assert m["looking_count"] == m["looked_count"] + 1
            covered["dropped"] += 1
        # duplicate one looking row's tuple into a filler row
        tr = traces[twc.table].copy()
        filler = [i for i in range(tr.shape[1]) if i not in set(rows)]
        if filler:
            for col in twc.columns:
                for c, _ in col.terms:
                    tr[c, filler[-1]] = tr[c, rows[0]]
            if set_filter(tr, twc, filler[-1], True):
                want = agree(be, mini, with_table(traces, twc.table, tr), li, "%s, looking row %d copied to %d:" % (name, rows[0], filler[-1]))
                assert want["mismatches"], li
                covered["duplicated"] += 1
        # change one data cell on the looking side: the first tuple word, the last tuple word
        for k in (0, len(twc.columns) - 1):
            col = twc.columns[k]
            if not col.terms:
                continue
            tr = traces[twc.table].copy()
            tr[col.terms[0][0], rows[0]] = (int(tr[col.terms[0][0], rows[0]]) + 3) % P
            want = agree(be, mini, with_table(traces, twc.table, tr), li, "%s, word %d of looking row %d changed:" % (name, k, rows[0]))
            assert want["mismatches"], li
            covered["first word" if k == 0 else "last word"] += 1
    print("corruptions checked:", dict(covered))
    assert min(covered[k] for k in ("dropped", "duplicated", "first word", "last word")) >= 8


# ------------------------------------------------------------------------------------------------ 3. several entries of one table
def test_a_row_of_the_second_looking_entry_is_named(be, mini, mini_instances):
    """CPU -> memory has store / load, call / ret (twice) and tape entries, all of the CPU table: a changed cell that only the second
    entry projects is reported with that entry's position."""
    traces = mini_instances["call"]
    ctl = mini.ctls[0]
    assert len(ctl.looking_tables) == 16 and {t.table for t in ctl.looking_tables} == {T.CPU}
    second = ctl.looking_tables[1]
    rows = selected(second, traces[T.CPU])
    assert rows
    c = second.columns[4].terms[0][0]                                        # COL_OP0: entry 1 projects it, entries 0 and 2 do not
    assert all(c not in [x for col in ctl.looking_tables[e].columns for x, _ in col.terms] for e in (0, 2))
    tr = traces[T.CPU].copy()
    tr[c, rows[-1]] = (int(tr[c, rows[-1]]) + 1) % P
    want = agree(be, mini, with_table(traces, T.CPU, tr), 0, "call, entry 1:")
    new = [m for m in want["mismatches"] if m["looked_count"] == 0]
    assert len(new) == 1 and (new[0]["looking_entry"], new[0]["looking_table"], new[0]["looking_row"]) == (1, T.CPU, rows[-1])
    assert len(want["mismatches"]) == 2


# ------------------------------------------------------------------------------------------------ 4. many mismatches, cap
def test_many_mismatches_and_a_small_cap(be):
    airset, traces = executed(1400)
    li = 0                                                                    # CPU -> memory: every tuple carries its clock
    looked = airset.ctls[li].looked_table
    assert traces[looked.table].shape[1] == 1 << 13
    tr = traces[looked.table].copy()
    for r in selected(looked, tr)[::2]:
        assert set_filter(tr, looked, r, False)
    bad = with_table(traces, looked.table, tr)
    want = agree(be, airset, bad, li, "every other looked row dropped:")
    assert want["totals"][2] > 256 and want["totals"][2] == len(want["mismatches"])
    assert want["totals"][0] % 64 and want["totals"][0] % 256                 # a selected-row count that is no multiple of a wave or a block
    got, n, totals, width = be.check_lookup_raw(airset.blob(), bad, li, cap=5)
    assert n == want["totals"][2] and totals == want["totals"] and width == want["width"]
    assert [dict(zip(("looking_count", "looked_count", "looking_entry", "looking_table", "looking_row", "looked_row", "values"), g)) for g in got] == \
        [{k: m[k] for k in KEYS} for m in want["mismatches"][:5]]
    got, n, totals, _ = be.check_lookup_raw(airset.blob(), bad, li, cap=0)
    assert got == [] and n == want["totals"][2] and totals == want["totals"]


# ------------------------------------------------------------------------------------------------ 5. compaction and run boundaries
@pytest.mark.parametrize("case", ["odd counts", "all rows", "none looked", "none looking", "one tuple", "widest", "two rows"])
def test_compaction_and_run_boundaries(be, case):
    kw = {"odd counts": dict(width=3, n_looking=1 << 10, n_looked=1 << 9, seed=1),
          "all rows": dict(width=2, n_looking=1 << 9, n_looked=1 << 10, seed=2, looking_filter="none", looked_filter="none"),
          "none looked": dict(width=2, n_looking=1 << 9, n_looked=1 << 8, seed=3),
          "none looking": dict(width=2, n_looking=1 << 8, n_looked=1 << 9, seed=4),
          "one tuple": dict(width=4, n_looking=1 << 11, n_looked=1 << 4, seed=5, looking_filter="none", spread=1),
          "widest": dict(width=24, n_looking=1 << 9, n_looked=1 << 9, seed=6, spread=2),
          "two rows": dict(width=1, n_looking=2, n_looked=2, seed=7, spread=8)}[case]
    airset, traces = synthetic(**kw)
    if case == "none looked":
        traces[1][0] = 0
    if case == "none looking":
        traces[0][0] = 0
        traces[0][kw["width"] + 1] = 2
    if case == "one tuple":
        traces[0][kw["width"] + 1] = 0                                          # the second entry selects nothing
        traces[1][0] = 0
    want = agree(be, airset, traces, 0, case + ":")
    n = traces[0].shape[1]
    if case == "odd counts":
        assert want["totals"][0] % 64 and want["totals"][1] % 64
    if case == "all rows":
        assert want["totals"][1] == traces[1].shape[1] and want["totals"][0] >= n
    if case == "none looked":
        assert want["totals"][1] == 0 and want["totals"][0] and all(m["looked_row"] is None for m in want["mismatches"])
    if case == "none looking":
        assert want["totals"][0] == 0 and want["totals"][1] and all(m["looking_entry"] is None for m in want["mismatches"])
    if case == "one tuple":
        assert len(want["mismatches"]) == 1 and want["mismatches"][0]["looking_count"] == n and want["totals"] == [n, 0, 1, n]
    if case == "widest":
        assert want["width"] == 24 and want["mismatches"]


def test_scan_and_sort_over_many_workgroups(be):
    """memory_program(3000): 2^16 CPU rows looking into a 2^17-row program table; one looked row dropped, one looking cell changed"""
    airset, traces = executed(3000)
    li = 16
    ctl = airset.ctls[li]
    assert traces[T.CPU].shape[1] == 1 << 16
    assert agree(be, airset, traces, li, "2^16 rows, valid:")["mismatches"] == []
    looked = ctl.looked_table
    tr = traces[looked.table].copy()
    r = selected(looked, tr)[1000]
    assert set_filter(tr, looked, r, False)
    cpu = traces[T.CPU].copy()
    c = ctl.looking_tables[0].columns[-1].terms[0][0]
    cpu[c, 40000] = (int(cpu[c, 40000]) + 1) % P
    want = agree(be, airset, with_table(with_table(traces, looked.table, tr), T.CPU, cpu), li, "2^16 rows, two corruptions:")
    assert 2 <= len(want["mismatches"]) <= 3 and want["totals"][0] > 1 << 16


# ------------------------------------------------------------------------------------------------ 6. input forms
def test_every_input_form_gives_the_same_report(be, mini, mini_instances):
    import torch
    from olavm_amd.backend import Backend
    traces = mini_instances["memory"]
    li = 0
    ctl = mini.ctls[li]
    tr = traces[T.CPU].copy()
    twc = ctl.looking_tables[0]
    r = selected(twc, tr)[0]
    tr[twc.columns[5].terms[0][0], r] = (int(tr[twc.columns[5].terms[0][0], r]) + 9) % P
    bad = with_table(traces, T.CPU, tr)
    want = agree(be, mini, bad, li, "memory, one cell:")
    assert want["mismatches"]
    named = {t.table for t in ctl.looking_tables} | {ctl.looked_table.table}
    # only the tables the lookup names
    only = [t if i in named else None for i, t in enumerate(bad)]
    assert strip(be.check_lookup(mini, only, li)) == want
    # non-canonical words: p added to a seeded third of the words below 2^32 - 1
    rng = np.random.default_rng(6)
    shifted = []
    for t in bad:
        t = t.copy()
        pick = (t < (1 << 32) - 1) & (rng.integers(0, 3, size=t.shape) == 0)
        t[pick] += np.uint64(P)
        shifted.append(t)
    assert any((t >= np.uint64(P)).any() for t in shifted)
    assert strip(be.check_lookup(mini, shifted, li)) == want
    # device-resident tables
    dev = [torch.from_numpy(t.view(np.int64)).to("cuda:0").contiguous() if i in named else None for i, t in enumerate(shifted)]
    torch.cuda.synchronize()
    assert strip(be.check_lookup(mini, dev, li)) == want
    # separately allocated columns
    cols = [[np.ascontiguousarray(t[c]).copy() for c in range(t.shape[0])] if i in named else None for i, t in enumerate(shifted)]
    assert strip(be.check_lookup(mini, cols, li)) == want
    # a context of two logical ranks on this GPU: the check runs on its first device
    two = Backend(devices=[0, 0])
    try:
        assert strip(two.check_lookup(mini, bad, li)) == want
    finally:
        two.close()
    # a lookup beyond the set
    from olavm_amd.backend import OlaGpuError
    with pytest.raises(OlaGpuError) as e:
        be.check_lookup_raw(mini.blob(), bad, len(mini.ctls))
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ 7. context state
def test_a_mismatching_call_leaves_the_context_proving_the_committed_bytes(full_instance):
    from olavm_amd.backend import Backend
    full = T.ola_stark()
    traces, params, compress = full_instance
    raw = open(os.path.join(HERE, "golden", "ref_verified", "wide_program.proof"), "rb").read()
    li = 3                                                                    # CPU -> bitwise
    looked = full.ctls[li].looked_table
    tr = traces[looked.table].copy()
    assert set_filter(tr, looked, selected(looked, tr)[0], False)
    bad = with_table(traces, looked.table, tr)
    b = Backend(device=0)
    try:
        before = b.upload_stats()
        assert b.check_lookup(full, bad, li)["totals"][2:] == [1, 1]
        assert b.upload_stats() == before
        assert bytes(b.prove_with_traces(full.blob(), traces, params, compress)) == raw
        assert b.check_lookup(full, bad, li)["totals"][2:] == [1, 1]
        assert bytes(b.prove_with_traces(full.blob(), traces, params, compress)) == raw
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ 8. host layer
def test_host_layer_prints_the_python_layers_report(be, mini, mini_instances, tmp_path):
    from olavm_amd.backend import format_lookup_report
    traces = mini_instances["mixed"]
    li = 16
    ctl = mini.ctls[li]
    looked = ctl.looked_table
    tr = traces[looked.table].copy()
    assert set_filter(tr, looked, selected(looked, tr)[2], False)
    cpu = traces[T.CPU].copy()
    cpu[ctl.looking_tables[0].columns[0].terms[0][0], selected(ctl.looking_tables[0], cpu)[1]] += np.uint64(1)
    bad = with_table(with_table(traces, looked.table, tr), T.CPU, cpu)
    rep = be.check_lookup(mini, bad, li)
    assert strip(rep) == reference(mini, bad, li) and len(rep["mismatches"]) >= 2
    blob = mini.blob()
    words = [blob.size] + [int(x) for x in blob] + [len(bad)]
    for t in bad:
        words += [int(t.shape[1]).bit_length() - 1, t.size] + [int(x) for x in np.ascontiguousarray(t).reshape(-1)]
    path = os.path.join(str(tmp_path), "instance.bin")
    np.array(words, dtype="<u8").tofile(path)
    exe = os.path.join(str(tmp_path), "host_check_lookup")
    lib = os.path.join(ROOT, "olavm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "host_check_lookup.cpp"), "-o", exe, "-L" + lib, "-lola_gpu", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([exe, path, str(li)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip("\n") == format_lookup_report(rep)
    r = subprocess.run([exe, path, str(li), "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip("\n") == format_lookup_report(be.check_lookup(mini, bad, li, max_tuples=1), max_tuples=1)
