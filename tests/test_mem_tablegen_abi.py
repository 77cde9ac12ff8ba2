"""CPU-side checks of ola_generate_memory_trace / ola_generate_cmp_trace (include/ola_gpu.h) and of the cells the native trace generator
hands out (OLA_TRACEGEN_CELLS_ONLY, include/ola_tracegen.h): the symbols are exported and declared -- header, olavm_amd/backend.py,
include/ola_host.hpp, integration/rust/ola_gpu_sys.rs -- with the same shapes and constants, the kernels' column header is the table
description and miniexec's op order, sizing calls need no context, arguments are validated before anything touches a device, a call that
would do work says that there is no device, and a cells-only run of the generator returns the cells, operands and values of the Python
executor next to the nine tables of the ordinary run (also under AddressSanitizer / UBSan, stand-alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_tablegen_abi import _header_args, _rust_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
ARGS = {"ola_generate_memory_trace": ["ctx", "cells", "n_cells", "flags", "out", "log_n_out", "rc_out", "rc_counts"],
        "ola_generate_cmp_trace": ["ctx", "ops", "n_ops", "out", "log_n_out", "abs_diff_out"]}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def next_pow2(n):
    return 2 if n < 2 else 1 << (n - 1).bit_length()


def test_symbols_are_exported_and_declared_with_equal_shapes(lib):
    from olavm_amd import backend as B
    host = open(os.path.join(ROOT, "include", "ola_host.hpp")).read()
    for name, args in ARGS.items():
        assert name in B.EXPORTS
        f = getattr(lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None
        h, r = _header_args(name), _rust_args(name)
        assert len(h) == len(r) == len(f.argtypes) == len(args), (name, h, r)
        assert [a.split()[-1].lstrip("*").split("[")[0] for a in h] == [a.split(":")[0] for a in r] == args, name
        assert hasattr(B.Backend, name[len("ola_"):])
        calls = re.findall(r"\b%s\((.*?)\)\);" % name, host, flags=re.S)
        assert calls and all(len(c.split(",")) == len(args) for c in calls), name             # ola_host.hpp passes every argument
    assert _header_args("ola_generate_memory_trace") == ["OlaCtx* ctx", "const uint64_t* cells", "size_t n_cells", "uint32_t flags", "uint64_t* out",
                                                         "uint32_t* log_n_out", "uint64_t* rc_out", "uint64_t rc_counts[2]"]
    assert _header_args("ola_generate_cmp_trace") == ["OlaCtx* ctx", "const uint64_t* ops", "size_t n_ops", "uint64_t* out", "uint32_t* log_n_out",
                                                      "uint64_t* abs_diff_out"]
    assert lib.ola_gpu_abi_version(None, None) == 7          # additions that change no struct keep the revision


def test_cell_width_ops_and_flags_agree_everywhere():
    from olavm_amd import backend as B
    from olavm_amd.air import dump, fastexec, miniexec as M, ola_tables as T
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    words = int(re.search(r"#define OLA_MEM_CELL_WORDS (\d+)", hdr).group(1))
    assert words == B.OLA_MEM_CELL_WORDS == dump.MEM_CELL_WORDS == fastexec.MEM_CELL_WORDS == 5
    assert "pub const OLA_MEM_CELL_WORDS: usize = %d;" % words in rs
    tg = open(os.path.join(ROOT, "include", "ola_tracegen.h")).read()
    assert "#define OLA_TRACEGEN_CELLS_ONLY 16u" in tg and fastexec.OLA_TRACEGEN_CELLS_ONLY == 16
    assert "#define OLA_TRACEGEN_STEPS_ONLY 8u" in tg and fastexec.OLA_TRACEGEN_STEPS_ONLY == 8
    # the ranks are the order sorted(cells) gives cells that share (address, clock): alphabetical by op name
    cells = [(5, 9, op, 0, 0) for op in reversed(dump.MEM_OPS)]
    assert [c[2] for c in sorted(cells)] == list(dump.MEM_OPS) and len(dump.MEM_OPS) == 9
    t, _, _ = M.memory_trace(cells)                              # every one of them is an op memory_trace knows
    assert t[T.COL_MEM_OP, :9].tolist() == [T.op_mask(op) for op in dump.MEM_OPS]


def test_column_header_of_the_kernels_is_the_table_description():
    from olavm_amd.air import dump, ola_tables as T
    text = open(os.path.join(ROOT, dump.TABLEGEN_MEM_COLUMNS_H)).read()
    assert text == dump.tablegen_mem_columns_header()
    assert "constexpr uint32_t COL_MEM_FILTER_LOOKING_RC_COND = %du;" % T.COL_MEM_FILTER_LOOKING_RC_COND in text
    assert "constexpr uint32_t COL_CMP_ABS_DIFF_INV = %du;" % T.COL_CMP_ABS_DIFF_INV in text
    assert "constexpr uint64_t ADDR_HEAP_PTR = %dull;" % T.ADDR_HEAP_PTR in text
    for rank, op in enumerate(dump.MEM_OPS):
        assert "constexpr uint64_t MEM_OP_MASK_%s = %dull; constexpr uint32_t MEM_OP_RANK_%s = %du;" % (op, T.op_mask(op), op, rank) in text
    mem = sorted(int(v) for v in re.findall(r"constexpr uint32_t COL_MEM_\w+ = (\d+)u;", text))
    cmp_ = sorted(int(v) for v in re.findall(r"constexpr uint32_t COL_CMP_\w+ = (\d+)u;", text))
    assert mem == list(range(T.NUM_MEM_COLS)) and cmp_ == list(range(T.COL_NUM_CMP))          # every column of both tables, once
    src = open(os.path.join(ROOT, "olavm_amd", "csrc", "tablegen.hip")).read()
    assert '#include "tablegen_mem_columns.h"' in src
    gen = src[src.index("mem_op_key"):src.index("u32 log2_rows")]
    assert not re.search(r"\bout \+ \(size_t\)\d+ \* n|\bout\[\(size_t\)\d+ \* n|put\(\d", gen), "a column index was typed in"


def test_sizing_calls_need_no_context(lib):
    counts = (C.c_uint64 * 2)(77, 78)
    log_n = C.c_uint32(99)
    for n_cells in (0, 1, 6, 7, 8, (1 << 16) - 1, 1 << 16):
        for flags in (0, 1):
            assert lib.ola_generate_memory_trace(None, None, n_cells, flags, None, C.byref(log_n), None, counts) == 0
            assert 1 << log_n.value == next_pow2(max(n_cells + 1, 8)), n_cells
    assert list(counts) == [77, 78]
    for n_ops in (0, 1, 2, 3):
        assert lib.ola_generate_cmp_trace(None, None, n_ops, None, C.byref(log_n), None) == 0
        assert 1 << log_n.value == max(2, next_pow2(n_ops)), n_ops


def test_arguments_are_validated_first(lib):
    cells = np.zeros(5 * 3, dtype=np.uint64)
    ops = np.zeros(2 * 3, dtype=np.uint64)
    out = np.full(29 * 8, 7, dtype=np.uint64)
    rc = np.full(6, 7, dtype=np.uint64)
    counts = (C.c_uint64 * 2)(77, 78)
    log_n = C.c_uint32(99)
    c, p, o, r = (C.c_void_p(a.ctypes.data) for a in (cells, ops, out, rc))
    bad = [
        lambda: lib.ola_generate_memory_trace(None, c, 3, 0, o, C.byref(log_n), r, None),               # nowhere to put the counts
        lambda: lib.ola_generate_memory_trace(None, None, 3, 0, None, C.byref(log_n), None, None),      # ... in a sizing call either
        lambda: lib.ola_generate_memory_trace(None, c, 3, 0, o, None, r, counts),
        lambda: lib.ola_generate_memory_trace(None, c, 1 << 31, 0, o, C.byref(log_n), r, counts),       # indices stay in 32 bits
        lambda: lib.ola_generate_memory_trace(None, None, 1 << 31, 0, None, C.byref(log_n), None, counts),
        lambda: lib.ola_generate_memory_trace(None, c, 3, 2, o, C.byref(log_n), r, counts),             # a flag nobody defined
        lambda: lib.ola_generate_memory_trace(None, None, 3, 0, o, C.byref(log_n), r, counts),          # cells without records
        lambda: lib.ola_generate_cmp_trace(None, p, 3, o, None, r),
        lambda: lib.ola_generate_cmp_trace(None, p, 1 << 31, o, C.byref(log_n), r),
        lambda: lib.ola_generate_cmp_trace(None, None, 3, o, C.byref(log_n), r),
    ]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in lib.ola_gpu_last_error()
    assert np.all(out == 7) and np.all(rc == 7) and list(counts) == [77, 78]


def test_a_working_call_without_a_context_answers_as_the_header_says(lib):
    """OLA_E_NO_DEVICE on a machine without a HIP device (there is no CPU fallback), OLA_E_INVALID_ARG where there is one"""
    import torch
    want, text = (OLA_E_INVALID_ARG, b"ctx is NULL") if torch.cuda.is_available() else (OLA_E_NO_DEVICE, b"no HIP device")
    cells = np.zeros(5 * 3, dtype=np.uint64)
    ops = np.zeros(2 * 3, dtype=np.uint64)
    out = np.full(29 * 8, 7, dtype=np.uint64)
    rc = np.full(6, 7, dtype=np.uint64)
    counts = (C.c_uint64 * 2)(77, 78)
    log_n = C.c_uint32()
    c, p, o, r = (C.c_void_p(a.ctypes.data) for a in (cells, ops, out, rc))
    for rcode in (lib.ola_generate_memory_trace(None, c, 3, 0, o, C.byref(log_n), r, counts),
                  lib.ola_generate_memory_trace(None, None, 0, 1, o, C.byref(log_n), None, counts),
                  lib.ola_generate_cmp_trace(None, p, 3, o, C.byref(log_n), r),
                  lib.ola_generate_cmp_trace(None, None, 0, o, C.byref(log_n), None)):
        assert rcode == want and text in lib.ola_gpu_last_error()
    assert np.all(out == 7) and np.all(rc == 7) and list(counts) == [77, 78]


@pytest.mark.parametrize("name", ["fibonacci", "mixed", "memory", "hash", "call", "tape", "storage", "heap", "storage_heavy"])
def test_cells_only_run_of_the_native_generator(lib, name):
    from olavm_amd.air import fastexec as F, miniexec as M, ola_tables as T
    make, kw = M.EXAMPLES[name]
    prog = make()
    tree = M.StorageTree()
    if kw.get("prove_program_hash"):
        listing = prog.words()[0]
        tree.set(prog.code_addr, M.program_hash(listing + [0] * (-len(listing) % 8)))
    _, side, _ = M.execute(prog, tree=tree)
    traces, params, compress = F.instance(prog, **kw)
    lean, lean_params, lean_compress, rec = F.instance(prog, cells_only=True, **kw)
    left_out = (T.CPU, T.PROGRAM, T.MEMORY, T.CMP, T.RANGECHECK)
    cells = [(a, c, T.op_mask(op), v, w) for a, c, op, v, w in side["mem"]]
    assert rec["cells"].shape == (5, len(cells)) and rec["cells"].T.tolist() == [list(c) for c in cells]
    assert rec["cmp_ops"].shape == (2, len(side["cmp"])) and rec["cmp_ops"].T.tolist() == [list(c) for c in side["cmp"]]
    assert rec["cpu_rc"].tolist() == list(side["rc"])
    for t in range(12):
        if t in left_out:
            assert lean[t] is None
        else:
            assert np.array_equal(lean[t], traces[t]), t                                        # the other nine, word for word
    assert [rec[k] for k in ("cpu_log_n", "prog_log_n", "mem_log_n", "cmp_log_n", "rc_log_n")] == [traces[t].shape[1].bit_length() - 1 for t in left_out]
    assert lean_params == params and lean_compress == compress
    # OLA_TRACEGEN_STEPS_ONLY by itself gives what it gave: two tables left out, the records and the listing of the cells-only run
    steps, _, _, srec = F.instance(prog, steps_only=True, **kw)
    assert set(srec) == {"steps", "cpu_log_n", "listing", "prog_log_n"}
    assert np.array_equal(srec["steps"], rec["steps"]) and np.array_equal(srec["listing"], rec["listing"])
    for t in range(12):
        assert (steps[t] is None) if t in (T.CPU, T.PROGRAM) else np.array_equal(steps[t], traces[t]), t
    # without the flag the accessors answer with an error
    L = F.load_library()
    code, stor, handle = (C.c_uint64 * 4)(*prog.code_addr), (C.c_uint64 * 4)(*prog.storage_addr), C.c_void_p()
    assert L.ola_tracegen_run(F.encode(prog), len(prog.ins), code, stor, 4, 2, 0, 0, 1 << 16, F.OLA_TRACEGEN_STEPS_ONLY, C.byref(handle)) == 0
    n, data = C.c_uint64(), C.POINTER(C.c_uint64)()
    for get in (L.ola_tracegen_mem_cells, L.ola_tracegen_cmp_ops, L.ola_tracegen_cpu_rc_values):
        assert get(handle, C.byref(n), C.byref(data)) == -1 and b"CELLS_ONLY" in L.ola_tracegen_last_error()
    L.ola_tracegen_free(handle)


def test_the_restated_rules_give_memory_trace():
    """tests/mem_cells_rules.py, which the GPU tests use for op words memory_trace has no name for: on named ops both of its ways give
    miniexec.memory_trace, and an op word without a name ranks behind the nine, by word, without a selector"""
    from olavm_amd.air import miniexec as M, ola_tables as T
    from tests import mem_cells_rules as R
    sets = dict(R.hand_made(), pattern=R.pattern(5), side=M.execute(M.hash_program())[1]["mem"])
    assert len(sets["side"]) > 20
    for name, cells in sets.items():
        want = M.memory_trace(cells)
        for patch in (False, True):
            got = R.table(R.words(cells[::-1]), patch=patch)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (name, patch)
    t, rc, cond = R.table(R.ties())
    live = t[:, :R.ties().shape[1]]
    at = lambda addr, clk: [(int(o), int(v), int(w)) for a, c, o, v, w in live[[T.COL_MEM_ADDR, T.COL_MEM_CLK, T.COL_MEM_OP, T.COL_MEM_VALUE, T.COL_MEM_IS_WRITE]].T
                            if (a, c) == (addr, clk)]
    m = T.op_mask
    assert at(50, 7) == [(m("CALL"), 9, 1), (m("MLOAD"), 2, 0), (m("POSEIDON"), 5, 0), (m("RET"), 5, 0), (m("TSTORE"), 1, 0)]
    assert at(50, 8) == [(m("POSEIDON"), 3, 1), (m("POSEIDON"), 4, 0), (m("POSEIDON"), 9, 0)]
    assert at(51, 8) == [(m("SLOAD"), 6, 0), (m("SLOAD"), 6, 1), (m("SLOAD"), 6, 1)]
    assert at(52, 1) == [(m("CALL"), 7, 0), (m("TSTORE"), 8, 0), (0, 1, 0), (3, 9, 0), (m("ADD"), 0, 0), (m("ADD"), 0, 1), (R.P - 1, 0, 0)]
    nameless = np.isin(live[T.COL_MEM_OP], [0, 3, m("ADD"), R.P - 1])
    assert nameless.sum() == 5 and not live[T.COL_MEM_S_MLOAD:T.COL_MEM_S_PROPHET + 1][:, nameless].any()
    assert (live[T.COL_MEM_S_MLOAD:T.COL_MEM_S_PROPHET + 1][:, ~nameless].sum(axis=0) == 1).all()


def test_cells_only_generator_is_clean_under_the_sanitizers(lib, tmp_path):
    """a stand-alone host program over tracegen.cpp, with and without OLA_TRACEGEN_CELLS_ONLY"""
    exe = str(tmp_path / "host_tracegen_cells")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host_tracegen_cells.cpp"), os.path.join(ROOT, "olavm_amd", "csrc", "host", "tracegen.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
