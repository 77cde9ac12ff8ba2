"""CPU-side checks of ola_generate_tape_trace / ola_generate_poseidon_chunk_trace / ola_generate_prog_chunk_trace (include/ola_gpu.h): the
symbols are exported and declared -- header, olavm_amd/backend.py, include/ola_host.hpp, integration/rust/ola_gpu_sys.rs -- with the same
shapes and constants, the kernels' column header is the table description, sizing calls need no context, arguments are validated before
anything touches a device, and a call that would do work says that there is no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_tablegen_abi import _header_args, _rust_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
P = 0xFFFFFFFF00000001
ARGS = {"ola_generate_tape_trace": ["ctx", "cells", "n_cells", "out", "log_n_out"],
        "ola_generate_poseidon_chunk_trace": ["ctx", "calls", "n_calls", "poseidon_table", "psdn_log_n", "out", "log_n_out"],
        "ola_generate_prog_chunk_trace": ["ctx", "words", "n_words", "code_addr", "flags", "poseidon_table", "psdn_log_n", "out", "log_n_out"]}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def next_pow2(n):
    return 1 if n < 2 else 1 << (n - 1).bit_length()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def calls_of(lens, rows=None):
    """5 x n call records: clk, src, len, dst, psdn_row (the blocks back to back from row 0 unless `rows` says otherwise)"""
    at = np.cumsum([0] + [l // 8 for l in lens[:-1]]) if lens else []
    return np.array([[3 + i for i in range(len(lens))], [100 * i for i in range(len(lens))], lens, [9000 + i for i in range(len(lens))],
                     list(at) if rows is None else rows], dtype=np.uint64).reshape(5, -1)


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
        assert len(calls) == 2 and all(len(c.split(",")) == len(args) for c in calls), name       # the sizing call and the working call
    assert _header_args("ola_generate_tape_trace") == ["OlaCtx* ctx", "const uint64_t* cells", "size_t n_cells", "uint64_t* out", "uint32_t* log_n_out"]
    assert _header_args("ola_generate_poseidon_chunk_trace") == [
        "OlaCtx* ctx", "const uint64_t* calls", "size_t n_calls", "const uint64_t* poseidon_table", "uint32_t psdn_log_n", "uint64_t* out",
        "uint32_t* log_n_out"]
    assert _header_args("ola_generate_prog_chunk_trace") == [
        "OlaCtx* ctx", "const uint64_t* words", "size_t n_words", "const uint64_t* code_addr", "uint32_t flags", "const uint64_t* poseidon_table",
        "uint32_t psdn_log_n", "uint64_t* out", "uint32_t* log_n_out"]
    assert lib.ola_gpu_abi_version(None, None) == 7          # additions that change no struct keep the revision


def test_record_widths_and_the_flag_agree_everywhere():
    from olavm_amd import backend as B
    from olavm_amd.air import dump
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    cols = open(os.path.join(ROOT, dump.TABLEGEN_SMALL_COLUMNS_H)).read()
    for name, mine, printed in (("OLA_TAPE_CELL_WORDS", B.OLA_TAPE_CELL_WORDS, dump.TAPE_CELL_WORDS),
                                ("OLA_POSEIDON_CALL_WORDS", B.OLA_POSEIDON_CALL_WORDS, dump.POSEIDON_CALL_WORDS)):
        words = int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
        assert words == mine == printed
        assert "pub const %s: usize = %d;" % (name, words) in rs
        assert "%s = %du" % (name[len("OLA_"):], words) in cols
    assert "#define OLA_PROG_CHUNK_RESULT_LINE 1u" in hdr and "pub const OLA_PROG_CHUNK_RESULT_LINE: u32 = 1;" in rs and B.OLA_PROG_CHUNK_RESULT_LINE == 1


def test_column_header_of_the_kernels_is_the_table_description():
    from olavm_amd.air import dump, ola_tables as T
    text = open(os.path.join(ROOT, dump.TABLEGEN_SMALL_COLUMNS_H)).read()
    assert text == dump.tablegen_small_columns_header()
    seen = {}
    for name, a, b in re.findall(r"constexpr uint32_t (COL_\w+)_START = (\d+)u, \w+_END = (\d+)u;", text):
        assert getattr(T, name) == range(int(a), int(b))
        seen[name] = set(range(int(a), int(b)))
    for name, v in re.findall(r"constexpr uint32_t (COL_\w+) = (\d+)u;", text):
        assert getattr(T, name) == int(v)
        seen[name] = {int(v)}
    for prefix, width in (("COL_TAPE_", T.NUM_COL_TAPE), ("COL_POSEIDON_CHUNK_", T.NUM_POSEIDON_CHUNK_COLS), ("COL_PROG_CHUNK_", T.NUM_PROG_CHUNK_COLS),
                          ("COL_SCCALL_", T.NUM_COL_SCCALL)):
        cols = set().union(*(v for k, v in seen.items() if k.startswith(prefix)))
        assert cols == set(range(width)), prefix                                                  # every column of the table
    assert seen["COL_POSEIDON_INPUT_RANGE"] == set(range(4, 16)) and seen["COL_POSEIDON_OUTPUT_RANGE"] == set(range(16, 28))
    assert "NUM_COL_TAPE = 6u, NUM_POSEIDON_CHUNK_COLS = 53u, NUM_PROG_CHUNK_COLS = 40u, NUM_COL_SCCALL = 26u;" in text
    assert "NUM_POSEIDON_COLS = %du;" % T.NUM_POSEIDON_COLS in text
    assert "OP_MASK_TLOAD = %dull;" % T.op_mask("TLOAD") in text and "OP_MASK_POSEIDON = %dull;" % T.op_mask("POSEIDON") in text
    src = open(os.path.join(ROOT, "olavm_amd", "csrc", "tablegen.hip")).read()
    assert '#include "tablegen_small_columns.h"' in src
    new = src[src.index("// ---- the tape, Poseidon-chunk and program-chunk tables"):src.index("u32 log2_rows(")]
    assert "tx::COL_TAPE_ADDR" in new and not re.search(r"\bout\[\(size_t\)\d+ \* n|\bv\[\d", new), "a column index was typed in"


def test_sizing_calls_need_no_context(lib):
    log_n = C.c_uint32(99)
    for n_cells in (0, 1, 7, 8, 9, (1 << 12) + 3, (1 << 31) - 1):
        assert lib.ola_generate_tape_trace(None, None, n_cells, None, C.byref(log_n)) == 0
        assert 1 << log_n.value == next_pow2(max(n_cells, 8)), n_cells
    for lens in ([], [8], [8, 16, 40], [8] * 100 + [24] * 25):
        rec = calls_of(lens)
        rows = sum(1 + l // 8 for l in lens)
        for table in (None, ptr(np.zeros(1, dtype=np.uint64))):                                  # with a table the rows are checked as well
            assert lib.ola_generate_poseidon_chunk_trace(None, ptr(rec) if lens else None, len(lens), table, 8, None, C.byref(log_n)) == 0
            assert 1 << log_n.value == next_pow2(max(rows, 8)), lens
    for n_words in (0, 8, 16, 64, 72, 8 * 257):
        for flags in (0, 1):
            assert lib.ola_generate_prog_chunk_trace(None, None, n_words, None, flags, None, 9, None, C.byref(log_n)) == 0
            assert 1 << log_n.value == next_pow2(max(n_words // 8, 8)), n_words


def test_arguments_are_validated_first(lib):
    out = np.full(53 * 64, 7, dtype=np.uint64)
    table = np.zeros(134 * 8, dtype=np.uint64)
    cells = np.zeros((3, 4), dtype=np.uint64)
    words = np.zeros(16, dtype=np.uint64)
    addr = np.zeros(4, dtype=np.uint64)
    log_n = C.c_uint32(99)
    L = C.byref(log_n)
    pc = lambda rec, n=None, t=table, lg=3, o=out, l=L: lib.ola_generate_poseidon_chunk_trace(
        None, None if rec is None else ptr(rec), rec.shape[1] if n is None else n, None if t is None else ptr(t), lg, None if o is None else ptr(o), l)
    pg = lambda n_words=16, w=words, a=addr, flags=0, t=table, lg=3, o=out, l=L: lib.ola_generate_prog_chunk_trace(
        None, None if w is None else ptr(w), n_words, None if a is None else ptr(a), flags, None if t is None else ptr(t), lg,
        None if o is None else ptr(o), l)
    bad = [
        lambda: lib.ola_generate_tape_trace(None, ptr(cells), 4, ptr(out), None),
        lambda: lib.ola_generate_tape_trace(None, ptr(cells), 1 << 31, ptr(out), L),             # 2^31 cells or more
        lambda: lib.ola_generate_tape_trace(None, None, 1 << 31, None, L),                       # ... in a sizing call too
        lambda: lib.ola_generate_tape_trace(None, None, 4, ptr(out), L),                         # work without cells
        lambda: pc(calls_of([8, 16]), l=None),
        lambda: pc(calls_of([0, 8])),                                                            # len 0
        lambda: pc(calls_of([8, 12])),                                                           # no whole blocks
        lambda: pc(calls_of([8, P + 12])),                                                       # ... judged by the canonical value
        lambda: pc(calls_of([8, 12]), o=None, t=None),                                           # ... in a sizing call too
        lambda: pc(calls_of([8, 16], rows=[0, 7])),                                              # psdn_row + 2 blocks run off the 8-row table
        lambda: pc(calls_of([8, 16], rows=[8, 0])),
        lambda: pc(calls_of([8, 16], rows=[0, P + 7])),
        lambda: pc(calls_of([8, 16], rows=[0, 7]), o=None),                                      # ... which a sizing call with the table says as well
        lambda: pc(calls_of([8, 16]), lg=2),                                                     # psdn_log_n out of range
        lambda: pc(calls_of([8, 16]), lg=27),
        lambda: pc(None, n=2),                                                                   # calls without records
        lambda: pc(calls_of([8, 16]), n=1 << 26),
        lambda: pc(calls_of([8, 16]), t=None),                                                   # work without the table
        lambda: pg(l=None),
        lambda: pg(12),                                                                          # no whole chunks
        lambda: pg(12, o=None),
        lambda: pg(72, w=np.zeros(72, dtype=np.uint64)),                                         # nine chunks, eight table rows
        lambda: pg(flags=2),                                                                     # a flag nobody defined
        lambda: pg(lg=2),
        lambda: pg((1 << 29) + 8, lg=26),
        lambda: pg(w=None), lambda: pg(a=None), lambda: pg(t=None),                              # work without an input
    ]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in lib.ola_gpu_last_error()
    assert np.all(out == 7)
    # the last row of the table is inside it: only the device is missing then
    assert pc(calls_of([8, 16], rows=[7, 0])) in (OLA_E_NO_DEVICE, OLA_E_INVALID_ARG)
    assert b"ctx is NULL" in lib.ola_gpu_last_error() or b"no HIP device" in lib.ola_gpu_last_error()


def test_a_working_call_without_a_context_answers_as_the_header_says(lib):
    """OLA_E_NO_DEVICE on a machine without a HIP device (there is no CPU fallback), OLA_E_INVALID_ARG where there is one"""
    import torch
    want, text = (OLA_E_INVALID_ARG, b"ctx is NULL") if torch.cuda.is_available() else (OLA_E_NO_DEVICE, b"no HIP device")
    out = np.full(53 * 8, 7, dtype=np.uint64)
    table = np.zeros(134 * 8, dtype=np.uint64)
    cells, rec, words, addr = np.zeros((3, 2), dtype=np.uint64), calls_of([8]), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    log_n = C.c_uint32()
    for rcode in (lib.ola_generate_tape_trace(None, ptr(cells), 2, ptr(out), C.byref(log_n)),
                  lib.ola_generate_tape_trace(None, None, 0, ptr(out), C.byref(log_n)),
                  lib.ola_generate_poseidon_chunk_trace(None, ptr(rec), 1, ptr(table), 3, ptr(out), C.byref(log_n)),
                  lib.ola_generate_poseidon_chunk_trace(None, None, 0, ptr(table), 3, ptr(out), C.byref(log_n)),
                  lib.ola_generate_prog_chunk_trace(None, ptr(words), 8, ptr(addr), 1, ptr(table), 3, ptr(out), C.byref(log_n)),
                  lib.ola_generate_prog_chunk_trace(None, None, 0, ptr(addr), 0, ptr(table), 3, ptr(out), C.byref(log_n))):
        assert rcode == want and text in lib.ola_gpu_last_error()
    assert np.all(out == 7)
