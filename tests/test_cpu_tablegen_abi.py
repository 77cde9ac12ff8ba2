"""CPU-side checks of ola_generate_cpu_trace / ola_generate_prog_trace_steps (include/ola_gpu.h) and of the step records the native trace
generator hands out (OLA_TRACEGEN_STEPS_ONLY, include/ola_tracegen.h): the symbols are exported and declared -- header,
olavm_amd/backend.py, integration/rust/ola_gpu_sys.rs -- with the same shapes and constants, the kernels' column header is the table
description, arguments are validated before anything touches a device, a call that would do work says that there is no device, and a
steps-only run of the generator returns the records and the listing of the ordinary run (also under AddressSanitizer / UBSan)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_tablegen_abi import _header_args, _rust_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
ARITY = {"ola_generate_cpu_trace": 5, "ola_generate_prog_trace_steps": 9}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def test_symbols_are_exported_and_declared_with_equal_shapes(lib):
    from olavm_amd import backend as B
    for name, arity in ARITY.items():
        assert name in B.EXPORTS
        f = getattr(lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None
        h, r = _header_args(name), _rust_args(name)
        assert len(h) == len(r) == len(f.argtypes) == arity, (name, h, r)
        assert [a.split()[-1].lstrip("*") for a in h] == [a.split(":")[0] for a in r], name
    assert _header_args("ola_generate_cpu_trace") == ["OlaCtx* ctx", "const uint64_t* steps", "size_t n_steps", "uint32_t log_n", "uint64_t* out"]
    assert [a.split()[-1].lstrip("*") for a in _header_args("ola_generate_prog_trace_steps")] == [
        "ctx", "steps", "n_steps", "prog", "log_n", "beta", "flags", "out", "exec_rows_out"]
    for method in ("generate_cpu_trace", "generate_prog_trace_steps"):
        assert hasattr(B.Backend, method)
    assert lib.ola_gpu_abi_version(None, None) == 7          # additions that change no struct keep the revision


def test_record_width_and_flag_agree_everywhere():
    from olavm_amd import backend as B
    from olavm_amd.air import cpu_steps, dump, ola_tables as T
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    words = int(re.search(r"#define OLA_CPU_STEP_WORDS (\d+)", hdr).group(1))
    assert words == B.OLA_CPU_STEP_WORDS == cpu_steps.STEP_WORDS == dump.CPU_STEP_WORDS == T.COL_S_DST.stop - T.COL_ENV_IDX + 1
    assert "pub const OLA_CPU_STEP_WORDS: usize = %d;" % words in rs
    assert "#define OLA_TABLEGEN_ZERO_FILLER 1u" in hdr and "pub const OLA_TABLEGEN_ZERO_FILLER: u32 = 1;" in rs and B.OLA_TABLEGEN_ZERO_FILLER == 1
    tg = open(os.path.join(ROOT, "include", "ola_tracegen.h")).read()
    from olavm_amd.air import fastexec
    assert "#define OLA_TRACEGEN_STEPS_ONLY 8u" in tg and fastexec.OLA_TRACEGEN_STEPS_ONLY == 8


def test_column_header_of_the_kernels_is_the_table_description():
    from olavm_amd.air import dump, ola_tables as T
    text = open(os.path.join(ROOT, dump.TABLEGEN_CPU_COLUMNS_H)).read()
    assert text == dump.tablegen_cpu_columns_header()
    assert "constexpr uint32_t COL_FILTER_LOOKING_PROG_IMM = %du;" % T.COL_FILTER_LOOKING_PROG_IMM in text
    assert "constexpr uint32_t COL_S_DST_START = %du, COL_S_DST_END = %du;" % (T.COL_S_DST.start, T.COL_S_DST.stop) in text
    assert "constexpr uint32_t OP_SHIFT_SCCALL = %du;" % T.OPCODE_SHIFT["SCCALL"] in text and "constexpr uint32_t STEP_WORDS = 66u;" in text
    assert "COL_MEM_" not in text and "COL_PROG_" not in text
    covered = [int(v) for v in re.findall(r"constexpr uint32_t (?:COL_\w+|IS_SCCALL_EXT_LINE) = (\d+)u;", text)]
    for lo, hi in re.findall(r"constexpr uint32_t COL_\w+_START = (\d+)u, COL_\w+_END = (\d+)u;", text):
        covered += range(int(lo), int(hi))
    assert sorted(covered) == list(range(T.NUM_CPU_COLS))                # every column of the CPU table, once
    src = open(os.path.join(ROOT, "olavm_amd", "csrc", "tablegen.hip")).read()
    assert '#include "tablegen_cpu_columns.h"' in src
    gen = src[src.index("cpu_fill_kernel"):]
    assert not re.search(r"\bout \+ \(size_t\)\d+ \* n|\bout\[\(size_t\)\d+ \* n", gen), "a column index was typed in"


def test_arguments_are_validated_first(lib):
    steps = np.zeros(66 * 9, dtype=np.uint64)
    side = np.zeros(7 * 8, dtype=np.uint64)
    out = np.full(94 * 8, 7, dtype=np.uint64)
    rows = C.c_uint64(99)
    s, p, o = C.c_void_p(steps.ctypes.data), C.c_void_p(side.ctypes.data), C.c_void_p(out.ctypes.data)
    bad = [
        lambda: lib.ola_generate_cpu_trace(None, None, 3, 3, o),                          # steps without records
        lambda: lib.ola_generate_cpu_trace(None, s, 3, 3, None),
        lambda: lib.ola_generate_cpu_trace(None, s, 9, 3, o),                             # 2^log_n < n_steps
        lambda: lib.ola_generate_cpu_trace(None, s, 3, 0, o),                             # a table of one row
        lambda: lib.ola_generate_cpu_trace(None, s, 3, 27, o),
        lambda: lib.ola_generate_prog_trace_steps(None, None, 3, p, 3, 5, 0, o, C.byref(rows)),
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, None, 3, 5, 0, o, C.byref(rows)),
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, p, 3, 5, 0, None, C.byref(rows)),
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, p, 3, 5, 0, o, None),          # nowhere to put the count
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, p, 0, 5, 0, o, C.byref(rows)),
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, p, 27, 5, 0, o, C.byref(rows)),
        lambda: lib.ola_generate_prog_trace_steps(None, s, 3, p, 3, 5, 2, o, C.byref(rows)),  # a flag nobody defined
        lambda: lib.ola_generate_prog_trace_steps(None, s, 1 << 31, p, 3, 5, 0, o, C.byref(rows)),     # indices stay in 32 bits
    ]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in lib.ola_gpu_last_error()
    assert np.all(out == 7) and rows.value == 99


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    steps = np.zeros(66 * 3, dtype=np.uint64)
    side = np.zeros(7 * 8, dtype=np.uint64)
    out = np.full(94 * 8, 7, dtype=np.uint64)
    rows = C.c_uint64(99)
    s, p, o = C.c_void_p(steps.ctypes.data), C.c_void_p(side.ctypes.data), C.c_void_p(out.ctypes.data)
    for rc in (lib.ola_generate_cpu_trace(None, s, 3, 3, o), lib.ola_generate_cpu_trace(None, None, 0, 3, o),
               lib.ola_generate_prog_trace_steps(None, s, 3, p, 3, 5, 1, o, C.byref(rows)),
               lib.ola_generate_prog_trace_steps(None, None, 0, p, 3, 5, 0, o, C.byref(rows))):
        assert rc == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()
    assert np.all(out == 7) and rows.value == 99


@pytest.mark.parametrize("name", ["tape_program", "storage_program", "memory_program"])
def test_steps_only_run_of_the_native_generator(lib, name):
    from olavm_amd.air import cpu_steps as S, fastexec as F, miniexec as M, ola_tables as T
    prog = getattr(M, name)()
    traces, params, compress = F.instance(prog)
    lean, lean_params, lean_compress, rec = F.instance(prog, steps_only=True)
    assert lean[T.CPU] is None and lean[T.PROGRAM] is None
    cpu, pg = traces[T.CPU], traces[T.PROGRAM]
    assert np.array_equal(rec["steps"], S.from_table(cpu, S.live_rows(cpu))) and rec["steps"].shape[0] == S.STEP_WORDS
    assert np.array_equal(rec["listing"], S.prog_listing(pg))
    assert (rec["cpu_log_n"], rec["prog_log_n"]) == (cpu.shape[1].bit_length() - 1, pg.shape[1].bit_length() - 1)
    for t in range(12):
        if t not in (T.CPU, T.PROGRAM):
            assert np.array_equal(lean[t], traces[t]), t
    assert lean_params == params and lean_compress == compress
    # without the flag the accessors answer with an error
    L = F.load_library()
    code, stor, handle = (C.c_uint64 * 4)(*prog.code_addr), (C.c_uint64 * 4)(*prog.storage_addr), C.c_void_p()
    ins = F.encode(prog)
    assert L.ola_tracegen_run(ins, len(prog.ins), code, stor, 4, 2, 0, 0, 1 << 16, 0, C.byref(handle)) == 0
    n, log_n, data = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint64)()
    assert L.ola_tracegen_cpu_steps(handle, C.byref(n), C.byref(data)) == -1 and b"STEPS_ONLY" in L.ola_tracegen_last_error()
    assert L.ola_tracegen_prog_listing(handle, C.byref(log_n), C.byref(data)) == -1
    L.ola_tracegen_free(handle)


def test_steps_only_generator_is_clean_under_the_sanitizers(lib, tmp_path):
    """a stand-alone host program over tracegen.cpp, with and without OLA_TRACEGEN_STEPS_ONLY"""
    exe = str(tmp_path / "host_tracegen_steps")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host_tracegen_steps.cpp"), os.path.join(ROOT, "olavm_amd", "csrc", "host", "tracegen.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
