"""CPU-side checks of ola_generate_storage_trace / ola_generate_poseidon_table (include/ola_gpu.h): the symbols are exported and declared
-- header, olavm_amd/backend.py, include/ola_host.hpp, integration/rust/ola_gpu_sys.rs -- with the same shapes and constants, the kernels'
column header is the table description, sizing calls need no context, arguments are validated before anything touches a device, a call
that would do work says that there is no device; and the reference's generate_storage_access_trace (generation/storage.rs, interpreted:
tests/golden/ref_storage_rows.json) on a write and its read-back gives the table miniexec's tree and storage_trace give -- the same
two accesses the GPU test feeds to the device; and a hashes-only run of the native generator (OLA_TRACEGEN_HASHES_ONLY, include/ola_tracegen.h)
returns the records and Poseidon inputs that stand behind the ordinary run's two tables (also under AddressSanitizer / UBSan, stand-alone)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_tablegen_abi import _header_args, _rust_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_storage_rows.json")
REF = "/root/reference"
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
ARGS = {"ola_generate_storage_trace": ["ctx", "accesses", "n_access", "siblings", "out", "log_n_out", "psdn_inputs", "psdn_filters", "psdn_stride",
                                       "roots_out"],
        "ola_generate_poseidon_table": ["ctx", "inputs", "filters", "n_rows", "stride", "out", "log_n_out"]}


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
    assert _header_args("ola_generate_storage_trace") == [
        "OlaCtx* ctx", "const uint64_t* accesses", "size_t n_access", "const uint64_t* siblings", "uint64_t* out", "uint32_t* log_n_out",
        "uint64_t* psdn_inputs", "uint64_t* psdn_filters", "size_t psdn_stride", "uint64_t roots_out[8]"]
    assert _header_args("ola_generate_poseidon_table") == ["OlaCtx* ctx", "const uint64_t* inputs", "const uint64_t* filters", "size_t n_rows",
                                                           "size_t stride", "uint64_t* out", "uint32_t* log_n_out"]
    # the older entry point keeps its signature
    assert _header_args("ola_generate_poseidon_trace") == ["OlaCtx* ctx", "const uint64_t* inputs", "const uint64_t* filters", "size_t n", "uint64_t* out"]
    assert lib.ola_gpu_abi_version(None, None) == 7          # additions that change no struct keep the revision


def test_record_width_and_flags_agree_everywhere():
    from olavm_amd import backend as B
    from olavm_amd.air import dump
    from tests import storage_rules as R
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    words = int(re.search(r"#define OLA_STORAGE_ACCESS_WORDS (\d+)", hdr).group(1))
    assert words == B.OLA_STORAGE_ACCESS_WORDS == dump.STORAGE_ACCESS_WORDS == R.WORDS == 14
    assert "pub const OLA_STORAGE_ACCESS_WORDS: usize = %d;" % words in rs
    for name, bit, mine in (("WRITE", 1, R.WRITE), ("FOR_PROG", 2, R.FOR_PROG), ("SILENT", 4, R.SILENT)):
        assert "#define OLA_STORAGE_%s %du" % (name, bit) in hdr and "pub const OLA_STORAGE_%s: u64 = %d;" % (name, bit) in rs
        assert getattr(B, "OLA_STORAGE_" + name) == mine == bit


def test_column_header_of_the_kernels_is_the_table_description():
    from olavm_amd.air import dump, ola_tables as T
    text = open(os.path.join(ROOT, dump.TABLEGEN_STORAGE_COLUMNS_H)).read()
    assert text == dump.tablegen_storage_columns_header()
    cols = set()
    for name, a, b in re.findall(r"constexpr uint32_t (COL_ST_\w+)_START = (\d+)u, \w+_END = (\d+)u;", text):
        assert getattr(T, name) == range(int(a), int(b))
        cols |= set(range(int(a), int(b)))
    for name, v in re.findall(r"constexpr uint32_t (COL_ST_\w+) = (\d+)u;", text):
        assert getattr(T, name) == int(v)
        cols.add(int(v))
    assert cols == set(range(T.NUM_COL_ST)) and T.NUM_COL_ST == 48                           # every column of the table
    assert "NUM_COL_ST = 48u, NUM_POSEIDON_COLS = %du;" % T.NUM_POSEIDON_COLS in text
    src = open(os.path.join(ROOT, "olavm_amd", "csrc", "storage.hip")).read()
    assert '#include "tablegen_storage_columns.h"' in src
    assert not re.search(r"\bout\[\(size_t\)\d+ \* n_out|col\(\d", src), "a column index was typed in"


def test_sizing_calls_need_no_context(lib):
    from tests import storage_rules as R
    log_n = C.c_uint32(99)
    for n_access in (0, 1, 2, 3, 141, (1 << 23) - 1):
        assert lib.ola_generate_storage_trace(None, None, n_access, None, None, C.byref(log_n), None, None, 0, None) == 0
        assert 1 << log_n.value == next_pow2(max(256 * n_access, 8)), n_access
    # with records the silent ones have no rows
    for name, batch in R.BATCHES.items():
        recs = R.records(batch)
        m = sum(1 for _, _, flags in batch if not flags & R.SILENT)
        assert lib.ola_generate_storage_trace(None, ptr(recs) if len(batch) else None, len(batch), None, None, C.byref(log_n), None, None, 0, None) == 0
        assert 1 << log_n.value == next_pow2(max(256 * m, 8)), name
    for n_rows in (0, 5, 8, 9, 300, 1 << 22):
        assert lib.ola_generate_poseidon_table(None, None, None, n_rows, n_rows + 3, None, C.byref(log_n)) == 0
        assert 1 << log_n.value == next_pow2(max(n_rows, 8)), n_rows


def test_arguments_are_validated_first(lib):
    from tests import storage_rules as R
    P = R.P
    batch = R.BATCHES["write_read_overwrite"]
    rows, stride = R.psdn_rows(batch)
    recs = R.records(batch)
    out = np.full(48 * 1024, 7, dtype=np.uint64)
    inputs, filters = np.full(12 * stride, 7, dtype=np.uint64), np.full(4 * stride, 7, dtype=np.uint64)
    sib = np.zeros(1024 * 3, dtype=np.uint64)
    roots = np.full(8, 7, dtype=np.uint64)
    log_n = C.c_uint32(99)
    silent, unknown, late, later = recs.copy(), recs.copy(), recs.copy(), recs.copy()
    silent[12, 0] = R.WRITE | R.SILENT
    unknown[12, 2] = 8
    late[13, 2] = stride - 511                    # its last row would be row `stride`
    later[13, 1] = stride + P                     # a row word >= p is judged by its canonical value
    call = lambda a, s=None, n=3, o=out, i=inputs, f=filters, st=stride, l=C.byref(log_n): lib.ola_generate_storage_trace(
        None, ptr(a), n, None if s is None else ptr(s), None if o is None else ptr(o), l, None if i is None else ptr(i), None if f is None else ptr(f),
        st, ptr(roots))
    bad = [
        lambda: call(recs, l=None),
        lambda: call(recs, n=1 << 23),                                   # 2^23 accesses or more
        lambda: lib.ola_generate_storage_trace(None, None, 1 << 23, None, None, C.byref(log_n), None, None, 0, None),    # ... in a sizing call too
        lambda: call(late),                                              # a psdn_row beyond the stride
        lambda: call(later),
        lambda: call(recs, st=rows[2] + 511),
        lambda: call(late, o=None),                                      # ... which a sizing call with the buffers says as well
        lambda: call(silent, s=sib),                                     # silent together with the caller's siblings
        lambda: call(unknown),                                           # a flag nobody defined
        lambda: call(recs, f=None),                                      # inputs without filters
        lambda: call(recs, i=None),
        lambda: lib.ola_generate_storage_trace(None, None, 3, None, ptr(out), C.byref(log_n), None, None, 0, None),      # work without records
        lambda: lib.ola_generate_poseidon_table(None, ptr(inputs), None, 9, 8, ptr(out), C.byref(log_n)),                # stride < n_rows
        lambda: lib.ola_generate_poseidon_table(None, None, None, 9, 8, None, C.byref(log_n)),
        lambda: lib.ola_generate_poseidon_table(None, ptr(inputs), None, 8, 8, ptr(out), None),
        lambda: lib.ola_generate_poseidon_table(None, None, None, (1 << 26) + 1, 1 << 27, None, C.byref(log_n)),
        lambda: lib.ola_generate_poseidon_table(None, None, None, 8, 8, ptr(out), C.byref(log_n)),                       # rows without inputs
    ]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in lib.ola_gpu_last_error()
    assert np.all(out == 7) and np.all(inputs == 7) and np.all(filters == 7) and np.all(roots == 7)
    # the same records with a stride that holds them pass the validation: only the device is missing then
    assert call(recs) in (OLA_E_NO_DEVICE, OLA_E_INVALID_ARG) and b"psdn" not in lib.ola_gpu_last_error()
    assert call(silent) in (OLA_E_NO_DEVICE, OLA_E_INVALID_ARG) and (b"ctx is NULL" in lib.ola_gpu_last_error() or b"no HIP device" in lib.ola_gpu_last_error())


def test_a_working_call_without_a_context_answers_as_the_header_says(lib):
    """OLA_E_NO_DEVICE on a machine without a HIP device (there is no CPU fallback), OLA_E_INVALID_ARG where there is one"""
    import torch
    from tests import storage_rules as R
    want, text = (OLA_E_INVALID_ARG, b"ctx is NULL") if torch.cuda.is_available() else (OLA_E_NO_DEVICE, b"no HIP device")
    recs = R.records(R.BATCHES["one_write"])
    out = np.full(134 * 256, 7, dtype=np.uint64)
    inputs = np.zeros(12 * 8, dtype=np.uint64)
    log_n = C.c_uint32()
    for rcode in (lib.ola_generate_storage_trace(None, ptr(recs), 1, None, ptr(out), C.byref(log_n), None, None, 0, None),
                  lib.ola_generate_storage_trace(None, None, 0, None, ptr(out), C.byref(log_n), None, None, 0, None),
                  lib.ola_generate_poseidon_table(None, ptr(inputs), None, 5, 8, ptr(out), C.byref(log_n)),
                  lib.ola_generate_poseidon_table(None, None, None, 0, 0, ptr(out), C.byref(log_n))):
        assert rcode == want and text in lib.ola_gpu_last_error()
    assert np.all(out == 7)


# ---- the reference's generator on a write and its read-back
@pytest.fixture(scope="module")
def ref():
    return json.load(open(FIXTURE))


def test_reference_rows_are_storage_trace_of_miniexecs_tree(ref):
    """generate_storage_access_trace's 512 live rows, column for column, and its padding rule.  The reference pads to at least 2 rows and this
    project to at least 8 (the smallest table the prover takes), so heights are not compared."""
    from olavm_amd.air import miniexec as M, ola_tables as T
    from tests import storage_rules as R
    batch = R.BATCHES["write_read_overwrite"]
    assert list(batch[0][0]) == ref["key"] and list(batch[0][1]) == ref["value"] and batch[1][1] is None          # the GPU test's first two accesses
    want = ref["accesses"]
    assert want["rows"] == 512 and len(want["column_sha256"]) == T.NUM_COL_ST
    tree = M.StorageTree()
    rows = [tree.access(ref["key"], ref["value"])[0], tree.access(ref["key"])[0]]
    sha = lambda col: hashlib.sha256(np.ascontiguousarray(col, dtype="<u8").tobytes()).hexdigest()
    for got in (M.storage_trace(rows), R.reference("write_read_overwrite")["table"][:, :512]):            # the second is what the device is held to
        assert got.shape == (T.NUM_COL_ST, 512)
        assert [[int(x) for x in got[:, i]] for i in ref["rows_kept"]] == want["kept"]
        for c in range(T.NUM_COL_ST):
            assert sha(got[c]) == want["column_sha256"][c], c
    # the read-back as the program-hash read: one column differs, set in the layer-256 row of the read alone
    prog = ref["write_then_prog_read"]
    assert prog["columns_that_differ"] == [T.COL_ST_FILTER_IS_FOR_PROG] and prog["rows_set"] == [[511]]
    got = M.storage_trace(rows[:1], rows[1:])
    assert np.flatnonzero(got[T.COL_ST_FILTER_IS_FOR_PROG]).tolist() == [511] and not M.storage_trace(rows)[T.COL_ST_FILTER_IS_FOR_PROG].any()
    # padding: IS_PADDING and the last root, zero in a table without rows
    none = np.array(ref["none"], dtype=np.uint64)
    got = M.storage_trace([])
    assert none.shape == (T.NUM_COL_ST, 2) and got.shape == (T.NUM_COL_ST, 8)
    for c in range(T.NUM_COL_ST):
        assert set(none[c].tolist()) == set(got[c].tolist()) == ({1} if c == T.COL_ST_IS_PADDING else {0}), c
    three = M.storage_trace(rows + rows[:1])                                                                        # 768 rows: 256 of padding
    assert three.shape[1] == 1024 and (three[T.COL_ST_IS_PADDING, 768:] == 1).all()
    for c in range(T.NUM_COL_ST):
        if c in T.COL_ST_ROOT_RANGE:
            assert (three[c, 768:] == three[c, 767]).all()
        elif c != T.COL_ST_IS_PADDING:
            assert not three[c, 768:].any(), c


# ---- OLA_TRACEGEN_HASHES_ONLY of the native generator
@pytest.mark.parametrize("name", ["storage", "storage_heavy", "hash"])
def test_hashes_only_run_of_the_native_generator(lib, name):
    """the lean run's records and Poseidon inputs are what the full run's tables contain; the other tables are the cells-only run's"""
    from olavm_amd.air import fastexec as F, miniexec as M, ola_tables as T
    from tests import storage_rules as R
    make, kw = M.EXAMPLES[name]
    prog = make()
    full, params, compress = F.instance(prog, **kw)
    lean, lean_params, lean_compress, rec = F.instance(prog, hashes_only=True, **kw)
    left_out = (T.CPU, T.MEMORY, T.CMP, T.RANGECHECK, T.POSEIDON, T.STORAGE_ACCESS, T.PROGRAM)
    for t in range(12):
        assert (lean[t] is None) if t in left_out else np.array_equal(lean[t], full[t]), t
    listing = prog.words()[0]
    silent = [(prog.code_addr, M.program_hash(listing + [0] * (-len(listing) % 8)))] if kw.get("prove_program_hash") else []
    want, owned = R.records_from_tables(full[T.STORAGE_ACCESS], full[T.POSEIDON], silent)
    assert rec["accesses"].shape == want.shape and np.array_equal(rec["accesses"], want)
    inputs, filters = full[T.POSEIDON][4:16].copy(), full[T.POSEIDON][0:4].copy()
    inputs[:, owned], filters[:, owned] = 0, 0
    assert np.array_equal(rec["psdn_inputs"], inputs) and np.array_equal(rec["psdn_filters"], filters)
    assert [rec["storage_log_n"], rec["poseidon_log_n"]] == [full[t].shape[1].bit_length() - 1 for t in (T.STORAGE_ACCESS, T.POSEIDON)]
    assert lean_params == [params[0], None] and lean_compress[T.PROGRAM] is None                  # not known before the device has hashed the tree
    if silent:                                                                                    # ... and drawn from the full run's roots it is the full run's
        st = full[T.STORAGE_ACCESS]
        last = int((st[T.COL_ST_IS_PADDING] == 0).sum()) - 1
        roots = [int(st[c, 0]) for c in T.COL_ST_PRE_ROOT_RANGE] + [int(st[c, last]) for c in T.COL_ST_ROOT_RANGE]
        assert F.program_beta(roots) == params[1] == M.derive_program_beta(roots[:4], roots[4:])
        assert int(rec["accesses"][12, 0]) == R.WRITE | R.SILENT and int(rec["accesses"][12, -1]) == R.FOR_PROG
    fixed = F.instance(prog, hashes_only=True, bitwise_beta=5, program_beta=6, **kw)
    assert fixed[1] == [5, 6]
    tg = open(os.path.join(ROOT, "include", "ola_tracegen.h")).read()
    assert "#define OLA_TRACEGEN_HASHES_ONLY 32u" in tg and F.OLA_TRACEGEN_HASHES_ONLY == 32 and F.STORAGE_ACCESS_WORDS == 14
    for f in ("ola_tracegen_storage_accesses", "ola_tracegen_poseidon_inputs", "ola_tracegen_program_beta"):
        assert f in tg and f in F.EXPORTS


def test_hashes_only_generator_is_clean_under_the_sanitizers(lib, tmp_path):
    """a stand-alone host program over tracegen.cpp, with and without OLA_TRACEGEN_HASHES_ONLY"""
    exe = str(tmp_path / "host_tracegen_hashes")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host_tracegen_hashes.cpp"), os.path.join(ROOT, "olavm_amd", "csrc", "host", "tracegen.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_what_the_reference_computes_today():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rust_air_eval.py"), "--tracegen", "storage", "--check", "--reference", REF],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "up to date" in r.stdout, r.stdout + r.stderr
