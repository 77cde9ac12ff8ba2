"""CPU-side checks of ola_check_lookup (include/ola_gpu.h): the symbol is exported and declared with prototypes in
olavm_amd/backend.py, header, ctypes struct and Rust declaration agree on the layout of OlaLookupMismatch, OLA_LOOKUP_MAX_VALUES is
the widest lookup of the AIR set, the arguments are validated before anything touches a device, and without a device the call says
so -- there is no CPU fallback."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
FIELDS = [("uint64_t", "looking_count"), ("uint64_t", "looked_count"), ("uint32_t", "looking_entry"), ("uint32_t", "looking_table"),
          ("uint64_t", "looking_row"), ("uint64_t", "looked_row"), ("uint64_t", "values")]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


@pytest.fixture(scope="module")
def call(lib):
    """a well-formed call for the miniature 12-table AIR set and fibonacci(5), with keyword overrides"""
    from olavm_amd.air import miniexec as M, ola_tables as T
    from olavm_amd.backend import U64P, OlaLookupMismatch
    traces = M.instance(M.fibonacci(5))[0]
    blob = np.ascontiguousarray(T.ola_stark(range_bits=4, limb_bits=2).blob(), dtype=np.uint64)
    keep = [np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
    tabs = [(U64P * t.shape[0])(*[C.cast(C.c_void_p(t.ctypes.data + 8 * t.shape[1] * c), U64P) for c in range(t.shape[0])]) for t in keep]
    ptrs = (C.POINTER(U64P) * len(tabs))(*[C.cast(a, C.POINTER(U64P)) for a in tabs])
    logs = (C.c_uint32 * len(keep))(*[int(t.shape[1]).bit_length() - 1 for t in keep])
    state = {"out": (OlaLookupMismatch * 8)(), "n_out": C.c_uint32(77), "totals": (C.c_uint64 * 4)(5, 5, 5, 5), "width": C.c_uint32(99), "keep": (keep, tabs)}

    def f(**kw):
        v = {"airset": blob.ctypes.data_as(U64P), "words": blob.size, "cols": ptrs, "logs": logs, "lookup": 16, "out": state["out"], "cap": 8,
             "n_out": C.byref(state["n_out"]), "totals": state["totals"], "width": C.byref(state["width"])}
        v.update(kw)
        return lib.ola_check_lookup(None, v["airset"], v["words"], v["cols"], v["logs"], v["lookup"], v["out"], v["cap"], v["n_out"], v["totals"],
                                    v["width"])
    f.state, f.ptrs, f.n_lookups = state, ptrs, int(blob[3])
    return f


def test_symbol_is_exported_and_has_prototypes(lib):
    from olavm_amd import backend as B
    assert "ola_check_lookup" in B.EXPORTS
    f = lib.ola_check_lookup
    assert f.restype is C.c_int32
    assert f.argtypes is not None and len(f.argtypes) == 11
    assert f.argtypes[5] is C.c_uint32 and f.argtypes[7] is C.c_uint32                  # lookup, cap
    assert f.argtypes[6]._type_ is B.OlaLookupMismatch and f.argtypes[8]._type_ is C.c_uint32 and f.argtypes[10]._type_ is C.c_uint32
    assert hasattr(B.Backend, "check_lookup") and hasattr(B.Backend, "check_lookup_raw")
    # the ABI revision did not move, and the history comment says what was added to it
    assert lib.ola_gpu_abi_version(None, None) == 7
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    history = hdr[hdr.index("/* ABI revision of this header."):hdr.index("#define OLA_GPU_ABI_VERSION 7")]
    assert "OlaLookupMismatch" in history and "ola_check_lookup" in history


def test_header_ctypes_and_rust_agree_on_the_struct():
    from olavm_amd import backend as B
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    max_values = int(re.search(r"#define OLA_LOOKUP_MAX_VALUES (\d+)", hdr).group(1))
    body = re.search(r"typedef struct OlaLookupMismatch \{(.*?)\} OlaLookupMismatch;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint\d+_t)\s+(\w+)(\[OLA_LOOKUP_MAX_VALUES\])?;", body)
    assert [(t, n) for t, n, _ in fields] == FIELDS and [bool(a) for _, _, a in fields] == [False] * 6 + [True]
    # natural alignment of the header's fields, in order -> offsets and size
    off, want = 0, {}
    for t, n, arr in fields:
        size = int(t[4:-2]) // 8
        off = (off + size - 1) // size * size
        want[n] = off
        off += size * (max_values if arr else 1)
    assert {n: getattr(B.OlaLookupMismatch, n).offset for _, n in FIELDS} == want
    assert C.sizeof(B.OlaLookupMismatch) == off == 40 + 8 * max_values and B.OLA_LOOKUP_MAX_VALUES == max_values
    assert [n for n, _ in B.OlaLookupMismatch._fields_] == [n for _, n in FIELDS]
    # the prototype
    proto = re.search(r"int32_t ola_check_lookup\((.*?)\);", hdr, flags=re.S).group(1)
    params = [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")]
    assert params == ["OlaCtx* ctx", "const uint64_t* airset", "size_t airset_words", "const uint64_t* const* const* cols", "const uint32_t* log_n",
                      "uint32_t lookup", "OlaLookupMismatch* out", "uint32_t cap", "uint32_t* n_out", "uint64_t totals[4]", "uint32_t* width"]
    # Rust: the #[repr(C)] struct and the declaration
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    assert "pub const OLA_LOOKUP_MAX_VALUES: usize = %d;" % max_values in rs
    m = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct OlaLookupMismatch \{(.*?)\n\}", rs, flags=re.S)
    assert m, "OlaLookupMismatch must be #[repr(C)]"
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", m.group(1)) == [
        ("looking_count", "u64"), ("looked_count", "u64"), ("looking_entry", "u32"), ("looking_table", "u32"), ("looking_row", "u64"), ("looked_row", "u64"),
        ("values", "[u64; OLA_LOOKUP_MAX_VALUES]")]
    decl = re.search(r"pub fn ola_check_lookup\((.*?)\) -> i32;", rs, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")] == [
        "ctx: *mut OlaCtx", "airset: *const u64", "airset_words: usize", "cols: *const *const *const u64", "log_n: *const u32", "lookup: u32",
        "out: *mut OlaLookupMismatch", "cap: u32", "n_out: *mut u32", "totals: *mut u64", "width: *mut u32"]
    shim = open(os.path.join(ROOT, "integration", "rust", "hip_prover.rs")).read()
    assert "ola_check_lookup(" in shim and "OLA_CHECK_LOOKUP" in shim


def test_max_values_is_the_widest_lookup_of_the_air_set():
    from olavm_amd import backend as B
    from olavm_amd.air import dump, ola_tables as T
    widest = max(len(twc.columns) for c in T.ola_stark().ctls for twc in c.looking_tables + [c.looked_table])
    assert B.OLA_LOOKUP_MAX_VALUES == widest == dump.lookup_max_values()
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    printed = subprocess.run([sys.executable, "-m", "olavm_amd.air.dump", "--lookup-max-values"], cwd=ROOT, capture_output=True, text=True, check=True)
    assert printed.stdout.strip() in hdr.split("\n")


def test_arguments_are_checked_before_a_device_is_looked_for(lib, call):
    from olavm_amd.backend import U64P
    for kw in ({"airset": None}, {"cols": None}, {"logs": None}, {"n_out": None}, {"out": None}, {"totals": None}, {"width": None}):
        assert call(**kw) == OLA_E_INVALID_ARG, kw
        assert b"null pointer" in lib.ola_gpu_last_error()
    for lookup in (call.n_lookups, call.n_lookups + 1, 0xFFFFFFFF):
        assert call(lookup=lookup) == OLA_E_INVALID_ARG and b"lookup index" in lib.ola_gpu_last_error()
    assert call(words=100) == OLA_E_INVALID_ARG           # a truncated AIR-set blob
    # a table the lookup names without columns; one it does not name may be NULL (lookup 16: CPU -> program)
    holes = (type(call.ptrs))(*call.ptrs)
    holes[10] = C.POINTER(U64P)()
    assert call(cols=holes) == OLA_E_INVALID_ARG and b"cols[t]" in lib.ola_gpu_last_error()
    holes = (type(call.ptrs))(*[p if t in (0, 10) else C.POINTER(U64P)() for t, p in enumerate(call.ptrs)])
    assert call(cols=holes) != OLA_E_INVALID_ARG or b"cols[t]" not in lib.ola_gpu_last_error()
    # nothing was written by the refused calls
    s = call.state
    assert s["n_out"].value == 77 and s["width"].value == 99 and list(s["totals"]) == [5, 5, 5, 5]


def test_a_column_beyond_its_table_in_another_lookup_is_refused_before_a_device_is_looked_for(lib, call):
    """the parser every entry point shares holds every lookup to its tables, not only the one asked about"""
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import U64P
    airset = T.ola_stark(range_bits=4, limb_bits=2)
    blob = np.ascontiguousarray(airset.blob(), dtype=np.uint64)
    side = airset.ctls[0].looking_tables[0]
    assert side.columns[0].terms
    at = 4 + sum(len(t.words()) for t in airset.tables) + 1 + 2 + 1     # lookup 0: count of looking sides | table, columns | terms | column
    assert int(blob[at]) == side.columns[0].terms[0][0]
    blob[at] = airset.tables[side.table].ncols
    p = blob.ctypes.data_as(U64P)
    assert call(airset=p, lookup=16) == OLA_E_INVALID_ARG and b"AIR-set blob" in lib.ola_gpu_last_error()
    flags = (C.c_uint8 * 12)()
    assert lib.ola_air_kernels_available(p, blob.size, flags, 12) == OLA_E_INVALID_ARG and b"AIR-set blob" in lib.ola_gpu_last_error()
    s = call.state
    assert s["n_out"].value == 77 and s["width"].value == 99 and list(s["totals"]) == [5, 5, 5, 5]


def test_a_lookup_wider_than_the_struct_is_refused(lib, call):
    from olavm_amd.air.dsl import AirSet, AirTable, Col, CrossTableLookup, TableWithColumns
    from olavm_amd.backend import OLA_LOOKUP_MAX_VALUES, U64P
    w = OLA_LOOKUP_MAX_VALUES + 1
    cols = [Col.single(k) for k in range(w)]
    blob = np.ascontiguousarray(AirSet([AirTable("a", w, 3), AirTable("b", w, 3)],
                                       [CrossTableLookup([TableWithColumns(0, cols)], TableWithColumns(1, cols))]).blob(), dtype=np.uint64)
    assert call(airset=blob.ctypes.data_as(U64P), words=blob.size, lookup=0) == OLA_E_INVALID_ARG
    assert b"OLA_LOOKUP_MAX_VALUES" in lib.ola_gpu_last_error()


def test_no_cpu_fallback_without_device(lib, call):
    """A context cannot be created without a device: a well-formed call then reports that instead of evaluating anything on the
    host, and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert call() == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()
    s = call.state
    assert s["n_out"].value == 77 and s["width"].value == 99 and all(m.looking_count == 0 for m in s["out"])


def test_host_program_compiles_and_checks_the_arguments(tmp_path, call):
    """tests/host_check_lookup.cpp against the in-tree library, warning-free: usage without arguments, and with --args the calls
    the library must refuse before it looks for a device."""
    from olavm_amd.air import miniexec as M, ola_tables as T
    exe = os.path.join(str(tmp_path), "host_check_lookup")
    lib_dir = os.path.join(ROOT, "olavm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_check_lookup.cpp"), "-o", exe, "-L" + lib_dir, "-lola_gpu", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
    traces = M.instance(M.fibonacci(5))[0]
    blob = T.ola_stark(range_bits=4, limb_bits=2).blob()
    words = [blob.size] + [int(x) for x in blob] + [len(traces)]
    for t in traces:
        words += [int(t.shape[1]).bit_length() - 1, t.size] + [int(x) for x in np.ascontiguousarray(t).reshape(-1)]
    path = os.path.join(str(tmp_path), "instance.bin")
    np.array(words, dtype="<u8").tofile(path)
    r = subprocess.run([exe, path, "--args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks: 0 failed" in r.stdout, r.stdout + r.stderr
