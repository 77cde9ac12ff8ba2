"""CPU-side checks of ola_check_constraints (include/ola_gpu.h): the symbol is exported and declared with prototypes in
olavm_amd/backend.py, its arguments are validated before anything touches a device, and without a device the call says so -- the
constraint check has no CPU fallback either."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def _args(traces, mask=None):
    """ctypes arguments of a well-formed call for the miniature 12-table AIR set"""
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import U64P, OlaConstraintFailure
    blob = np.ascontiguousarray(T.ola_stark(range_bits=4, limb_bits=2).blob(), dtype=np.uint64)
    keep = [np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
    tabs = [(U64P * t.shape[0])(*[C.cast(C.c_void_p(t.ctypes.data + 8 * t.shape[1] * c), U64P) for c in range(t.shape[0])]) for t in keep]
    ptrs = (C.POINTER(U64P) * len(tabs))(*[C.cast(a, C.POINTER(U64P)) for a in tabs])
    logs = (C.c_uint32 * len(keep))(*[int(t.shape[1]).bit_length() - 1 for t in keep])
    out = (OlaConstraintFailure * 8)()
    n_out = C.c_uint32(77)
    return {"blob": blob, "keep": (keep, tabs), "ptrs": ptrs, "logs": logs, "out": out, "n_out": n_out,
            "mask": (1 << len(keep)) - 1 if mask is None else mask}


@pytest.fixture(scope="module")
def instance():
    from olavm_amd.air import miniexec as M
    traces, params, _ = M.instance(M.fibonacci(5))
    return traces, np.ascontiguousarray(params, dtype=np.uint64)


def test_symbol_is_exported_and_has_prototypes(lib):
    from olavm_amd import backend as B
    assert "ola_check_constraints" in B.EXPORTS
    f = lib.ola_check_constraints
    assert f.restype is C.c_int32
    assert f.argtypes is not None and len(f.argtypes) == 11
    assert f.argtypes[7] is C.c_uint32 and f.argtypes[9] is C.c_uint32              # table_mask, cap
    assert f.argtypes[8]._type_ is B.OlaConstraintFailure and f.argtypes[10]._type_ is C.c_uint32
    # the struct is the header's: 4 x 32 bits, 2 x 64 bits
    assert C.sizeof(B.OlaConstraintFailure) == 32 and B.OlaConstraintFailure.first_row.offset == 16
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    body = re.search(r"typedef struct OlaConstraintFailure \{(.*?)\} OlaConstraintFailure;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(uint\d+_t)\s+(\w+);", body) == [("uint32_t", "table"), ("uint32_t", "section"), ("uint32_t", "index"), ("uint32_t", "kind"),
                                                           ("uint64_t", "first_row"), ("uint64_t", "rows_failing")]
    assert [n for n, _ in B.OlaConstraintFailure._fields_] == ["table", "section", "index", "kind", "first_row", "rows_failing"]
    assert hasattr(B.Backend, "check_constraints")
    # the ABI revision did not move
    assert lib.ola_gpu_abi_version(None, None) == 7


def test_null_arguments_are_refused(lib, instance):
    from olavm_amd.backend import U64P
    traces, params = instance
    a = _args(traces)
    blob, p = a["blob"], a["blob"].ctypes.data_as(U64P)
    pr = params.ctypes.data_as(U64P)

    def call(**kw):
        v = {"airset": p, "words": blob.size, "cols": a["ptrs"], "logs": a["logs"], "out": a["out"], "cap": 8, "n_out": C.byref(a["n_out"])}
        v.update(kw)
        return lib.ola_check_constraints(None, v["airset"], v["words"], v["cols"], v["logs"], pr, None, a["mask"], v["out"], v["cap"], v["n_out"])

    for kw in ({"airset": None}, {"cols": None}, {"logs": None}, {"n_out": None}, {"out": None}):
        assert call(**kw) == OLA_E_INVALID_ARG, kw
        assert b"null pointer" in lib.ola_gpu_last_error()
    assert call(words=blob.size - 1) == OLA_E_INVALID_ARG                       # a truncated AIR-set blob
    # a table of the mask without columns
    holes = (type(a["ptrs"]))(*a["ptrs"])
    holes[3] = C.POINTER(U64P)()
    assert call(cols=holes) == OLA_E_INVALID_ARG and b"cols[t]" in lib.ola_gpu_last_error()


def test_table_mask_beyond_the_set_is_refused(lib, instance):
    from olavm_amd.backend import U64P
    traces, params = instance
    a = _args(traces)
    p = a["blob"].ctypes.data_as(U64P)
    for mask in (1 << 12, 0xFFFFFFFF, (1 << 12) | 1):
        rc = lib.ola_check_constraints(None, p, a["blob"].size, a["ptrs"], a["logs"], params.ctypes.data_as(U64P), None, mask, a["out"], 8,
                                       C.byref(a["n_out"]))
        assert rc == OLA_E_INVALID_ARG and b"table_mask" in lib.ola_gpu_last_error()


def test_a_program_that_names_a_register_beyond_n_regs_is_refused_before_a_device_is_looked_for(lib, instance):
    """the parser every entry point shares holds the constraint programs to their tables: the caller's error, device or not"""
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import U64P
    traces, params = instance
    a = _args(traces)
    table = T.ola_stark(range_bits=4, limb_bits=2).tables[0]
    ops, n_regs = table.compile()
    at = 4 + len(table.words()) - 2 * len(ops)                # the first op of table 0
    bad = a["blob"].copy()
    w0 = int(ops[0][0])
    assert int(bad[at]) == w0 and w0 & 0xff != 7             # not an emit: it writes dst
    bad[at] = (w0 & ~(0xffff << 16)) | (int(n_regs) << 16)
    p = bad.ctypes.data_as(U64P)

    def call(blob_p):
        return lib.ola_check_constraints(None, blob_p, bad.size, a["ptrs"], a["logs"], params.ctypes.data_as(U64P), None, a["mask"], a["out"], 8,
                                         C.byref(a["n_out"]))
    assert call(p) == OLA_E_INVALID_ARG and b"AIR-set blob" in lib.ola_gpu_last_error()
    flags = (C.c_uint8 * 12)()
    assert lib.ola_air_kernels_available(p, bad.size, flags, 12) == OLA_E_INVALID_ARG and b"AIR-set blob" in lib.ola_gpu_last_error()
    assert lib.ola_air_kernels_available(a["blob"].ctypes.data_as(U64P), bad.size, flags, 12) == 0
    assert a["n_out"].value == 77 and all(f.rows_failing == 0 for f in a["out"])


def test_no_cpu_fallback_without_device(lib, instance):
    """A context cannot be created without a device (ola_gpu_init answers OLA_E_NO_DEVICE): a well-formed call then reports the
    same instead of evaluating anything on the host, and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from olavm_amd.backend import U64P
    traces, params = instance
    a = _args(traces)
    rc = lib.ola_check_constraints(None, a["blob"].ctypes.data_as(U64P), a["blob"].size, a["ptrs"], a["logs"], params.ctypes.data_as(U64P), None,
                                   a["mask"], a["out"], 8, C.byref(a["n_out"]))
    assert rc == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()
    assert a["n_out"].value == 77 and all(f.rows_failing == 0 for f in a["out"])


def test_rust_binding_declares_the_struct_as_the_header_does():
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    body = re.search(r"pub struct OlaConstraintFailure \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("table", "u32"), ("section", "u32"), ("index", "u32"), ("kind", "u32"), ("first_row", "u64"),
                                                        ("rows_failing", "u64")]
    shim = open(os.path.join(ROOT, "integration", "rust", "hip_prover.rs")).read()
    assert "rc == OLA_E_QUOTIENT_DEGREE" in shim and "ola_check_constraints(" in shim
