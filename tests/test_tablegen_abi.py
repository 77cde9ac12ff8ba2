"""CPU-side checks of ola_generate_rc_trace / ola_generate_bitwise_trace / ola_generate_prog_trace (include/ola_gpu.h): the symbols
are exported and declared -- in the header, in olavm_amd/backend.py and in integration/rust/ola_gpu_sys.rs, with equal arity --, the
column indices the kernels use are the ones of olavm_amd/air/ola_tables.py, arguments are validated before anything touches a
device, the sizing call answers without one, and a call that would do work says that there is no device (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
NAMES = ("ola_generate_rc_trace", "ola_generate_bitwise_trace", "ola_generate_prog_trace")
ARITY = {"ola_generate_rc_trace": 7, "ola_generate_bitwise_trace": 8, "ola_generate_prog_trace": 6}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def _header_args(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ola_gpu.h")).read(), flags=re.S)
    m = re.search(r"int32_t %s\((.*?)\);" % name, hdr, flags=re.S)
    assert m, name + " is not declared in include/ola_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


def _rust_args(name):
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, rs, flags=re.S)
    assert m, name + " is not declared in integration/rust/ola_gpu_sys.rs"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_are_exported_and_declared_with_equal_arity(lib):
    from olavm_amd import backend as B
    for name in NAMES:
        assert name in B.EXPORTS
        f = getattr(lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None
        h, r = _header_args(name), _rust_args(name)
        assert len(h) == len(r) == len(f.argtypes) == ARITY[name], (name, h, r)
        # the same names in the same order on both sides of the boundary
        assert [a.split()[-1].lstrip("*") for a in h] == [a.split(":")[0] for a in r], name
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    assert "#define OLA_TABLEGEN_REFERENCE_QUIRKS 1u" in hdr and "pub const OLA_TABLEGEN_REFERENCE_QUIRKS: u32 = 1;" in rs
    assert B.OLA_TABLEGEN_REFERENCE_QUIRKS == 1
    for method in ("generate_rc_trace", "generate_bitwise_trace", "generate_prog_trace"):
        assert hasattr(B.Backend, method)
    assert callable(B.bitwise_beta)
    assert lib.ola_gpu_abi_version(None, None) == 7          # additions that change no struct keep the revision


def test_column_header_of_the_kernels_is_the_table_description():
    """olavm_amd/csrc/tablegen_columns.h is committed (tablegen.hip is compiled before anything is generated): it must be what
    olavm_amd/air/dump.py prints from ola_tables.py today, and tablegen.hip must take its indices from there."""
    from olavm_amd.air import dump, ola_tables as T
    text = open(os.path.join(ROOT, dump.TABLEGEN_COLUMNS_H)).read()
    assert text == dump.tablegen_columns_header()
    assert "constexpr uint32_t RC_LIMB_HI_PERMUTED = %du;" % T.RC_LIMB_HI_PERMUTED in text
    assert "constexpr uint32_t BW_FIX_COMPRESS_PERMUTED_START = %du" % T.BW_FIX_COMPRESS_PERMUTED.start in text
    assert "constexpr uint64_t OP_MASK_XOR = %dull;" % T.op_mask("XOR") in text
    src = open(os.path.join(ROOT, "olavm_amd", "csrc", "tablegen.hip")).read()
    assert '#include "tablegen_columns.h"' in src
    assert not re.search(r"\bout \+ \(size_t\)\d+ \* n|\bout\[\(size_t\)\d+ \* n", src), "a column index was typed in"


def test_sizing_call_needs_no_context(lib):
    log_n = C.c_uint32(99)
    for n_rows, bits, want in ((0, 4, 4), (3, 4, 4), (17, 4, 5), (0, 16, 16), (1 << 16, 16, 16), ((1 << 16) + 1, 16, 17), (0, 1, 1)):
        assert lib.ola_generate_rc_trace(None, None, None, n_rows, bits, None, C.byref(log_n)) == 0 and log_n.value == want, (n_rows, bits)
    for n_ops, bits, want in ((0, 2, 6), (5, 2, 6), (65, 2, 7), (0, 8, 18), (1 << 18, 8, 18), ((1 << 18) + 1, 8, 19), (0, 1, 4)):
        assert lib.ola_generate_bitwise_trace(None, None, n_ops, bits, 0, 0, None, C.byref(log_n)) == 0 and log_n.value == want, (n_ops, bits)


def test_null_and_zero_size_arguments_are_refused(lib):
    vals = np.arange(8, dtype=np.uint64)
    out = np.full(12 * 16, 7, dtype=np.uint64)
    log_n = C.c_uint32(99)
    v, o = C.c_void_p(vals.ctypes.data), C.c_void_p(out.ctypes.data)
    bad = [
        lambda: lib.ola_generate_rc_trace(None, v, None, 8, 4, o, None),                 # nowhere to put the height
        lambda: lib.ola_generate_rc_trace(None, None, None, 8, 4, o, C.byref(log_n)),    # rows without values
        lambda: lib.ola_generate_rc_trace(None, v, None, 8, 0, o, C.byref(log_n)),       # a fixed table of one row
        lambda: lib.ola_generate_rc_trace(None, v, None, 8, 25, o, C.byref(log_n)),
        lambda: lib.ola_generate_rc_trace(None, v, None, (1 << 28) + 1, 4, o, C.byref(log_n)),
        lambda: lib.ola_generate_bitwise_trace(None, v, 1, 2, 5, 0, o, None),
        lambda: lib.ola_generate_bitwise_trace(None, None, 1, 2, 5, 0, o, C.byref(log_n)),
        lambda: lib.ola_generate_bitwise_trace(None, v, 1, 0, 5, 0, o, C.byref(log_n)),
        lambda: lib.ola_generate_bitwise_trace(None, v, 1, 13, 5, 0, o, C.byref(log_n)),
        lambda: lib.ola_generate_bitwise_trace(None, v, 1, 2, 5, 2, o, C.byref(log_n)),  # a flag nobody defined
        lambda: lib.ola_generate_prog_trace(None, None, v, 1, 5, o),
        lambda: lib.ola_generate_prog_trace(None, v, None, 1, 5, o),
        lambda: lib.ola_generate_prog_trace(None, v, v, 1, 5, None),
        lambda: lib.ola_generate_prog_trace(None, v, v, 0, 5, o),                        # a table of one row
        lambda: lib.ola_generate_prog_trace(None, v, v, 27, 5, o),
    ]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in lib.ola_gpu_last_error()
    assert np.all(out == 7)


def test_no_cpu_fallback_without_device(lib):
    """A context cannot be created without a device: a well-formed call that would do work then answers OLA_E_NO_DEVICE instead of
    filling the table on the host, and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    vals = np.arange(8, dtype=np.uint64)
    sides = np.zeros(7 * 2, dtype=np.uint64)
    out = np.full(59 * 64, 7, dtype=np.uint64)
    log_n = C.c_uint32(99)
    v, s, o = C.c_void_p(vals.ctypes.data), C.c_void_p(sides.ctypes.data), C.c_void_p(out.ctypes.data)
    for rc in (lib.ola_generate_rc_trace(None, v, None, 8, 4, o, C.byref(log_n)),
               lib.ola_generate_rc_trace(None, None, None, 0, 4, o, C.byref(log_n)),
               lib.ola_generate_bitwise_trace(None, v, 1, 2, 5, 0, o, C.byref(log_n)),
               lib.ola_generate_prog_trace(None, s, s, 1, 5, o)):
        assert rc == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()
    assert np.all(out == 7)


def test_bitwise_beta_is_the_generators_transcript(lib):
    """bitwise_beta observes the twelve limb columns at full height, as tracegen.bitwise_trace does with a transcript (miniature table)."""
    from olavm_amd.air import miniexec as M, ola_tables as T, tracegen as TG
    from olavm_amd.backend import bitwise_beta
    named = [("AND", 0xA5, 0x3C), ("XOR", 0xFF, 0x81), ("OR", 7, 0xF0)]
    fn = {"AND": lambda x, y: x & y, "OR": lambda x, y: x | y, "XOR": lambda x, y: x ^ y}
    ops = np.array([[1] * 3, [T.op_mask(n) for n, _, _ in named], [x for _, x, _ in named], [y for _, _, y in named],
                    [fn[n](x, y) for n, x, y in named]], dtype=np.uint64)
    for quirks in (False, True):
        _, beta = TG.bitwise_trace(None, 2, named, looked_by_cpu=True, transcript=M._transcript, reference_quirks=quirks)
        assert bitwise_beta(ops, 2, reference_quirks=quirks) == beta
    p = np.uint64(0xFFFFFFFF00000001)
    assert bitwise_beta(ops + np.array([[0], [0], [p], [0], [p]], dtype=np.uint64), 2) == bitwise_beta(ops, 2)
