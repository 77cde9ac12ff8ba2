"""CPU-side checks of ola_verify_all_proof / ola_verify_opening (include/ola_gpu.h): the symbols are exported and declared with
prototypes in olavm_amd/backend.py; header, ctypes struct and Rust declaration agree on the layout of OlaVerifyReport and on the
OLA_VERIFY_* reasons; the arguments are validated before anything touches a device, and without a device the calls say so -- there is
no CPU fallback; the ABI revision is still 7."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
FIELDS = [("uint32_t", "accepted"), ("uint32_t", "reason"), ("int32_t", "table"), ("int32_t", "query"), ("int32_t", "oracle_or_layer"),
          ("uint32_t", "merkle_jobs"), ("uint32_t", "query_jobs"), ("uint32_t", "kernel_launches"), ("double", "host_ms"), ("double", "device_ms"),
          ("char", "message")]
RUST = {"uint32_t": "u32", "int32_t": "i32", "double": "f64", "char": "[c_char; 96]"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "ola_gpu.h")).read()


def test_symbols_are_exported_and_have_prototypes(lib, header):
    from olavm_amd import backend as B
    for name, nargs in (("ola_verify_all_proof", 7), ("ola_verify_opening", 9)):
        assert name in B.EXPORTS
        f = getattr(lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None and len(f.argtypes) == nargs
        assert f.argtypes[-1]._type_ is B.OlaVerifyReport
    assert lib.ola_verify_opening.argtypes[7]._type_ is B.OlaChallenger
    assert hasattr(B.Backend, "verify_all_proof") and hasattr(B.Backend, "verify_opening")
    # the ABI revision did not move, and the history comment says what was added to it
    assert lib.ola_gpu_abi_version(None, None) == 7
    history = header[header.index("/* ABI revision of this header."):header.index("#define OLA_GPU_ABI_VERSION 7")]
    assert "OlaVerifyReport" in history and "ola_verify_all_proof" in history and "ola_verify_opening" in history
    # the header says what a word >= p is
    assert "A field word >= p anywhere in the proof is refused as OLA_VERIFY_MALFORMED" in header


def test_header_ctypes_and_rust_agree_on_the_struct_and_the_reasons(header):
    from olavm_amd import backend as B
    body = re.search(r"typedef struct OlaVerifyReport \{(.*?)\} OlaVerifyReport;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|int32_t|double|char)\s+(\w+)(\[96\])?;", body)
    assert [(t, n) for t, n, _ in fields] == FIELDS and [bool(a) for _, _, a in fields] == [False] * 10 + [True]
    size = {"uint32_t": 4, "int32_t": 4, "double": 8, "char": 1}
    off, want = 0, {}
    for t, n, arr in fields:
        off = (off + size[t] - 1) // size[t] * size[t]
        want[n] = off
        off += size[t] * (96 if arr else 1)
    assert {n: getattr(B.OlaVerifyReport, n).offset for _, n in FIELDS} == want
    assert C.sizeof(B.OlaVerifyReport) == off == 144
    assert [n for n, _ in B.OlaVerifyReport._fields_] == [n for _, n in FIELDS]
    # the reasons: consecutive from 0, the same names in the backend and in the Rust declarations
    reasons = [(n, int(v)) for n, v in re.findall(r"#define OLA_VERIFY_(\w+) (\d+)u", header)]
    assert [v for _, v in reasons] == list(range(len(reasons))) and tuple(n for n, _ in reasons) == B.VERIFY_REASONS
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    for n, v in reasons:
        assert "pub const OLA_VERIFY_%s: u32 = %d;" % (n, v) in rs
    m = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct OlaVerifyReport \{(.*?)\n\}", rs, flags=re.S)
    assert m, "OlaVerifyReport must be #[repr(C)]"
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", m.group(1)) == [(n, RUST[t]) for t, n in FIELDS]
    # the prototypes
    proto = re.search(r"int32_t ola_verify_all_proof\((.*?)\);", header, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")] == [
        "OlaCtx* ctx", "const uint64_t* airset", "size_t airset_words", "const uint64_t* params", "const uint8_t* proof", "size_t proof_len",
        "OlaVerifyReport* report"]
    proto = re.search(r"int32_t ola_verify_opening\((.*?)\);", header, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")] == [
        "OlaCtx* ctx", "const uint64_t* caps", "const uint32_t num_polys[3]", "uint32_t degree_bits", "uint32_t num_permutation_zs",
        "const uint8_t* proof", "size_t proof_len", "OlaChallenger* challenger", "OlaVerifyReport* report"]
    decl = re.search(r"pub fn ola_verify_all_proof\((.*?)\) -> i32;", rs, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")] == [
        "ctx: *mut OlaCtx", "airset: *const u64", "airset_words: usize", "params: *const u64", "proof: *const u8", "proof_len: usize",
        "report: *mut OlaVerifyReport"]
    decl = re.search(r"pub fn ola_verify_opening\((.*?)\) -> i32;", rs, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")] == [
        "ctx: *mut OlaCtx", "caps: *const u64", "num_polys: *const u32", "degree_bits: u32", "num_permutation_zs: u32", "proof: *const u8",
        "proof_len: usize", "challenger: *mut OlaChallenger", "report: *mut OlaVerifyReport"]
    shim = open(os.path.join(ROOT, "integration", "rust", "hip_prover.rs")).read()
    assert "ola_verify_all_proof(" in shim


@pytest.fixture(scope="module")
def call(lib):
    from olavm_amd.air import ola_tables as T
    from olavm_amd.backend import U64P, OlaVerifyReport
    blob = np.ascontiguousarray(T.ola_stark().blob(), dtype=np.uint64)
    proof = open(os.path.join(ROOT, "tests", "golden", "ref_verified", "wide_program.proof"), "rb").read()
    rep = OlaVerifyReport()
    rep.reason, rep.table = 77, 55

    def f(**kw):
        v = {"airset": blob.ctypes.data_as(U64P), "words": blob.size, "proof": proof, "len": len(proof), "report": C.byref(rep)}
        v.update(kw)
        return lib.ola_verify_all_proof(None, v["airset"], v["words"], None, v["proof"], v["len"], v["report"])
    f.rep = rep
    return f


def test_arguments_are_checked_before_a_device_is_looked_for(lib, call):
    from olavm_amd.backend import OlaChallenger, OlaVerifyReport
    for kw in ({"airset": None}, {"proof": None}, {"report": None}):
        assert call(**kw) == OLA_E_INVALID_ARG and b"null pointer" in lib.ola_gpu_last_error(), kw
    ch, rep = OlaChallenger(), OlaVerifyReport()
    caps = np.zeros(3 * 16 * 4, dtype=np.uint64)
    from olavm_amd.backend import U64P
    widths = (C.c_uint32 * 3)(3, 2, 2)
    for args in ((None, widths, b"x", C.byref(ch), C.byref(rep)), (caps.ctypes.data_as(U64P), None, b"x", C.byref(ch), C.byref(rep)),
                 (caps.ctypes.data_as(U64P), widths, None, C.byref(ch), C.byref(rep)), (caps.ctypes.data_as(U64P), widths, b"x", None, C.byref(rep)),
                 (caps.ctypes.data_as(U64P), widths, b"x", C.byref(ch), None)):
        assert lib.ola_verify_opening(None, args[0], args[1], 5, 0, args[2], 1, args[3], args[4]) == OLA_E_INVALID_ARG
        assert b"null pointer" in lib.ola_gpu_last_error()
    assert (call.rep.reason, call.rep.table) == (77, 55)             # nothing was written by the refused calls


def test_no_cpu_fallback_without_device(lib, call):
    """A context cannot be created without a device: a well-formed call then reports that instead of verifying anything on the host,
    and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert call() == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()
    assert (call.rep.reason, call.rep.table, call.rep.accepted) == (77, 55, 0)
    from olavm_amd.backend import OlaChallenger, OlaVerifyReport, U64P
    ch, rep = OlaChallenger(), OlaVerifyReport()
    caps = np.zeros(3 * 16 * 4, dtype=np.uint64)
    assert lib.ola_verify_opening(None, caps.ctypes.data_as(U64P), (C.c_uint32 * 3)(3, 2, 2), 5, 0, b"x", 1, C.byref(ch), C.byref(rep)) == OLA_E_NO_DEVICE
