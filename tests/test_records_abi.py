"""The records path on the CPU side.  OlaExecRecords and ola_tables_from_records / ola_tables_get / ola_tables_free / ola_prove_from_records
(include/ola_gpu.h): prototypes equal in the header, the ctypes binding and the Rust declarations, the struct's field offsets and size
from a compiled C program equal to the ctypes and the Rust layout, arguments refused before any work and the no-device answer.
OLA_TRACEGEN_RECORDS_ONLY of the native trace generator (include/ola_tracegen.h): the flag and its four accessors are declared and
bound, a records-only run builds no table and returns the Python executor's side lists for the nine examples -- bitwise operations, tape
cells, POSEIDON calls with their Poseidon-table rows, the padded listing -- next to everything the hashes-only run returns, the other
flags' output is unchanged, and the generator is clean under AddressSanitizer / UBSan (a stand-alone program)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.air import fastexec
    return fastexec.load_library()


def test_flag_and_accessors_are_declared_and_bound(lib):
    from olavm_amd.air import dump, fastexec as F
    from olavm_amd import backend as B
    tg = open(os.path.join(ROOT, "include", "ola_tracegen.h")).read()
    assert "#define OLA_TRACEGEN_RECORDS_ONLY 64u" in tg and F.OLA_TRACEGEN_RECORDS_ONLY == 64
    for value, name in ((1, "PROVE_PROGRAM_HASH"), (2, "EXPLICIT_BETAS"), (4, "REFERENCE_QUIRKS"), (8, "STEPS_ONLY"), (16, "CELLS_ONLY"), (32, "HASHES_ONLY")):
        assert "#define OLA_TRACEGEN_%s %du" % (name, value) in tg and getattr(F, "OLA_TRACEGEN_" + name) == value      # the older flags keep their bits
    for f in ("ola_tracegen_bitwise_ops", "ola_tracegen_tape_cells", "ola_tracegen_poseidon_calls", "ola_tracegen_listing_words"):
        assert "int32_t %s(const OlaTraceSet* set, " % f in tg and f in F.EXPORTS
        assert getattr(lib, f).argtypes is not None
    assert F.TAPE_CELL_WORDS == B.OLA_TAPE_CELL_WORDS == dump.TAPE_CELL_WORDS == 3
    assert F.POSEIDON_CALL_WORDS == B.OLA_POSEIDON_CALL_WORDS == dump.POSEIDON_CALL_WORDS == 5


@pytest.fixture(scope="module")
def python_side():
    """name -> (padded listing, the Python executor's side lists)"""
    from olavm_amd.air import miniexec as M
    out = {}
    for name, (make, kw) in M.EXAMPLES.items():
        prog = make()
        listing = prog.words()[0]
        listing = listing + [0] * (-len(listing) % 8)
        tree = M.StorageTree()
        if kw.get("prove_program_hash"):
            tree.set(prog.code_addr, M.program_hash(listing))
        out[name] = (listing, M.execute(prog, tree=tree)[1])
    return out


def _examples():
    from olavm_amd.air import miniexec as M
    return sorted(M.EXAMPLES)


@pytest.mark.parametrize("name", _examples())
def test_records_only_run_returns_the_python_executors_side_lists(lib, python_side, name):
    from olavm_amd import backend as B
    from olavm_amd.air import fastexec as F, miniexec as M, ola_tables as T
    make, kw = M.EXAMPLES[name]
    prog = make()
    listing, side = python_side[name]
    full, params, compress = F.instance(prog, **kw)
    none, lean_params, lean_compress, rec = F.instance(prog, records_only=True, **kw)
    assert len(none) == 12 and all(t is None for t in none)                                       # no table is built ...
    assert rec["log_n"] == [t.shape[1].bit_length() - 1 for t in full]                            # ... and every shape is the ordinary run's
    assert rec["words"].tolist() == listing and rec["code_addr"] == list(prog.code_addr)
    tags = {"AND": T.op_mask("AND"), "OR": T.op_mask("OR"), "XOR": T.op_mask("XOR")}
    fn = {"AND": lambda a, b: a & b, "OR": lambda a, b: a | b, "XOR": lambda a, b: a ^ b}
    want = np.array([[1, tags[op], a, b, fn[op](a, b)] for op, a, b in side["bitwise"]], dtype=np.uint64).reshape(-1, 5).T
    assert np.array_equal(rec["bitwise_ops"], want)
    want = np.array([[c[0], T.op_mask(c[2]), c[3]] for c in side["tape"]], dtype=np.uint64).reshape(-1, 3).T
    assert np.array_equal(rec["tape_cells"], want)
    calls, row = [], len(listing) // 8                                                            # the program chunks come first in the Poseidon table
    for c in side["psdn"]:
        calls.append((c["clk"], c["src"], c["len"], c["dst"], row))
        row += len(c["chunks"])
    assert np.array_equal(rec["psdn_calls"], np.array(calls, dtype=np.uint64).reshape(-1, 5).T)
    for (_, _, _, _, first), c in zip(calls, side["psdn"]):                                       # that numbering is the one of the Poseidon inputs
        for j, ch in enumerate(c["chunks"]):
            assert [int(x) for x in rec["psdn_inputs"][:, first + j]] == list(ch[1]) + list(ch[2])
            assert [int(x) for x in full[T.POSEIDON][4:16, first + j]] == list(ch[1]) + list(ch[2])
    # neither challenge is known yet; the bitwise one drawn from the operations is the ordinary run's
    assert lean_params == [None, None] and lean_compress[T.BITWISE] is None and lean_compress[T.PROGRAM] is None
    assert B.bitwise_beta(rec["bitwise_ops"], 2) == params[0]
    assert F.instance(prog, records_only=True, bitwise_beta=5, program_beta=6, **kw)[1] == [5, 6]
    if name == "mixed":
        assert rec["bitwise_ops"].shape[1] == 3
    if name == "tape":
        assert rec["tape_cells"].shape[1] == 6
    if name == "hash":
        assert rec["psdn_calls"].shape[1] == 1


@pytest.mark.parametrize("name", ["mixed", "tape", "hash", "storage"])
def test_the_other_flags_give_what_they_gave(lib, name):
    """what the hashes-only run returns is part of the records-only run's answer, word for word, and the hashes-only run still builds the
    bitwise, Poseidon-chunk, tape, SCCALL and program-chunk tables of the ordinary run"""
    from olavm_amd.air import fastexec as F, miniexec as M, ola_tables as T
    make, kw = M.EXAMPLES[name]
    prog = make()
    full, params, compress = F.instance(prog, **kw)
    lean, lean_params, _, hrec = F.instance(prog, hashes_only=True, **kw)
    rec = F.instance(prog, records_only=True, **kw)[3]
    built = (T.BITWISE, T.POSEIDON_CHUNK, T.TAPE, T.SCCALL, T.PROG_CHUNK)
    for t in range(12):
        assert np.array_equal(lean[t], full[t]) if t in built else lean[t] is None, t
    assert lean_params == [params[0], None]
    assert set(hrec) < set(rec)
    for k, v in hrec.items():
        assert np.array_equal(rec[k], v), k
    for mode in ("steps_only", "cells_only"):
        part = F.instance(prog, **{mode: True}, **kw)
        assert part[1] == params and all(a is None or np.array_equal(a, b) for a, b in zip(part[0], full))


def test_records_only_generator_is_clean_under_the_sanitizers(lib, tmp_path):
    """a stand-alone host program over tracegen.cpp: one program with tape, storage, hash and bitwise instructions, with and without
    OLA_TRACEGEN_RECORDS_ONLY"""
    exe = str(tmp_path / "host_tracegen_records")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "host_tracegen_records.cpp"), os.path.join(ROOT, "olavm_amd", "csrc", "host", "tracegen.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr


# ---- OlaExecRecords and the records entry points of include/ola_gpu.h
RECORD_ARGS = {"ola_tables_from_records": ["ctx", "rec", "out"],
               "ola_tables_get": ["set", "ptrs", "log_n", "params", "compress"],
               "ola_tables_free": ["set"],
               "ola_prove_from_records": ["ctx", "airset", "airset_words", "rec", "out", "cap", "out_len"]}


@pytest.fixture(scope="module")
def gpu_lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


def test_record_entry_points_are_declared_alike(gpu_lib):
    import ctypes as C
    from olavm_amd import backend as B
    from tests.test_tablegen_abi import _header_args, _rust_args
    host = open(os.path.join(ROOT, "include", "ola_host.hpp")).read()
    prover = open(os.path.join(ROOT, "integration", "rust", "hip_prover.rs")).read()
    for name, args in RECORD_ARGS.items():
        assert name in B.EXPORTS
        f = getattr(gpu_lib, name)
        assert f.restype is C.c_int32 and len(f.argtypes) == len(args)
        h, r = _header_args(name), _rust_args(name)
        assert [a.split()[-1].lstrip("*").split("[")[0] for a in h] == [a.split(":")[0] for a in r] == args, name
    assert "ola_prove_from_records(g.ctx(), airset.data(), airset.size(), &rec, out.data(), out.size(), &len)" in host
    assert "pub fn prove_from_records<" in prover and "ola_prove_from_records(c, words.as_ptr(), words.len()," in prover
    assert hasattr(B.Backend, "tables_from_records") and hasattr(B.Backend, "prove_from_records")
    assert gpu_lib.ola_gpu_abi_version(None, None) == 7          # additions that change no existing struct keep the revision
    hdr = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    for name, bit in (("REFERENCE_QUIRKS", 1), ("ZERO_FILLER", 2), ("RESULT_LINE", 4), ("EXPLICIT_BETAS", 8)):
        assert "#define OLA_RECORDS_%s %du" % (name, bit) in hdr and "pub const OLA_RECORDS_%s: u32 = %d;" % (name, bit) in rs
        assert getattr(B, "OLA_RECORDS_" + name) == bit


def test_exec_records_layout_is_the_same_in_c_ctypes_and_rust(tmp_path):
    """field offsets and size from a compiled C program against the ctypes struct; the Rust struct is repr(C) with the same fields in the
    same order and types of the same width"""
    import ctypes as C
    import re
    from olavm_amd import backend as B
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ola_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct OlaExecRecords \{(.*?)\} OlaExecRecords;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [d.split()[-1].lstrip("*").split("[")[0] for d in decls]
    assert names[0] == "size" and decls[0] == "uint32_t size"
    assert names == [f[0] for f in B.OlaExecRecords._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ola_gpu.h"\nint main(void) {\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(OlaExecRecords, %s));\n' % (n, n) for n in names) +
                   '    printf("sizeof %zu\\n", sizeof(OlaExecRecords));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for n in names:
        assert int(got[n]) == getattr(B.OlaExecRecords, n).offset, n
    assert int(got["sizeof"]) == C.sizeof(B.OlaExecRecords) == 264
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\n#\[derive\(Clone, Copy\)\]\npub struct OlaExecRecords \{(.*?)\n\}", rs, flags=re.S).group(1)
    rfields = [tuple(x.strip() for x in f.replace("pub ", "").split(":")) for f in rbody.split(",") if f.strip()]
    width = {"uint32_t": "u32", "uint64_t": "u64", "const uint64_t*": "*const u64"}
    want = []
    for d in decls:
        ctype, name = d.rsplit(" ", 1)
        want.append((name.split("[")[0], "[u64; 4]" if name.endswith("[4]") else width[ctype]))
    assert rfields == want


def test_record_calls_validate_before_they_work(gpu_lib):
    import ctypes as C
    import torch
    from olavm_amd import backend as B
    OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
    rec = B.OlaExecRecords()
    rec.size = C.sizeof(B.OlaExecRecords)
    rec.cpu_log_n, rec.prog_log_n, rec.range_bits, rec.limb_bits = 3, 3, 4, 2
    handle, need = C.c_void_p(123), C.c_size_t(0)
    blob = (C.c_uint64 * 4)()
    short, unknown, wide = B.OlaExecRecords(), B.OlaExecRecords(), B.OlaExecRecords()
    for r in (short, unknown, wide):
        C.memmove(C.byref(r), C.byref(rec), C.sizeof(rec))
    short.size, unknown.flags, wide.psdn_stride = C.sizeof(rec) - 8, 16, 8           # an older struct; a flag nobody defined; rows without buffers
    bad = [lambda: gpu_lib.ola_tables_from_records(None, None, C.byref(handle)),
           lambda: gpu_lib.ola_tables_from_records(None, C.byref(rec), None),
           lambda: gpu_lib.ola_tables_from_records(None, C.byref(short), C.byref(handle)),
           lambda: gpu_lib.ola_tables_from_records(None, C.byref(unknown), C.byref(handle)),
           lambda: gpu_lib.ola_tables_from_records(None, C.byref(wide), C.byref(handle)),
           lambda: gpu_lib.ola_prove_from_records(None, None, 0, C.byref(rec), None, 0, C.byref(need)),
           lambda: gpu_lib.ola_prove_from_records(None, blob, 4, C.byref(rec), None, 0, None),
           lambda: gpu_lib.ola_prove_from_records(None, blob, 4, C.byref(short), None, 0, C.byref(need)),
           lambda: gpu_lib.ola_tables_get(None, None, None, None, None)]
    for i, f in enumerate(bad):
        assert f() == OLA_E_INVALID_ARG, i
        assert b"invalid argument" in gpu_lib.ola_gpu_last_error()
    assert handle.value is None                                                       # a refused call hands out no set
    # well-formed records without a context: the answer the header gives for a call that would do work
    want, text = (OLA_E_INVALID_ARG, b"ctx is NULL") if torch.cuda.is_available() else (OLA_E_NO_DEVICE, b"no HIP device")
    for rcode in (gpu_lib.ola_tables_from_records(None, C.byref(rec), C.byref(handle)),
                  gpu_lib.ola_prove_from_records(None, blob, 4, C.byref(rec), None, 0, C.byref(need))):
        assert rcode == want and text in gpu_lib.ola_gpu_last_error()
    assert gpu_lib.ola_tables_free(None) == 0                                         # like free(NULL)
