"""FriReductionStrategy::reduction_arity_bits for all three variants (plonky2 fri/reduction_strategies.rs:27-164), without a device.

Three things agree on every entry of tests/golden/ref_fri_plans.json: the fixture (the reference's own source, interpreted by
tools/rust_air_eval.py --fri-plans), ola_fri_reduction_arity_bits (olavm_amd/csrc/fri_plan.h), and a restatement written for the
tests (tests/fri_plan_reference.py).  The fixture covers degree_bits 0..26, rate_bits 1..4, 10 / 28 / 84 queries, MinSize with None
and 1..4, ConstantArityBits and Fixed lists.  Where the reference is present a part of the fixture is derived again here (the whole of
it takes minutes: `tools/rust_air_eval.py --fri-plans --check`): the default rate and query count at every degree under MinSize(None)
and MinSize(Some(3)), every other entry up to degree_bits 12.

Then: the arguments the two entry points refuse, the setter's answer without a device, the prototypes in the header, in ctypes and
in the Rust declarations, and tests/host_fri_plan_check.cpp -- the planner in a program of its own, built plain and with
-fsanitize=address,undefined and run directly."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from tests import fri_plan_reference as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_fri_plans.json")
OLA_E_INVALID_ARG, OLA_E_NO_DEVICE = -1, -2
CONSTANT, FIXED, MIN_SIZE = 0, 1, 2

# the table of the change's description: degree_bits -> (MinSize(None), its size, ConstantArityBits(4, 5), its size) at rate_bits 3,
# 28 queries, in relative_proof_size units
ISSUE_TABLE = {
    6: ([], 256, [4], 2704), 9: ([], 2048, [4], 3152), 10: ([3], 2752, [4, 4], 5840), 12: ([4], 4384, [4, 4], 6336),
    13: ([3, 3], 5328, [4, 4], 6624), 15: ([4, 3], 7072, [4, 4, 4], 9776), 16: ([4, 4], 8192, [4, 4, 4], 10144),
    18: ([4, 3, 3], 10096, [4, 4, 4, 4], 13456), 20: ([3, 3, 3, 3], 12448, [4, 4, 4, 4], 14400),
    22: ([4, 4, 3, 3], 14576, [4, 4, 4, 4, 4], 17936), 24: ([4, 3, 3, 3, 3], 17152, [4, 4, 4, 4, 4], 19104)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from olavm_amd.backend import load_library
    return load_library()


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


def entries(fx):
    """(strategy entry, rate_bits, num_queries, degree_bits, plan)"""
    for e in fx["plans"]:
        for db, plan in zip(fx["degree_bits"], e["reduction_arity_bits"]):
            yield e["strategy"], e["rate_bits"], e["num_queries"], db, plan


def test_fixture_covers_what_it_should(fixture):
    assert fixture["degree_bits"] == list(range(27)) and fixture["cap_height"] == 4
    seen = {(json.dumps(e["strategy"]), e["rate_bits"], e["num_queries"]) for e in fixture["plans"]}
    for arg in (None, 1, 2, 3, 4):
        for rb in (1, 2, 3, 4):
            for nq in (10, 28, 84):
                assert (json.dumps(["MinSize", [arg]]), rb, nq) in seen
    for rb in (1, 2, 3, 4):
        assert (json.dumps(["ConstantArityBits", [4, 5]]), rb, 28) in seen
    for v in ([], [1, 1], [4, 3, 3], [1, 4, 2, 3]):
        assert any(s == json.dumps(["Fixed", [v]]) for s, _, _ in seen)
    assert all(plan is not None and plan != "skipped" for *_, plan in entries(fixture))


def test_library_restatement_and_fixture_agree_on_every_entry(lib, fixture):
    from olavm_amd.backend import fri_reduction_arity_bits
    count = 0
    for strat, rb, nq, db, plan in entries(fixture):
        strategy, over = FP.strategy_of(strat)
        cfg = dict(over, rate_bits=rb, num_query_rounds=nq, cap_height=fixture["cap_height"])
        assert FP.arity_bits(strategy, db, **cfg) == plan, ("restatement", strat, rb, nq, db)
        assert fri_reduction_arity_bits(strategy, db, **cfg) == plan, ("library", strat, rb, nq, db)
        count += 1
    assert count >= 27 * (5 * 12 + 4 + 4)


def test_the_table_of_the_description_comes_out_of_the_fixture(fixture):
    plans = {}
    for strat, rb, nq, db, plan in entries(fixture):
        if (rb, nq) == (3, 28) and strat in (["MinSize", [None]], ["ConstantArityBits", [4, 5]]):
            plans[(strat[0], db)] = plan
    for db, (ms, ms_size, ca, ca_size) in ISSUE_TABLE.items():
        assert plans[("MinSize", db)] == ms and plans[("ConstantArityBits", db)] == ca, db
        assert FP.relative_proof_size(db, 3, 28, ms) == ms_size and FP.relative_proof_size(db, 3, 28, ca) == ca_size, db
    for db in (6, 7, 8, 9):
        assert plans[("MinSize", db)] == [] and plans[("ConstantArityBits", db)] == [4]
    # MinSize(Some(3)): runs of 3s
    for strat, rb, nq, db, plan in entries(fixture):
        if strat == ["MinSize", [3]] and (rb, nq) == (3, 28):
            assert set(plan) <= {3}, (db, plan)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
def test_fixture_is_what_the_reference_source_computes(fixture):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rust_air_eval as X
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)
    try:
        def keep(strategy, db, rb, nq):
            return db <= 12 or ((rb, nq) == (3, 28) and strategy in (["MinSize", [None]], ["MinSize", [3]]))
        again = X.fri_plans(REF, keep)
    finally:
        sys.setrecursionlimit(old)
    assert [(e["strategy"], e["rate_bits"], e["num_queries"]) for e in again["plans"]] == [(e["strategy"], e["rate_bits"], e["num_queries"]) for e in fixture["plans"]]
    derived = 0
    for a, b in zip(again["plans"], fixture["plans"]):
        for db, x, y in zip(fixture["degree_bits"], a["reduction_arity_bits"], b["reduction_arity_bits"]):
            if x != "skipped":
                assert x == y, (a["strategy"], a["rate_bits"], a["num_queries"], db)
                derived += 1
    assert derived >= 13 * len(fixture["plans"]) + 2 * 14


def plan_call(lib, strategy, args, n, degree_bits=12, cap=64, cfg=None):
    arr = (C.c_uint32 * max(1, len(args)))(*args) if args is not None else None
    out, n_out = (C.c_uint32 * 64)(), C.c_uint32(777)
    rc = lib.ola_fri_reduction_arity_bits(cfg, strategy, arr, n, degree_bits, out, cap, C.byref(n_out))
    return rc, [out[i] for i in range(min(n_out.value, 64))] if rc == 0 else None, n_out.value


def test_bad_arguments_are_refused_by_both_entry_points(lib):
    bad = [(FIXED, [4, 0, 3], 3), (FIXED, [5], 1), (FIXED, [1] * 33, 33), (MIN_SIZE, [3, 3], 2), (MIN_SIZE, [0], 1), (MIN_SIZE, [5], 1),
           (3, [], 0), (0xFFFFFFFF, [], 0), (CONSTANT, [4], 1), (FIXED, None, 2)]
    for strategy, args, n in bad:
        rc, _, n_out = plan_call(lib, strategy, args, n)
        assert rc == OLA_E_INVALID_ARG and n_out == 777, (strategy, args, n)
        # the setter validates before it looks for a context or a device
        arr = (C.c_uint32 * max(1, len(args)))(*args) if args is not None else None
        assert lib.ola_gpu_set_fri_reduction(None, strategy, arr, n) == OLA_E_INVALID_ARG, (strategy, args, n)
        assert b"no HIP device" not in lib.ola_gpu_last_error()
    # what is fine: the boundaries, and the defaults for cfg == NULL
    assert plan_call(lib, FIXED, [1] * 32, 32) == (0, [1] * 32, 32)
    assert plan_call(lib, FIXED, [], 0) == (0, [], 0) and plan_call(lib, FIXED, None, 0) == (0, [], 0)
    assert plan_call(lib, MIN_SIZE, [4], 1, degree_bits=18) == (0, [4, 3, 3], 3) and plan_call(lib, MIN_SIZE, [], 0, degree_bits=18) == (0, [4, 3, 3], 3)
    assert plan_call(lib, CONSTANT, [], 0, degree_bits=18) == (0, [4, 4, 4, 4], 4)
    # a buffer that is too small: the length is still reported
    rc, _, n_out = plan_call(lib, MIN_SIZE, [], 0, degree_bits=18, cap=2)
    assert (rc, n_out) == (OLA_E_INVALID_ARG, 3)
    assert lib.ola_fri_reduction_arity_bits(None, MIN_SIZE, None, 0, 18, None, 0, None) == OLA_E_INVALID_ARG
    assert plan_call(lib, MIN_SIZE, [], 0, degree_bits=33)[0] == OLA_E_INVALID_ARG
    # a configuration that is none
    from olavm_amd.backend import OlaGpuConfig
    assert plan_call(lib, MIN_SIZE, [], 0, cfg=C.byref(OlaGpuConfig(-1, None, 0, 4, 16, 4, 5, 28, 2, 0)))[0] == OLA_E_INVALID_ARG


def test_setter_without_a_context(lib):
    """valid arguments and ctx == NULL: OLA_E_NO_DEVICE on a machine without a HIP device (there is no CPU fallback), OLA_E_INVALID_ARG
    on one with a device"""
    import torch
    rc = lib.ola_gpu_set_fri_reduction(None, MIN_SIZE, None, 0)
    if torch.cuda.is_available():
        assert rc == OLA_E_INVALID_ARG and b"ctx is NULL" in lib.ola_gpu_last_error()
    else:
        assert rc == OLA_E_NO_DEVICE and b"no HIP device" in lib.ola_gpu_last_error()


def test_prototypes_in_header_ctypes_and_rust(lib):
    from olavm_amd import backend as B
    header = open(os.path.join(ROOT, "include", "ola_gpu.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "ola_gpu_sys.rs")).read()
    for name, nargs in (("ola_gpu_set_fri_reduction", 4), ("ola_fri_reduction_arity_bits", 8)):
        assert name in B.EXPORTS
        f = getattr(lib, name)
        assert f.restype is C.c_int32 and f.argtypes is not None and len(f.argtypes) == nargs
    proto = re.search(r"int32_t ola_gpu_set_fri_reduction\((.*?)\);", header, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")] == ["OlaCtx* ctx", "uint32_t strategy", "const uint32_t* args", "uint32_t n"]
    proto = re.search(r"int32_t ola_fri_reduction_arity_bits\((.*?)\);", header, flags=re.S).group(1)
    assert [re.sub(r"\s+", " ", p).strip() for p in proto.split(",")] == [
        "const OlaGpuConfig* cfg", "uint32_t strategy", "const uint32_t* args", "uint32_t n", "uint32_t degree_bits", "uint32_t* out", "uint32_t cap",
        "uint32_t* n_out"]
    decl = re.search(r"pub fn ola_gpu_set_fri_reduction\((.*?)\) -> i32;", rs, flags=re.S).group(1)
    assert [p.strip() for p in decl.split(",")] == ["ctx: *mut OlaCtx", "strategy: u32", "args: *const u32", "n: u32"]
    decl = re.search(r"pub fn ola_fri_reduction_arity_bits\((.*?)\) -> i32;", rs, flags=re.S).group(1)
    assert [p.strip() for p in decl.split(",")] == ["cfg: *const OlaGpuConfig", "strategy: u32", "args: *const u32", "n: u32", "degree_bits: u32",
                                                    "out: *mut u32", "cap: u32", "n_out: *mut u32"]
    for name, val in (("OLA_FRI_CONSTANT_ARITY_BITS", 0), ("OLA_FRI_FIXED", 1), ("OLA_FRI_MIN_SIZE", 2)):
        assert re.search(r"#define %s %du\b" % (name, val), header) and "pub const %s: u32 = %d;" % (name, val) in rs
        assert B.FRI_STRATEGIES[name[len("OLA_FRI_"):].lower()] == val
    # the ABI revision did not move, the history says what was added to it, and no struct grew
    assert lib.ola_gpu_abi_version(None, None) == 7
    size = C.c_size_t()
    lib.ola_gpu_abi_version(None, C.byref(size))
    assert size.value == C.sizeof(B.OlaGpuConfig)
    history = header[header.index("/* ABI revision of this header."):header.index("#define OLA_GPU_ABI_VERSION 7")]
    assert "ola_gpu_set_fri_reduction" in history and "ola_fri_reduction_arity_bits" in history
    # the shim maps all three variants and keys its cached context by the strategy
    shim = open(os.path.join(ROOT, "integration", "rust", "hip_prover.rs")).read()
    for needle in ("FriReductionStrategy::Fixed(", "FriReductionStrategy::MinSize(", "FriReductionStrategy::ConstantArityBits(", "ola_gpu_set_fri_reduction(",
                   "plan_args: [u32; 32]"):
        assert needle in shim, needle
    assert "ConstantArityBits only" not in shim


def test_python_layer_refuses_what_it_cannot_express():
    from olavm_amd.backend import fri_reduction_arity_bits, OlaGpuError
    with pytest.raises(ValueError):
        fri_reduction_arity_bits(("largest",), 12)
    with pytest.raises(OlaGpuError) as e:
        fri_reduction_arity_bits(("fixed", [4, 5]), 12)
    assert e.value.code == OLA_E_INVALID_ARG and "1..4" in str(e.value)
    assert fri_reduction_arity_bits(None, 12) == [4, 4] and fri_reduction_arity_bits("min_size", 12) == [4]


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_planner_in_a_program_of_its_own(tmp_path, flags):
    """tests/host_fri_plan_check.cpp has its own main: the planner and the verifier's host stage compile with g++ alone, and the
    sanitized build runs directly (no Python process loads sanitized code)."""
    exe = tmp_path / "host_fri_plan_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags, "-o", str(exe),
                           os.path.join(ROOT, "tests", "host_fri_plan_check.cpp")])
    fx = json.load(open(FIXTURE))
    number = {"constant_arity_bits": CONSTANT, "fixed": FIXED, "min_size": MIN_SIZE}
    lines = []
    for strat, rb, nq, db, plan in entries(fx):
        strategy, over = FP.strategy_of(strat)
        args = list(strategy[1]) if strategy[0] == "fixed" else ([] if len(strategy) < 2 or strategy[1] is None else [strategy[1]])
        lines.append(" ".join(map(str, [number[strategy[0]], len(args), *args, over.get("fri_arity_bits", 4), over.get("fri_final_poly_bits", 5), rb, nq,
                                        fx["cap_height"], db, len(plan), *plan])))
    plans = tmp_path / "plans.txt"
    plans.write_text("\n".join(lines) + "\n")
    # the committed MinSize proof and the challenges the reference derived from it (tests/make_ref_verdict_minsize.py)
    from olavm_amd.air import ola_tables as T
    ref_dir = os.path.join(ROOT, "tests", "golden", "ref_verified")
    rec = json.load(open(os.path.join(ref_dir, "wide_program_blake3_minsize.json")))
    assert rec["verify_proof"] == "Ok(())" and rec["reduction_strategy"] == "MinSize(None)" and rec["fri_layers"] == [0, 0, 3, 0, 2, 1, 0, 0, 0, 0, 0, 0]
    blob = [int(x) for x in T.ola_stark().blob()]
    w = ["hasher", 1, "proof", os.path.join(ref_dir, "wide_program_blake3_minsize.proof"), "blob", len(blob)] + blob
    w += ["tables", len(rec["challenges"]["stark_challenges"])]
    for s in rec["challenges"]["stark_challenges"]:
        f = s["fri_challenges"]
        w += s["stark_zeta"] + f["fri_alpha"] + [len(f["fri_betas"])] + [x for b in f["fri_betas"] for x in b]
        w += [f["fri_pow_response"], len(f["fri_query_indices"])] + f["fri_query_indices"]
    case = tmp_path / "proof_case.txt"
    case.write_text(" ".join(str(x) for x in w) + "\n")
    r = subprocess.run([str(exe), str(plans), str(case)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d entries agree, the proof is accepted under its plan" % len(lines) in r.stdout


def test_the_record_belongs_to_the_committed_proof():
    import hashlib
    ref_dir = os.path.join(ROOT, "tests", "golden", "ref_verified")
    raw = open(os.path.join(ref_dir, "wide_program_blake3_minsize.proof"), "rb").read()
    rec = json.load(open(os.path.join(ref_dir, "wide_program_blake3_minsize.json")))
    assert (rec["proof_bytes"], rec["proof_sha256"]) == (len(raw), hashlib.sha256(raw).hexdigest())
    assert rec["write_all_proof_reproduces_the_bytes"] is True and rec["verify_proof"] == "Ok(())"
    assert rec["verify_proof_under_constant_arity_bits_4_5"].startswith("Err validate_shape.rs")
    assert len(rec["tampered"]) == 19 and all(t["reference"].startswith("Err ") for t in rec["tampered"])
    # strictly shorter than the same instance's proof under the default strategy, both lengths on record
    default = json.load(open(os.path.join(ref_dir, "wide_program_blake3.json")))
    assert (len(raw), default["proof_bytes"]) == (539288, 586616)
    for shape, layers in zip(rec["trace_shapes"], rec["fri_layers"]):
        assert len(FP.arity_bits(("min_size", None), shape[1].bit_length() - 1)) == layers
