"""ola_generate_rc_trace / ola_generate_bitwise_trace / ola_generate_prog_trace: the range-check, bitwise and program tables
completed on the device from their primary columns (include/ola_gpu.h), against
  - the reference's own generator output (tests/golden/ref_tracegen_vectors.json, ref_tracegen_bitwise.json: digests and heads),
  - olavm_amd/air/tracegen.py and miniexec.py, word for word,
  - whole proofs: the three tables regenerated in HBM and passed as resident tables give the all-host AllProof bytes,
  - ola_permuted_cols_dev and a big-integer evaluation of the compress columns at 2^22 rows."""
import hashlib
import json
import os

import numpy as np
import pytest

from olavm_amd.air import ola_tables as T, tracegen as TG
from olavm_amd.air.dsl import P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FN = {"AND": lambda x, y: x & y, "OR": lambda x, y: x | y, "XOR": lambda x, y: x ^ y}


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


def digest(t):
    return {"columns": int(t.shape[0]), "rows": int(t.shape[1]), "sha256": hashlib.sha256(np.ascontiguousarray(t, dtype="<u8").tobytes()).hexdigest()}


def to_dev(a):
    """A device copy that is COMPLETE on return: torch copies and fills on its own stream, the library works on the context's, and a
    device buffer handed to the library must be complete when the call is made (include/ola_gpu.h)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def dev_table(ncols, log_n, fill=-1):
    import torch
    t = torch.full((ncols, 1 << log_n), fill, dtype=torch.int64, device="cuda")          # every word must be overwritten
    torch.cuda.synchronize()                                                               # ... by the library, not by a late fill
    return t


def add_p(rng, a, share=0.3):
    """p added to a seeded share of the words that leave room for it (a word + p must fit 64 bits)"""
    a = np.array(a, dtype=np.uint64)
    pick = (rng.random(a.shape) < share) & (a < np.uint64((1 << 64) - P))
    return np.where(pick, a + np.uint64(P), a)


# ------------------------------------------------------------------------------------------------ inputs from rows
def rc_inputs(rows):
    vals = np.array([r[0] for r in rows], dtype=np.uint64)
    filters = np.array([[r[1 + k] for r in rows] for k in range(4)], dtype=np.uint64).reshape(4, len(rows))
    return vals, filters


def bw_inputs(named, looked_by_cpu=True):
    cols = [[int(looked_by_cpu)] * len(named), [T.op_mask(n) for n, _, _ in named], [x for _, x, _ in named], [y for _, _, y in named],
            [FN[n](x, y) for n, x, y in named]]
    return np.array(cols, dtype=np.uint64).reshape(5, len(named))


def prog_sides(t):
    ex = list(T.COL_PROG_EXEC_CODE_ADDR_RANGE) + [T.COL_PROG_EXEC_PC, T.COL_PROG_EXEC_INST, T.COL_PROG_FILTER_EXEC]
    pr = list(T.COL_PROG_CODE_ADDR_RANGE) + [T.COL_PROG_PC, T.COL_PROG_INST, T.COL_PROG_FILTER_PROG_CHUNK]
    return np.ascontiguousarray(t[ex]), np.ascontiguousarray(t[pr])


# ------------------------------------------------------------------------------------------------ the reference's generator output
def test_range_check_table_equals_the_reference_generators(be):
    v = json.load(open(os.path.join(HERE, "golden", "ref_tracegen_vectors.json")))["rangecheck"]
    vals, filters = rc_inputs([tuple(r) for r in v["rows_in"]])
    t = be.generate_rc_trace(vals, filters, range_bits=16)
    assert t.shape == (T.COL_NUM_RC, 1 << 16)
    assert digest(t) == {k: v[k] for k in ("columns", "rows", "sha256")}
    assert t[:, :8].tolist() == v["head"]


def test_bitwise_table_and_beta_equal_the_reference_generators(be):
    from olavm_amd.backend import bitwise_beta
    v = json.load(open(os.path.join(HERE, "golden", "ref_tracegen_bitwise.json")))
    ops = bw_inputs([(name, int(x), int(y)) for name, x, y in v["ops"]])
    beta = bitwise_beta(ops, 8)
    assert beta == v["beta"]
    t = be.generate_bitwise_trace(ops, beta, limb_bits=8)
    assert t.shape == (T.COL_NUM_BITWISE, 1 << 18)
    assert t[:, :ops.shape[1]].T.tolist() == v["rows_head"]
    assert digest(t) == {k: v[k] for k in ("columns", "rows", "sha256")}


# ------------------------------------------------------------------------------------------------ word for word: range check
def rc_cases():
    rng = np.random.default_rng(41)
    rows = lambda count, bits: [(int(rng.integers(0, 1 << (2 * bits))), *[int(x) for x in rng.integers(0, 2, 4)]) for _ in range(count)]
    return [(4, []), (4, rows(5, 4)), (4, rows(40, 4)),                     # miniature: no rows, a few, more than the fixed table
            (16, []), (16, rows(9, 16)), (16, rows((1 << 16) + 5, 16))]     # full size; the last one is 2^17 rows high


@pytest.mark.parametrize("case", range(6))
def test_range_check_table_word_for_word(be, case):
    range_bits, rows = rc_cases()[case]
    want = TG.generate_rc_trace(rows, range_bits)
    vals, filters = rc_inputs(rows)
    log_n = be.rc_trace_log_n(len(rows), range_bits)
    assert want.shape == (T.COL_NUM_RC, 1 << log_n)
    got = be.generate_rc_trace(vals, filters, range_bits=range_bits)
    assert np.array_equal(got, want)
    rng = np.random.default_rng(case)
    if rows:
        # words >= p, inputs on the device, the table written into HBM
        out = dev_table(T.COL_NUM_RC, log_n)
        assert be.generate_rc_trace(to_dev(add_p(rng, vals)), to_dev(add_p(rng, filters)), range_bits=range_bits, out=out) == log_n
        assert np.array_equal(to_host(out), want)
        # host inputs, device table; device inputs, host table
        out = dev_table(T.COL_NUM_RC, log_n)
        be.generate_rc_trace(add_p(rng, vals), filters, range_bits=range_bits, out=out)
        assert np.array_equal(to_host(out), want)
        assert np.array_equal(be.generate_rc_trace(to_dev(vals), to_dev(filters), range_bits=range_bits), want)
    if not any(any(r[1:]) for r in rows):
        assert np.array_equal(be.generate_rc_trace(vals, None, range_bits=range_bits), want)
    no_filters = TG.generate_rc_trace([(r[0], 0, 0, 0, 0) for r in rows], range_bits)
    assert np.array_equal(be.generate_rc_trace(vals, None, range_bits=range_bits), no_filters)


def test_an_oversize_range_check_value_is_not_refused(be):
    """val >= 2^(2 range_bits): LIMB_LO = val mod 2^range_bits, LIMB_HI = val >> range_bits (not in the fixed table: a table the AIR
    rejects, as the reference's would be), and the permuted pairs of exactly those columns."""
    range_bits, size = 4, 16
    vals = [3, 300, 255, P - 1, 17]
    n = 16
    want = np.zeros((T.COL_NUM_RC, n), dtype=np.uint64)
    want[T.RC_CPU_FILTER, :5] = 1
    want[T.RC_VAL, :5] = vals
    want[T.RC_LIMB_LO, :5] = [v % size for v in vals]
    want[T.RC_LIMB_HI, :5] = [v >> range_bits for v in vals]
    fix = list(range(size))
    want[T.RC_FIX_RANGE_CHECK_U16] = fix
    want[T.RC_LIMB_LO_PERMUTED], want[T.RC_FIX_RANGE_CHECK_U16_PERMUTED_LO] = TG.permuted_cols(want[T.RC_LIMB_LO], fix)
    want[T.RC_LIMB_HI_PERMUTED], want[T.RC_FIX_RANGE_CHECK_U16_PERMUTED_HI] = TG.permuted_cols(want[T.RC_LIMB_HI], fix)
    filters = np.zeros((4, 5), dtype=np.uint64)
    filters[0] = 1
    got = be.generate_rc_trace(np.array(vals, dtype=np.uint64), filters, range_bits=range_bits)
    assert np.array_equal(got, want)
    assert got[T.RC_LIMB_HI, 1] == 18 and got[T.RC_LIMB_HI, 3] == (P - 1) >> 4


# ------------------------------------------------------------------------------------------------ word for word: bitwise
def bw_cases():
    rng = np.random.default_rng(43)
    ops = lambda count, bits: [(("AND", "OR", "XOR")[int(rng.integers(0, 3))], int(rng.integers(0, 1 << bits)), int(rng.integers(0, 1 << bits)))
                               for _ in range(count)]
    return [(2, [], False), (2, ops(6, 8), False), (2, ops(6, 8), True), (2, ops(70, 8), False),      # 70 operations > 64 fixed rows
            (8, ops(12, 32), False), (8, ops(12, 32), True)]                                           # 32-bit operands, limb 3 live


@pytest.mark.parametrize("case", range(6))
def test_bitwise_table_word_for_word(be, case):
    limb_bits, named, quirks = bw_cases()[case]
    beta = 0x1234567 + case
    want = TG.bitwise_trace(beta, limb_bits, named, looked_by_cpu=True, reference_quirks=quirks)
    ops = bw_inputs(named)
    log_n = be.bitwise_trace_log_n(len(named), limb_bits)
    assert want.shape == (T.COL_NUM_BITWISE, 1 << log_n)
    got = be.generate_bitwise_trace(ops, beta, limb_bits=limb_bits, reference_quirks=quirks)
    assert np.array_equal(got, want)
    if named and limb_bits == 8:
        assert quirks == (not got[T.BW_OP0_LIMBS.start + 3].any())
    rng = np.random.default_rng(case)
    if named:
        out = dev_table(T.COL_NUM_BITWISE, log_n)
        assert be.generate_bitwise_trace(to_dev(add_p(rng, ops)), beta + P, limb_bits=limb_bits, reference_quirks=quirks, out=out) == log_n
        assert np.array_equal(to_host(out), want)
        assert np.array_equal(be.generate_bitwise_trace(add_p(rng, ops), beta, limb_bits=limb_bits, reference_quirks=quirks), want)
    else:
        out = dev_table(T.COL_NUM_BITWISE, log_n)
        be.generate_bitwise_trace(None, beta, limb_bits=limb_bits, out=out)
        assert np.array_equal(to_host(out), want)


def test_bitwise_rows_are_copied_as_given(be):
    """filter, tag and res are the caller's: a filter of 0 and a wrong res are written as they are (the AIR judges them)."""
    ops = bw_inputs([("AND", 0xA5, 0x3C), ("XOR", 0xFF, 0x81)], looked_by_cpu=False)
    ops[4, 1] = 0x11
    t = be.generate_bitwise_trace(ops, 99, limb_bits=2)
    assert t[:5, :2].tolist() == ops.tolist()
    assert [int(t[T.BW_RES_LIMBS.start + i, 1]) for i in range(4)] == [1, 0, 1, 0]
    b = 99
    assert int(t[T.BW_COMPRESS_LIMBS.start, 1]) == (T.op_mask("XOR") + 3 * b + 1 * b * b + 1 * b ** 3) % P


# ------------------------------------------------------------------------------------------------ word for word: program
def test_program_table_word_for_word(be):
    from olavm_amd.air import miniexec as M
    rng = np.random.default_rng(47)
    seen_long_run = False
    for prog in (M.fibonacci(5), M.fibonacci(200), M.memory_program()):
        traces, params, _ = M.instance(prog)
        want, beta = traces[10], params[1]
        listing = int(want[T.COL_PROG_FILTER_PROG_CHUNK].sum())
        seen_long_run |= int(want[T.COL_PROG_FILTER_EXEC].sum()) > listing          # the executed side exceeds the listing
        ex, pr = prog_sides(want)
        assert np.array_equal(be.generate_prog_trace(ex, pr, beta), want)
        log_n = want.shape[1].bit_length() - 1
        out = dev_table(T.NUM_PROG_COLS, log_n)
        beta_p = beta + P if beta + P < 1 << 64 else beta            # the same challenge as a word >= p, where 64 bits have room for it
        assert be.generate_prog_trace(to_dev(add_p(rng, ex)), to_dev(add_p(rng, pr)), beta_p, out=out) == log_n
        assert np.array_equal(to_host(out), want)
        out = dev_table(T.NUM_PROG_COLS, log_n)
        be.generate_prog_trace(ex, to_dev(pr), beta, out=out)
        assert np.array_equal(to_host(out), want)
    assert seen_long_run


def test_program_table_with_the_references_zero_filler_rows(be):
    """generation/prog.rs leaves the rows beyond the executed words and beyond the listing zero: compress = 0 there."""
    rng = np.random.default_rng(53)
    n, listed, executed, beta = 64, 24, 41, 0xDEADBEEFCAFE
    addr = [11, 22, 33, 44]
    words = [int(x) for x in rng.integers(0, 1 << 40, listed)]
    run = [int(x) for x in rng.integers(0, listed, executed)]
    want = np.zeros((T.NUM_PROG_COLS, n), dtype=np.uint64)
    comp = lambda pc, w: (addr[0] + addr[1] * beta + addr[2] * beta ** 2 + addr[3] * beta ** 3 + pc * beta ** 4 + w * beta ** 5) % P
    for pc, w in enumerate(words):
        want[list(T.COL_PROG_CODE_ADDR_RANGE), pc] = addr
        want[T.COL_PROG_PC, pc], want[T.COL_PROG_INST, pc], want[T.COL_PROG_FILTER_PROG_CHUNK, pc], want[T.COL_PROG_COMP_PROG, pc] = pc, w, 1, comp(pc, w)
    for i, pc in enumerate(run):
        want[list(T.COL_PROG_EXEC_CODE_ADDR_RANGE), i] = addr
        want[T.COL_PROG_EXEC_PC, i], want[T.COL_PROG_EXEC_INST, i], want[T.COL_PROG_FILTER_EXEC, i] = pc, words[pc], 1
        want[T.COL_PROG_EXEC_COMP_PROG, i] = comp(pc, words[pc])
    want[T.COL_PROG_EXEC_COMP_PROG_PERM], want[T.COL_PROG_COMP_PROG_PERM] = TG.permuted_cols(want[T.COL_PROG_EXEC_COMP_PROG], want[T.COL_PROG_COMP_PROG])
    ex, pr = prog_sides(want)
    assert np.array_equal(be.generate_prog_trace(ex, pr, beta), want)


# ------------------------------------------------------------------------------------------------ whole proofs
def regenerate_on_device(b, traces, params, limb_bits, range_bits):
    """bitwise, range-check and program tables of an instance from their primary columns, resident in HBM"""
    bw, rc, pg = traces[2], traces[4], traces[10]
    n_ops = int(np.flatnonzero(bw[T.BW_TAG]).max()) + 1 if bw[T.BW_TAG].any() else 0
    live = np.flatnonzero(rc[:5].any(axis=0))
    n_rows = int(live.max()) + 1 if live.size else 0
    d_bw = dev_table(T.COL_NUM_BITWISE, bw.shape[1].bit_length() - 1)
    d_rc = dev_table(T.COL_NUM_RC, rc.shape[1].bit_length() - 1)
    d_pg = dev_table(T.NUM_PROG_COLS, pg.shape[1].bit_length() - 1)
    assert b.generate_bitwise_trace(np.ascontiguousarray(bw[:5, :n_ops]), params[0], limb_bits=limb_bits, out=d_bw) == bw.shape[1].bit_length() - 1
    assert b.generate_rc_trace(np.ascontiguousarray(rc[T.RC_VAL, :n_rows]), np.ascontiguousarray(rc[:4, :n_rows]), range_bits=range_bits,
                               out=d_rc) == rc.shape[1].bit_length() - 1
    ex, pr = prog_sides(pg)
    b.generate_prog_trace(ex, pr, params[1], out=d_pg)
    return d_bw, d_rc, d_pg


@pytest.fixture(scope="module")
def full_instances():
    from olavm_amd.air import miniexec as M
    return {"wide_program": M.instance(M.wide_program(), range_bits=16, limb_bits=8, prove_program_hash=True),
            "memory_program": M.instance(M.memory_program(), range_bits=16, limb_bits=8)}


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_device_generated_tables_prove_the_all_host_bytes(hasher, full_instances):
    from olavm_amd.backend import Backend
    full = T.ola_stark()
    blob = full.blob()
    committed = {"poseidon": "wide_program.proof", "blake3": "wide_program_blake3.proof"}[hasher]
    b = Backend(device=0, hasher=hasher)
    try:
        for name, (traces, params, compress) in full_instances.items():
            assert traces[4].shape[1] == 1 << 16 and traces[2].shape[1] == 1 << 18
            d_bw, d_rc, d_pg = regenerate_on_device(b, traces, params, 8, 16)
            for d, h in ((d_bw, traces[2]), (d_rc, traces[4]), (d_pg, traces[10])):
                assert np.array_equal(to_host(d), h), name
            mixed = list(traces)
            mixed[2], mixed[4], mixed[10] = d_bw, d_rc, d_pg
            assert b.check_constraints(full, mixed, params) == [], name
            proof = bytes(b.prove_with_traces(blob, mixed, params, compress))
            assert proof == bytes(b.prove_with_traces(blob, traces, params, compress)), name
            if name == "wide_program":
                assert proof == open(os.path.join(HERE, "golden", "ref_verified", committed), "rb").read()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ full height, resident
def test_program_table_at_2_to_22_rows_resident(be):
    import torch
    rng = np.random.default_rng(59)
    log_n, n, beta = 22, 1 << 22, 0x0123456789ABCDEF
    listed = 3 * n // 4
    pr = np.zeros((7, n), dtype=np.uint64)
    pr[:4, :listed] = rng.integers(0, 1 << 63, (4, 1), dtype=np.uint64)
    pr[4, :listed] = np.arange(listed, dtype=np.uint64)
    pr[5, :listed] = rng.integers(0, 1 << 63, listed, dtype=np.uint64) * np.uint64(2)
    pr[5, :listed:7] = np.uint64(P) + rng.integers(0, 1 << 31, len(range(0, listed, 7)), dtype=np.uint64)     # every seventh word is >= p
    pr[6, :listed] = 1
    pick = rng.integers(0, listed // 2, n)                       # half of the listing is never executed, hot words many times
    ex = np.ascontiguousarray(pr[:, pick])
    ex[6, n - 1000:] = 0
    d_ex, d_pr = to_dev(ex), to_dev(pr)
    out = dev_table(T.NUM_PROG_COLS, log_n)
    assert be.generate_prog_trace(d_ex, d_pr, beta, out=out) == log_n
    # the primary columns are copies (canonical)
    got_ex, got_pr = prog_sides(to_host(out))
    assert np.array_equal(got_ex, ex % np.uint64(P)) and np.array_equal(got_pr, pr % np.uint64(P))
    # the permuted pair is ola_permuted_cols_dev of the two compress columns
    pi, pt = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    be.permuted_cols_dev(out[T.COL_PROG_EXEC_COMP_PROG].data_ptr(), out[T.COL_PROG_COMP_PROG].data_ptr(), n, pi.data_ptr(), pt.data_ptr())
    assert torch.equal(out[T.COL_PROG_EXEC_COMP_PROG_PERM], pi) and torch.equal(out[T.COL_PROG_COMP_PROG_PERM], pt)
    # the compress columns against big integers
    host = to_host(out)
    for r in [int(x) for x in rng.integers(0, n, 4096)]:
        for side, col in ((ex, T.COL_PROG_EXEC_COMP_PROG), (pr, T.COL_PROG_COMP_PROG)):
            w = [int(x) for x in side[:6, r]]
            assert int(host[col, r]) == sum(w[k] * beta ** k for k in range(6)) % P, (r, col)
