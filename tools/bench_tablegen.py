"""Times ola_generate_rc_trace / ola_generate_bitwise_trace / ola_generate_prog_trace -- and ola_generate_cpu_trace /
ola_generate_prog_trace_steps, the cases cpu:20 cpu:22 progsteps:21 progsteps:23, and ola_generate_memory_trace / ola_generate_cmp_trace,
the cases mem:19 mem:21 cmp:16, and ola_generate_storage_trace / ola_generate_poseidon_table, the cases storage:141 storage:8170
storagesib:141 storagesib:8170 (the number is the number of accesses; `sib` = with the caller's siblings) poseidon:22, and
ola_generate_tape_trace / ola_generate_poseidon_chunk_trace / ola_generate_prog_chunk_trace, the cases tape:N pchunk:N progchunk:N (the
number is the number of tape cells, of POSEIDON calls, of 8-word listing chunks) -- with resident inputs and outputs, next to
the same derived columns obtained without them: one ola_permuted_cols_dev call per pair (device) plus numpy for the other columns
(host), and next to the oracle's sequential permuted_cols on one host core (as tools/bench_lookup.py measures it).

    python tools/bench_tablegen.py [--runs 7] [--json out.json] [--skip-launches] [case ...]     # cases: bitwise:18 rc:16 rc:21 prog:20 prog:23

Device times: two events on the context's stream around the whole call (the call synchronises inside), median of --runs after a
warm-up.  Wall times: time.perf_counter around the same calls.  Launch counts: the kernel-trace rows of a child process that makes
two calls minus those of one that makes one (rocprofv3 --kernel-trace; `--child` is that process)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from olavm_amd.air import cpu_steps as S, ola_tables as T
from olavm_amd.air.dsl import P

CASES = ["bitwise:18", "rc:16", "rc:21", "prog:20", "prog:23"]
STEP_CASES = ["cpu:20", "cpu:22", "progsteps:21", "progsteps:23"]       # named on the command line
CELL_CASES = ["mem:19", "mem:21", "cmp:16"]                              # named on the command line
HASH_CASES = ["storage:141", "storage:8170", "storagesib:141", "storagesib:8170", "poseidon:22"]     # named on the command line
SMALL_CASES = ["tape:100000", "pchunk:30000", "progchunk:100000"]          # named on the command line
FN = (lambda x, y: x & y, lambda x, y: x | y, lambda x, y: x ^ y)


def inputs(kind, log_n, rng):
    """-> (primary inputs as numpy arrays, keyword arguments) of a table that fills 2^log_n rows"""
    if kind in ("storage", "storagesib"):
        # log_n is the number of accesses here: a third of them writes of fresh random keys, then a read and an overwrite of each in turn
        # (storage_heavy_program's pattern); 512 Poseidon rows each, back to back.  With siblings the accesses are independent and any
        # words do: the work does not depend on them
        k = log_n
        keys = rng.integers(0, P, (4, (k + 2) // 3), dtype=np.uint64)
        recs = np.zeros((14, k), dtype=np.uint64)
        which = np.concatenate([np.arange(keys.shape[1]), np.repeat(np.arange(keys.shape[1]), 2)])[:k]
        recs[0:4] = keys[:, which]
        recs[4:12] = rng.integers(0, P, (8, k), dtype=np.uint64)
        recs[12] = 1
        recs[12, keys.shape[1] + 1::2] = 0
        recs[13] = 512 * np.arange(k)
        sib = (rng.integers(0, P, (1024, k), dtype=np.uint64),) if kind == "storagesib" else ()
        return (recs,) + sib, {"stride": 512 * k}
    if kind in SMALL_KINDS:
        # log_n is a count here as well.  tape: a quarter as many addresses as cells, written once and read three times on average;
        # pchunk: call i hashes 1 + i % 4 blocks, the blocks back to back in the Poseidon table; progchunk: one table row per chunk.
        # The Poseidon table is random words: the gathers do not depend on them
        k = log_n
        if kind == "tape":
            return (np.stack([rng.integers(0, max(k // 4, 1), k, dtype=np.uint64), np.full(k, T.op_mask("TLOAD"), dtype=np.uint64),
                              rng.integers(0, P, k, dtype=np.uint64)]),), {}
        blocks = 1 + np.arange(k, dtype=np.uint64) % np.uint64(4) if kind == "pchunk" else np.ones(k, dtype=np.uint64)
        psdn = rng.integers(0, P, (T.NUM_POSEIDON_COLS, 1 << max(3, (int(blocks.sum()) - 1).bit_length())), dtype=np.uint64)
        if kind == "progchunk":
            return (rng.integers(0, P, 8 * k, dtype=np.uint64), rng.integers(0, P, 4, dtype=np.uint64), psdn), {}
        first = np.concatenate([[0], np.cumsum(blocks)[:-1]]).astype(np.uint64)
        return (np.stack([10 + np.arange(k, dtype=np.uint64), rng.integers(0, 1 << 32, k, dtype=np.uint64), 8 * blocks,
                          rng.integers(0, 1 << 32, k, dtype=np.uint64), first]), psdn), {}
    n = 1 << log_n
    if kind == "poseidon":
        return (rng.integers(0, P, (12, n), dtype=np.uint64), rng.integers(0, 2, (4, n), dtype=np.uint64)), {}
    if kind == "rc":
        rows = n if log_n > 16 else n // 2
        vals = rng.integers(0, 1 << 32, rows, dtype=np.uint64)
        vals[: rows // 4] = rng.integers(0, 50, rows // 4)             # small values dominate, as with real range checks
        return (vals, rng.integers(0, 2, (4, rows), dtype=np.uint64)), {"range_bits": 16}
    if kind == "bitwise":
        rows = n // 2
        which = rng.integers(0, 3, rows)
        x, y = rng.integers(0, 1 << 32, rows, dtype=np.uint64), rng.integers(0, 1 << 32, rows, dtype=np.uint64)
        res = np.choose(which, [x & y, x | y, x ^ y])
        tag = np.array([T.op_mask("AND"), T.op_mask("OR"), T.op_mask("XOR")], dtype=np.uint64)[which]
        return (np.stack([np.ones(rows, dtype=np.uint64), tag, x, y, res]),), {"limb_bits": 8, "beta": 0x123456789ABCDEF}
    if kind == "mem":          # the synthetic pattern of docs/EXPERIMENTS.md's host figures, in execution order: every address stored once,
        k = 290000 * n >> 21   # then loaded three times in reverse order; as many cells as memory_program(290000) has at 2^21 rows (1.16 M).
        # Not memory_program's own cells (store, then load / store / load per address): the clocks differ; the values are random field
        # elements, as wide as its Fibonacci numbers mod p, so that the value pass of the sort covers 64 bits as it does there
        addr = np.arange(1, k + 1, dtype=np.uint64)
        value = rng.integers(0, P, k, dtype=np.uint64)
        cells = np.zeros((5, 4 * k), dtype=np.uint64)
        cells[0], cells[1, :k], cells[2, :k], cells[4, :k] = np.concatenate([addr] + 3 * [addr[::-1]]), 10 + 2 * np.arange(k), T.op_mask("MSTORE"), 1
        cells[1, k:], cells[2, k:] = 10 + 2 * k + 3 * np.arange(3 * k), T.op_mask("MLOAD")
        cells[3] = np.concatenate([value] + 3 * [value[::-1]])
        return (cells,), {}
    if kind == "cmp":          # 15/16 of the rows live, 32-bit operands
        return (rng.integers(0, 1 << 32, (2, n - n // 16), dtype=np.uint64),), {}
    if kind == "cpu":          # 15/16 of the rows live, every word of the record random
        return (rng.integers(0, P, (S.STEP_WORDS, n - n // 16), dtype=np.uint64),), {"log_n": log_n}
    listed = 3 * n // 4
    pr = np.zeros((7, n), dtype=np.uint64)
    pr[:4, :listed] = rng.integers(0, P, (4, 1), dtype=np.uint64)
    pr[4, :listed] = np.arange(listed, dtype=np.uint64)
    pr[5, :listed] = rng.integers(0, P, listed, dtype=np.uint64)
    pr[6, :listed] = 1
    if kind == "progsteps":    # 5/8 n steps, every fifth an extension line, half of the others with an immediate word: about 0.75 n executed rows
        k = 5 * n // 8
        steps = np.zeros((S.STEP_WORDS, k), dtype=np.uint64)
        w = lambda col: col - S.STEP_FIRST_COL
        pick = rng.integers(0, listed // 2, k)
        steps[w(T.COL_ADDR_CODE_RANGE.start):w(T.COL_ADDR_CODE_RANGE.stop)] = pr[:4, :1]
        steps[w(T.COL_PC)], steps[w(T.COL_INST)] = pr[4, pick], pr[5, pick]
        steps[w(T.COL_IMM_VAL)] = pr[5, (pick + 1) % listed]
        steps[w(T.COL_OPCODE)] = T.op_mask("ADD")
        steps[w(T.COL_OP1_IMM)] = rng.integers(0, 2, k)
        steps[w(T.COL_IS_EXT_LINE), ::5] = 1
        return (steps, pr), {"beta": 0x123456789ABCDEF}
    ex = np.ascontiguousarray(pr[:, rng.integers(0, listed // 2, n)])
    return (ex, pr), {"beta": 0x123456789ABCDEF}


def to_dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()           # complete before the library's stream reads it
    return t


def call(be, kind, dev, kw, out):
    if kind == "rc":
        return be.generate_rc_trace(dev[0], dev[1], range_bits=kw["range_bits"], out=out)
    if kind == "bitwise":
        return be.generate_bitwise_trace(dev[0], kw["beta"], limb_bits=kw["limb_bits"], out=out)
    if kind == "cpu":
        return be.generate_cpu_trace(dev[0], kw["log_n"], out=out)
    if kind in ("mem", "cmp"):             # the value list stays in HBM as well
        import torch
        if "list" not in kw:
            kw["list"] = torch.empty((2 * dev[0].shape[1] + 1,), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
        if kind == "mem":
            return be.generate_memory_trace(dev[0], out=out, rc_out=kw["list"])[0]
        return be.generate_cmp_trace(dev[0], out=out, abs_diff_out=kw["list"])[0]
    if kind in ("storage", "storagesib"):  # the Poseidon inputs stay in HBM as well
        import torch
        if "psdn" not in kw:
            kw["psdn"] = torch.zeros((12, kw["stride"]), dtype=torch.int64, device="cuda"), torch.zeros((4, kw["stride"]), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
        return be.generate_storage_trace(dev[0], siblings=dev[1] if kind == "storagesib" else None, out=out, psdn_inputs=kw["psdn"][0],
                                         psdn_filters=kw["psdn"][1], roots_out=False)[0]
    if kind == "poseidon":
        return be.generate_poseidon_table(dev[0], dev[1], out=out)
    if kind == "tape":
        return be.generate_tape_trace(dev[0], out=out)
    if kind == "pchunk":
        return be.generate_poseidon_chunk_trace(dev[0], dev[1], out=out)
    if kind == "progchunk":
        return be.generate_prog_chunk_trace(dev[0], dev[1], dev[2], result_line=True, out=out)
    if kind == "progsteps":
        return be.generate_prog_trace_steps(dev[0], dev[1], kw["beta"], out=out)[0]
    return be.generate_prog_trace(dev[0], dev[1], kw["beta"], out=out)


NCOLS = {"rc": T.COL_NUM_RC, "bitwise": T.COL_NUM_BITWISE, "prog": T.NUM_PROG_COLS, "cpu": T.NUM_CPU_COLS, "progsteps": T.NUM_PROG_COLS,
         "mem": T.NUM_MEM_COLS, "cmp": T.COL_NUM_CMP, "storage": T.NUM_COL_ST, "storagesib": T.NUM_COL_ST, "poseidon": T.NUM_POSEIDON_COLS,
         "tape": T.NUM_COL_TAPE, "pchunk": T.NUM_POSEIDON_CHUNK_COLS, "progchunk": T.NUM_PROG_CHUNK_COLS}
SMALL_KINDS = ("tape", "pchunk", "progchunk")


def table_log_n(kind, arg):
    """log2 of the table's height: the case's number, but for the storage cases, whose number counts accesses, and the tape and chunk
    cases, whose number counts cells, calls (call i: a header row and 1 + i % 4 extension rows) and chunks"""
    if kind in SMALL_KINDS:
        rows = arg if kind != "pchunk" else sum(2 + i % 4 for i in range(arg))
        return max(3, (rows - 1).bit_length())
    return max(3, (256 * arg - 1).bit_length()) if kind in ("storage", "storagesib") else arg


def pairs_of(kind):
    """(input column, table column, permuted input column, permuted table column) of every lookup pair of the table"""
    if kind == "rc":
        return [(T.RC_LIMB_LO, T.RC_FIX_RANGE_CHECK_U16, T.RC_LIMB_LO_PERMUTED, T.RC_FIX_RANGE_CHECK_U16_PERMUTED_LO),
                (T.RC_LIMB_HI, T.RC_FIX_RANGE_CHECK_U16, T.RC_LIMB_HI_PERMUTED, T.RC_FIX_RANGE_CHECK_U16_PERMUTED_HI)]
    if kind in ("cpu", "mem", "cmp", "storage", "storagesib", "poseidon") + SMALL_KINDS:
        return []
    if kind in ("prog", "progsteps"):
        return [(T.COL_PROG_EXEC_COMP_PROG, T.COL_PROG_COMP_PROG, T.COL_PROG_EXEC_COMP_PROG_PERM, T.COL_PROG_COMP_PROG_PERM)]
    out = []
    for g, (src, perm) in enumerate(((T.BW_OP0_LIMBS, T.BW_OP0_LIMBS_PERMUTED), (T.BW_OP1_LIMBS, T.BW_OP1_LIMBS_PERMUTED), (T.BW_RES_LIMBS, T.BW_RES_LIMBS_PERMUTED))):
        out += [(src.start + i, T.BW_FIX_RANGE_CHECK_U8, perm.start + i, T.BW_FIX_RANGE_CHECK_U8_PERMUTED.start + 4 * g + i) for i in range(4)]
    return out + [(T.BW_COMPRESS_LIMBS.start + i, T.BW_FIX_COMPRESS, T.BW_COMPRESS_PERMUTED.start + i, T.BW_FIX_COMPRESS_PERMUTED.start + i) for i in range(4)]


def host_columns(kind, host, kw, n):
    """the non-permuted derived columns with numpy, the way a host without the entry points fills them (wall seconds)"""
    t0 = time.perf_counter()
    if kind == "rc":
        vals = host[0]
        lo, hi = vals & np.uint64(0xFFFF), vals >> np.uint64(16)
        fix = np.minimum(np.arange(n, dtype=np.uint64), np.uint64(0xFFFF))
        keep = (lo, hi, fix)
    else:
        b = kw["beta"] % P
        pw = [pow(b, k, P) for k in range(6)]
        if kind == "prog":
            keep = []
            for side in host:
                acc = np.zeros(n, dtype=object)
                for k in range(6):
                    acc = acc + side[k].astype(object) * pw[k]
                keep.append((acc % P).astype(np.uint64))
        else:
            ops = host[0]
            keep = []
            for i in range(4):
                limbs = [(ops[k] >> np.uint64(8 * i)) & np.uint64(255) for k in (2, 3, 4)]
                acc = ops[1].astype(object) + limbs[0].astype(object) * pw[1] + limbs[1].astype(object) * pw[2] + limbs[2].astype(object) * pw[3]
                keep += limbs + [(acc % P).astype(np.uint64)]
            idx = np.arange(1 << 16, dtype=np.uint64)
            x, y = idx >> np.uint64(8), idx & np.uint64(255)
            for f, name in zip(FN, ("AND", "OR", "XOR")):
                acc = T.op_mask(name) + x.astype(object) * pw[1] + y.astype(object) * pw[2] + f(x, y).astype(object) * pw[3]
                keep.append((acc % P).astype(np.uint64))
    return time.perf_counter() - t0, keep


def measure(kind, log_n, runs):
    import torch
    import ctypes as C
    from olavm_amd.backend import Backend
    from tests import oracle_lib
    rng = np.random.default_rng(log_n)
    host, kw = inputs(kind, log_n, rng)
    arg, log_n = log_n, table_log_n(kind, log_n)
    n = 1 << log_n
    be = Backend(device=0)
    sp = C.c_void_p()
    be._chk(be.lib.ola_gpu_get_stream(be.ctx, C.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    dev = [to_dev(a) for a in host]
    out = torch.empty((NCOLS[kind], n), dtype=torch.int64, device="cuda")
    assert call(be, kind, dev, kw, out) == log_n           # warm-up (pool blocks, code objects)

    def timed(f):
        dev_ms, wall_ms = [], []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record(stream)
            f()
            b.record(stream)
            b.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(a.elapsed_time(b))
        return statistics.median(dev_ms), statistics.median(wall_ms)

    rec = {"table": kind, "log_n": log_n, "runs": runs}
    rec["call_device_ms"], rec["call_wall_ms"] = timed(lambda: call(be, kind, dev, kw, out))
    if kind in ("storage", "storagesib", "poseidon"):      # the host-side counterpart is StorageTree::access / poseidon_row of the native generator
        if kind == "poseidon":
            rec["effective_GBps"] = 8 * (16 + T.NUM_POSEIDON_COLS) * n / (rec["call_device_ms"] * 1e6)
        else:
            rec["accesses"], rec["permutations"] = arg, 512 * arg
        rec["table_words"] = NCOLS[kind] * n
        be.close()
        return rec
    if kind in SMALL_KINDS:                # no permuted pairs; the host-side counterpart is tape_table() / poseidon_chunk_table() / prog_chunk_and_poseidon()
        rec["records"] = arg
        rec["table_words"] = NCOLS[kind] * n
        be.close()
        return rec
    if kind in ("mem", "cmp"):             # no permuted pairs; the host-side counterpart is memory_table() / cmp_table() of the native generator (docs/EXPERIMENTS.md, the last section)
        rec["cells" if kind == "mem" else "operand_pairs"] = int(host[0].shape[1])
        rec["table_words"] = NCOLS[kind] * n
        be.close()
        return rec
    if kind in ("cpu", "progsteps"):       # no host-side counterpart to compare with: the table path never had these inputs
        rec["steps"] = int(host[0].shape[1])
        if kind == "cpu":                  # bytes read and written: the records and the table
            rec["effective_GBps"] = 8 * (S.STEP_WORDS * rec["steps"] + T.NUM_CPU_COLS * n) / (rec["call_device_ms"] * 1e6)
        rec["table_words"] = NCOLS[kind] * n
        be.close()
        return rec
    # the same permuted columns pair by pair, from the columns the call just wrote
    pairs = pairs_of(kind)
    tmp = torch.empty((2, n), dtype=torch.int64, device="cuda")

    def pair_by_pair():
        for ci, ct, _, _ in pairs:
            be.permuted_cols_dev(out[ci].data_ptr(), out[ct].data_ptr(), n, tmp[0].data_ptr(), tmp[1].data_ptr())
    pair_by_pair()
    rec["pairs"] = len(pairs)
    rec["pair_by_pair_device_ms"], rec["pair_by_pair_wall_ms"] = timed(pair_by_pair)
    same = True
    for ci, ct, pi, pt in pairs:
        be.permuted_cols_dev(out[ci].data_ptr(), out[ct].data_ptr(), n, tmp[0].data_ptr(), tmp[1].data_ptr())
        same &= bool(torch.equal(tmp[0], out[pi]) and torch.equal(tmp[1], out[pt]))
    rec["pair_by_pair_identical"] = same
    if kind != "prog" or log_n <= 20:
        rec["numpy_other_columns_wall_ms"] = host_columns(kind, host, kw, n)[0] * 1e3
    # the sequential loop on one host core, one pair
    o = oracle_lib.load()
    ci, ct = pairs[0][0], pairs[0][1]
    a, b = out[ci].cpu().numpy().view(np.uint64), out[ct].cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    o.permuted_cols(a, b)
    rec["oracle_one_pair_wall_ms"] = (time.perf_counter() - t0) * 1e3
    rec["oracle_all_pairs_wall_ms_projected"] = rec["oracle_one_pair_wall_ms"] * len(pairs)
    rec["table_words"] = NCOLS[kind] * n
    be.close()
    return rec


def child(kind, log_n, calls, pair_by_pair):
    import torch
    from olavm_amd.backend import Backend
    host, kw = inputs(kind, log_n, np.random.default_rng(log_n))
    n = 1 << table_log_n(kind, log_n)
    be = Backend(device=0)
    dev = [to_dev(a) for a in host]
    out = torch.empty((NCOLS[kind], n), dtype=torch.int64, device="cuda")
    tmp = torch.empty((2, n), dtype=torch.int64, device="cuda")
    call(be, kind, dev, kw, out)
    for _ in range(calls):
        if pair_by_pair:
            for ci, ct, _, _ in pairs_of(kind):
                be.permuted_cols_dev(out[ci].data_ptr(), out[ct].data_ptr(), n, tmp[0].data_ptr(), tmp[1].data_ptr())
        else:
            call(be, kind, dev, kw, out)
    be.close()


def traced_kernels(kind, log_n, calls, pair_by_pair):
    """kernel launches (by name) of a child that makes `calls` calls after its warm-up"""
    d = tempfile.mkdtemp(prefix="tablegen_trace_")
    # the child under a time limit of its own that also ends the traced process; 20 children at most (5 cases x 2 ways x 2 runs),
    # a few seconds each
    cmd = ["timeout", "-k", "10", "60", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__), "--child",
           kind, str(log_n), str(calls), "1" if pair_by_pair else "0"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tempfile.gettempdir())
    names = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row.get("Kernel_Name", "?")
            names[k] = names.get(k, 0) + 1
    return names


def launches(kind, log_n):
    rec = {}
    for label, pbp in (("call", False), ("pair_by_pair", True)):
        if pbp and kind in ("storage", "storagesib", "poseidon") + SMALL_KINDS:      # no lookup pairs: nothing to compare with
            continue
        one, two = traced_kernels(kind, log_n, 1, pbp), traced_kernels(kind, log_n, 2, pbp)
        per = {k: two.get(k, 0) - one.get(k, 0) for k in two}
        rec[label + "_launches"] = sum(per.values())
        sorts = {k: v for k, v in per.items() if "radix" in k.lower() or "onesweep" in k.lower() or "sort" in k.lower()}
        rec[label + "_sort_kernel_launches"] = sum(sorts.values())
        rec[label + "_kernels"] = {k: v for k, v in sorted(per.items()) if v}      # the whole name: rocPRIM's kernels differ only far into it
    return rec


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] == "1")
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    recs = []
    for case in a.cases or CASES:
        kind, log_n = case.split(":")
        rec = measure(kind, int(log_n), a.runs)
        if not a.skip_launches:
            rec.update(launches(kind, int(log_n)))
        recs.append(rec)
        print(json.dumps({k: v for k, v in rec.items() if not k.endswith("_kernels")}), flush=True)
        if a.json:
            json.dump(recs, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
