"""ola_prove_with_traces on a REAL execution with a 2^20-row CPU table.

The traces come from the executor (native generator include/ola_tracegen.h, or olavm_amd/air/miniexec.py with --python)
running the memory program -- a store loop and a
load / add / store / load loop over `count` cells -- against the full-size fixed tables (range_bits 16, limb_bits 8):
count = 70000 gives 980 k executed CPU rows (2^20), 280 k memory cells, a 2^21-row program table (every fetched instruction and
immediate word) and 280 k range-checked sort values.  The proof is checked with the oracle's verifier; with OLA_TIMING=1 the
library prints its per-phase times (named after the reference's `timed!` scopes) to stderr.

    python tools/bench_prove_real.py [count] [reps] [--json out.json] [--phases] [--oracle] [--python] [--storage-slots N] [--hasher blake3] [--steps | --cells | --hashes | --records] [--shape readme]

--steps compares the two ways from an execution to proof bytes, taken in alternation `reps` times in this process: the table path
(the native generator fills all twelve tables, they are uploaded and proven) and the step path (the generator runs with
OLA_TRACEGEN_STEPS_ONLY, the step records go up, ola_generate_cpu_trace and ola_generate_prog_trace_steps write the CPU and the program
table into HBM and the proof runs on them as resident tables).  Timed apart: the native generator's call (ola_tracegen_run), the
Python binding's copies of its output into numpy arrays (harness cost, larger on the table path: it copies the two tables the step
path never builds), device table generation, and the proof.  --cells adds a third way to the alternation, the cell path: the generator runs with OLA_TRACEGEN_CELLS_ONLY, and on top of the step path's
two tables ola_generate_cmp_trace, ola_generate_memory_trace and ola_generate_rc_trace write the comparison, memory and range-check tables
into HBM -- the range-check table from a `vals` buffer in HBM that holds the CPU's values and, behind them, the lists the first two calls
leave there.  --hashes adds a fourth way, the hashes path: the generator runs with OLA_TRACEGEN_HASHES_ONLY -- it hashes no node of the
state tree and records no Poseidon row for it -- and on top of the cell path's five tables ola_generate_storage_trace hashes the tree on the
device, writes the storage-access table and fills the accesses' rows of the Poseidon table's inputs, ola_generate_poseidon_table makes
the Poseidon table from them, and the program table's challenge is drawn from the two roots the storage call returns; usable with
--storage-slots.  --records takes three ways in alternation: the table path, the hashes path and the records path -- the generator runs
with OLA_TRACEGEN_RECORDS_ONLY, builds no table, and one call, ola_prove_from_records, makes all twelve tables in HBM and proves them (so
its device_table_generation_s is part of prove_s); every path also reports link_bytes, the bytes that crossed the link: the tables'
(ola_gpu_upload_stats) plus the records handed to the device.  Identical proof bytes on every path are asserted in every round.  --shape readme runs the README's Fibonacci shape
(miniexec.fibonacci_loop(47, 3000): 864 002 CPU rows, every other table small) instead of the memory program.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    count = int(args[0]) if args else 70000
    reps = int(args[1]) if len(args) > 1 else 3
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    hasher = sys.argv[sys.argv.index("--hasher") + 1] if "--hasher" in sys.argv else "poseidon"
    from olavm_amd.air import fastexec, miniexec as M, ola_tables as T
    from olavm_amd.backend import Backend
    s = T.ola_stark()
    blob = s.blob()
    t0 = time.time()
    gen = M if "--python" in sys.argv else fastexec          # the native generator reproduces the Python executor word for word
    slots = int(sys.argv[sys.argv.index("--storage-slots") + 1]) if "--storage-slots" in sys.argv else 0
    shape = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else "memory"
    if shape not in ("readme", "memory"):
        raise SystemExit("--shape is readme or memory")
    if slots:       # BASELINE config 4: a Poseidon table of 1026 * slots live rows next to the CPU / memory tables
        prog, kw = M.storage_heavy_program(slots, count), {"prove_program_hash": True}
    elif shape == "readme":
        prog, kw = M.fibonacci_loop(47, 3000), {}
    else:
        prog, kw = M.memory_program(count), {}
    if "--steps" in sys.argv or "--cells" in sys.argv or "--hashes" in sys.argv or "--records" in sys.argv:
        return steps_against_tables(prog, kw, blob, reps, hasher, out, "--cells" in sys.argv or "--hashes" in sys.argv or "--records" in sys.argv,
                                    "storage_heavy_program(%d, %d)" % (slots, count) if slots else
                                    "fibonacci_loop(47, 3000)" if shape == "readme" else "memory_program(%d)" % count, "--hashes" in sys.argv or "--records" in sys.argv,
                                    "--records" in sys.argv)
    traces, params, compress = gen.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, **kw)
    gen_s = time.time() - t0
    heights = [int(t.shape[1]).bit_length() - 1 for t in traces]
    print("executed + filled 12 tables in %.1f s; log2 heights %s" % (gen_s, heights), flush=True)
    be = Backend(device=0, hasher=hasher)
    times = []
    for _ in range(reps):
        t0 = time.time()
        proof = be.prove_with_traces(blob, traces, params, compress)
        times.append(time.time() - t0)
        print("prove_with_traces: %.3f s, proof %d bytes" % (times[-1], len(proof)), flush=True)
    if "--phases" in sys.argv:          # one more proof on a context created with OLA_TIMING=1 (phase lines go to stderr)
        os.environ["OLA_TIMING"] = "1"
        be2 = Backend(device=0, hasher=hasher)
        be2.prove_with_traces(blob, traces, params, compress)          # cold context: tables, twiddles, allocations
        print("[ola-timing] ---- warm proof ----", file=sys.stderr, flush=True)
        be2.prove_with_traces(blob, traces, params, compress)
        be2.close()
    from tests import oracle_lib
    o = oracle_lib.load()
    import contextlib
    cfg = o.hasher(hasher)
    with cfg:
        rc, why = o.verify_all_proof(blob, proof, params)
    print("oracle verifier (%s configuration):" % hasher, rc, why, flush=True)
    oracle_s = None
    if "--oracle" in sys.argv:          # the CPU restatement on the same traces (all host cores it uses), byte comparison included
        t0 = time.time()
        with o.hasher(hasher):
            ref = o.prove_with_traces(blob, traces, params, compress)
        oracle_s = time.time() - t0
        print("oracle prove_with_traces (CPU port, %d threads): %.1f s, bytes identical: %s" % (o.lib.oracle_num_threads(), oracle_s, ref == proof), flush=True)
        if ref != proof:
            rc = 1
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump({"workload": ("storage_heavy_program(%d, %d)" % (slots, count) if slots else "memory_program(%d)" % count) + ", ola_stark(range_bits=16, limb_bits=8)", "log2_heights": heights, "hasher": hasher,
                       "trace_generation_s": round(gen_s, 1), "prove_s": [round(t, 4) for t in times], "proof_bytes": len(proof),
                       "oracle_verifier_rc": rc, "oracle_cpu_port_prove_s": None if oracle_s is None else round(oracle_s, 1)}, f, indent=1)
    if rc != 0:
        raise SystemExit(1)


def steps_against_tables(prog, kw, blob, reps, hasher, out, cells, workload, hashes=False, records=False):
    import numpy as np
    import torch
    from olavm_amd.air import fastexec, ola_tables as T
    from olavm_amd.backend import Backend
    be = Backend(device=0, hasher=hasher)
    runs = {"table_path": []}
    if not records:                    # --records: the table, hashes and records path alone
        runs["step_path"] = []
    if cells and not records:
        runs["cell_path"] = []
    if hashes:
        runs["hashes_path"] = []
    if records:
        runs["records_path"] = []
    proofs = {}
    nbytes = lambda rec, keys: int(sum(np.asarray(rec[k]).nbytes for k in keys))
    STEP_KEYS = ("steps", "listing")
    CELL_KEYS = STEP_KEYS + ("cells", "cmp_ops", "cpu_rc")
    HASH_KEYS = CELL_KEYS + ("accesses", "psdn_inputs", "psdn_filters")
    RECORD_KEYS = HASH_KEYS + ("bitwise_ops", "tape_cells", "psdn_calls", "words")

    def five_tables(rec, beta):
        """the CPU, program, comparison, memory and range-check tables in HBM from the records of a cells-only (or hashes-only) run"""
        d = {t: torch.empty((ncols, 1 << rec[key]), dtype=torch.int64, device="cuda")
             for t, ncols, key in ((T.CPU, T.NUM_CPU_COLS, "cpu_log_n"), (T.PROGRAM, T.NUM_PROG_COLS, "prog_log_n"), (T.MEMORY, T.NUM_MEM_COLS, "mem_log_n"),
                                   (T.CMP, T.COL_NUM_CMP, "cmp_log_n"), (T.RANGECHECK, T.COL_NUM_RC, "rc_log_n"))}
        n_cpu, n_cmp, n_cells = len(rec["cpu_rc"]), rec["cmp_ops"].shape[1], rec["cells"].shape[1]
        vals = torch.empty((n_cpu + n_cmp + 2 * n_cells + 1,), dtype=torch.int64, device="cuda")
        vals[:n_cpu] = torch.from_numpy(rec["cpu_rc"].view(np.int64)).cuda()
        d_steps = torch.from_numpy(rec["steps"].view(np.int64)).cuda()
        d_cells = torch.from_numpy(rec["cells"].view(np.int64)).cuda()
        torch.cuda.synchronize()
        be.generate_cpu_trace(d_steps, rec["cpu_log_n"], out=d[T.CPU])
        be.generate_prog_trace_steps(d_steps, rec["listing"], beta, out=d[T.PROGRAM])
        be.generate_cmp_trace(rec["cmp_ops"], out=d[T.CMP], abs_diff_out=vals.data_ptr() + 8 * n_cpu)
        _, _, (n_sort, n_region) = be.generate_memory_trace(d_cells, out=d[T.MEMORY], rc_out=vals.data_ptr() + 8 * (n_cpu + n_cmp))
        n_rows = n_cpu + n_cmp + n_sort + n_region
        filters = torch.zeros((4, n_rows), dtype=torch.int64, device="cuda")
        for col, lo, hi in ((0, 0, n_cpu), (3, n_cpu, n_cpu + n_cmp), (1, n_cpu + n_cmp, n_cpu + n_cmp + n_sort), (2, n_cpu + n_cmp + n_sort, n_rows)):
            filters[col, lo:hi] = 1
        torch.cuda.synchronize()
        be.generate_rc_trace(vals.data_ptr(), filters, range_bits=16, out=d[T.RANGECHECK], n_rows=n_rows)
        return d
    for rep in range(reps + 1):                                  # rep 0 warms both paths up and is not kept
        tm = {}
        t0 = time.perf_counter()
        traces, params, compress = fastexec.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, timings=tm, **kw)
        t1 = time.perf_counter()
        proofs["table_path"] = bytes(be.prove_with_traces(blob, traces, params, compress))
        t2 = time.perf_counter()
        a = {"native_trace_generation_s": tm["native_s"], "binding_copies_s": tm["copy_s"], "device_table_generation_s": 0.0, "prove_s": t2 - t1,
             "total_s": t2 - t0, "total_without_binding_copies_s": t2 - t0 - tm["copy_s"], "link_bytes": be.upload_stats()["link_bytes"]}
        del traces
        if not records:
            t0 = time.perf_counter()
            lean, params, compress, rec = fastexec.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, steps_only=True, timings=tm, **kw)
            t1 = time.perf_counter()
            d_cpu = torch.empty((T.NUM_CPU_COLS, 1 << rec["cpu_log_n"]), dtype=torch.int64, device="cuda")
            d_pg = torch.empty((T.NUM_PROG_COLS, 1 << rec["prog_log_n"]), dtype=torch.int64, device="cuda")
            d_steps = torch.from_numpy(rec["steps"].view(np.int64)).cuda()
            torch.cuda.synchronize()                                 # complete before the library's stream reads and writes them
            be.generate_cpu_trace(d_steps, rec["cpu_log_n"], out=d_cpu)
            be.generate_prog_trace_steps(d_steps, rec["listing"], params[1], out=d_pg)
            t2 = time.perf_counter()
            lean[T.CPU], lean[T.PROGRAM] = d_cpu, d_pg
            proofs["step_path"] = bytes(be.prove_with_traces(blob, lean, params, compress))
            t3 = time.perf_counter()
            b = {"native_trace_generation_s": tm["native_s"], "binding_copies_s": tm["copy_s"], "device_table_generation_s": t2 - t1, "prove_s": t3 - t2,
                 "total_s": t3 - t0, "total_without_binding_copies_s": t3 - t0 - tm["copy_s"],
                 "link_bytes": be.upload_stats()["link_bytes"] + nbytes(rec, STEP_KEYS)}
            del lean, d_cpu, d_pg, d_steps
            assert proofs["step_path"] == proofs["table_path"], "the two paths give different proof bytes"
        if cells and not records:
            t0 = time.perf_counter()
            lean, params, compress, rec = fastexec.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, cells_only=True, timings=tm, **kw)
            t1 = time.perf_counter()
            d = five_tables(rec, params[1])
            t2 = time.perf_counter()
            for t, table in d.items():
                lean[t] = table
            proofs["cell_path"] = bytes(be.prove_with_traces(blob, lean, params, compress))
            t3 = time.perf_counter()
            c = {"native_trace_generation_s": tm["native_s"], "binding_copies_s": tm["copy_s"], "device_table_generation_s": t2 - t1, "prove_s": t3 - t2,
                 "total_s": t3 - t0, "total_without_binding_copies_s": t3 - t0 - tm["copy_s"],
                 "link_bytes": be.upload_stats()["link_bytes"] + nbytes(rec, CELL_KEYS)}
            del lean, d
            assert proofs["cell_path"] == proofs["table_path"], "the cell path gives different proof bytes"
        if hashes:
            t0 = time.perf_counter()
            lean, params, compress, rec = fastexec.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, hashes_only=True, timings=tm, **kw)
            t1 = time.perf_counter()
            d_st = torch.empty((T.NUM_COL_ST, 1 << rec["storage_log_n"]), dtype=torch.int64, device="cuda")
            d_ps = torch.empty((T.NUM_POSEIDON_COLS, 1 << rec["poseidon_log_n"]), dtype=torch.int64, device="cuda")
            d_in, d_f = torch.from_numpy(rec["psdn_inputs"].view(np.int64)).cuda(), torch.from_numpy(rec["psdn_filters"].view(np.int64)).cuda()
            torch.cuda.synchronize()
            _, roots = be.generate_storage_trace(rec["accesses"], out=d_st, psdn_inputs=d_in, psdn_filters=d_f)
            be.generate_poseidon_table(d_in, d_f, out=d_ps)
            params[1] = compress[T.PROGRAM] = fastexec.program_beta(roots)        # the challenge the table path drew from its own tree's roots
            d = five_tables(rec, params[1])
            t2 = time.perf_counter()
            for t, table in d.items():
                lean[t] = table
            lean[T.STORAGE_ACCESS], lean[T.POSEIDON] = d_st, d_ps
            proofs["hashes_path"] = bytes(be.prove_with_traces(blob, lean, params, compress))
            t3 = time.perf_counter()
            h = {"native_trace_generation_s": tm["native_s"], "binding_copies_s": tm["copy_s"], "device_table_generation_s": t2 - t1, "prove_s": t3 - t2,
                 "total_s": t3 - t0, "total_without_binding_copies_s": t3 - t0 - tm["copy_s"],
                 "link_bytes": be.upload_stats()["link_bytes"] + nbytes(rec, HASH_KEYS)}
            del lean, d, d_st, d_ps, d_in, d_f
            assert proofs["hashes_path"] == proofs["table_path"], "the hashes path gives different proof bytes"
        if records:
            t0 = time.perf_counter()
            _, _, _, rec = fastexec.instance(prog, range_bits=16, limb_bits=8, max_steps=1 << 24, records_only=True, timings=tm, **kw)
            t1 = time.perf_counter()
            proofs["records_path"] = bytes(be.prove_from_records(blob, rec, range_bits=16, limb_bits=8, result_line=bool(kw.get("prove_program_hash"))))
            t3 = time.perf_counter()
            r = {"native_trace_generation_s": tm["native_s"], "binding_copies_s": tm["copy_s"], "device_table_generation_s": 0.0, "prove_s": t3 - t1,
                 "total_s": t3 - t0, "total_without_binding_copies_s": t3 - t0 - tm["copy_s"],
                 "link_bytes": be.upload_stats()["link_bytes"] + nbytes(rec, RECORD_KEYS)}
            del rec
            assert proofs["records_path"] == proofs["table_path"], "the records path gives different proof bytes"
        if rep:
            runs["table_path"].append(a)
            if not records:
                runs["step_path"].append(b)
            if cells and not records:
                runs["cell_path"].append(c)
            if hashes:
                runs["hashes_path"].append(h)
            if records:
                runs["records_path"].append(r)
        print(("warm-up " if not rep else "") + "table path %s" % {k: round(v, 3) for k, v in a.items()}, flush=True)
        if not records:
            print(("warm-up " if not rep else "") + "step path  %s" % {k: round(v, 3) for k, v in b.items()}, flush=True)
        if records:
            print(("warm-up " if not rep else "") + "records path %s" % {k: round(v, 3) for k, v in r.items()}, flush=True)
        if cells and not records:
            print(("warm-up " if not rep else "") + "cell path  %s" % {k: round(v, 3) for k, v in c.items()}, flush=True)
        if hashes:
            print(("warm-up " if not rep else "") + "hashes path %s" % {k: round(v, 3) for k, v in h.items()}, flush=True)
    be.close()
    med = lambda path, key: sorted(r[key] for r in runs[path])[len(runs[path]) // 2]
    summary = {path: {key: round(med(path, key), 3) for key in runs[path][0]} for path in runs}
    spans = {path: [round(min(r["total_s"] for r in runs[path]), 3), round(max(r["total_s"] for r in runs[path]), 3)] for path in runs}
    print(json.dumps(summary), flush=True)
    print(json.dumps({"total_s_span": spans}), flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        json.dump({"workload": workload + ", ola_stark(range_bits=16, limb_bits=8)", "hasher": hasher, "reps": reps,
                   "proof_bytes_identical": True, "median": summary, "total_s_span": spans, "runs": runs}, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
