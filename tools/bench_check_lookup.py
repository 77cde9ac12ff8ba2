#!/usr/bin/env python3
"""Times ola_check_lookup on an executed program whose CPU table has 2^log_n rows (memory_program, the benchmark's real trace):

  * the CPU -> memory lookup (16 looking entries of the CPU table, 6 words) and the CPU -> program lookup (2 entries, 6 words), on the
    valid trace and with one looked row dropped;
  * per case: the whole call from device-resident tables (wall clock, so that the link is not what is measured), the device time
    between the first count kernel and the last read-back (printed by the library under OLA_TIMING=1), nanoseconds per selected
    row, and the launch count (kernels of check.hip + rocPRIM sort / scan calls);
  * the yardstick: ola_check_constraints' whole-call time in the same process on the same CPU table (tables=[cpu], host columns
    and device-resident).

    python tools/bench_check_lookup.py [--log-n 22] [--reps 5] [--json out.json]         -> one JSON line

One warm-up call per case (it allocates), then --reps timed calls: median, minimum and maximum are reported."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(xs, digits=3):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], digits), "min": round(xs[0], digits), "max": round(xs[-1], digits)}


def drop_first_looked_row(looked, table):
    """a copy of `table` whose first filter-selected row is not selected any more (the filter: a sum of selector columns) -> (copy, row)"""
    import numpy as np
    f = looked.filter_column
    assert f.constant == 0 and all(k == 1 for _, k in f.terms)
    out = table.copy()
    row = int(np.nonzero(sum(out[c] for c, _ in f.terms) == 1)[0][0])
    col = next(c for c, _ in f.terms if out[c, row] == 1)
    out[col, row] = 0
    return out, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    os.environ["OLA_TIMING"] = "1"                     # read when the context is created
    import numpy as np
    import torch
    from bench_check_constraints import Stderr
    from olavm_amd.air import fastexec, miniexec as M, ola_tables as T
    from olavm_amd.backend import Backend
    airset = T.ola_stark()
    blob = airset.blob()
    count = ((1 << a.log_n) - 8) // 14
    traces, params, _ = fastexec.instance(M.memory_program(count), range_bits=16, limb_bits=8, max_steps=1 << (a.log_n + 1))
    assert traces[T.CPU].shape[1] == 1 << a.log_n
    with Stderr():
        be = Backend(device=0)
    res = {"instance": "memory_program(%d): heights 2^%s" % (count, [int(t.shape[1]).bit_length() - 1 for t in traces]), "reps": a.reps, "lookups": {}}
    pat = re.compile(r"check_lookup: lookup (\d+), width (\d+), (\d+) looking entries, (\d+) selected rows: (\d+) kernel launches \+ (\d+) sort / scan calls, ([0-9.]+) ms")
    dev = {}

    def resident(t, arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0").contiguous()

    for name, li in (("cpu_memory", 0), ("cpu_program", 16)):
        ctl = airset.ctls[li]
        named = sorted({t.table for t in ctl.looking_tables} | {ctl.looked_table.table})
        for t in named:
            if t not in dev:
                dev[t] = resident(t, traces[t])
        dropped, row = drop_first_looked_row(ctl.looked_table, traces[ctl.looked_table.table])
        looked = ctl.looked_table
        dev_dropped = resident(looked.table, dropped)
        torch.cuda.synchronize()
        for case, looked_dev in (("valid", dev[looked.table]), ("one looked row dropped", dev_dropped)):
            tabs = [None] * len(traces)
            for t in named:
                tabs[t] = dev[t]
            tabs[looked.table] = looked_dev
            whole, device, info = [], [], None
            for _ in range(a.reps + 1):
                with Stderr() as err:
                    t0 = time.perf_counter()
                    got, n, totals, width = be.check_lookup_raw(blob, tabs, li, cap=16)
                    whole.append((time.perf_counter() - t0) * 1e3)
                m = pat.search(err.text)
                device.append(float(m.group(7)))
                info = m
            assert n == (0 if case == "valid" else 1) and totals[3] == n, (name, case, totals)
            rows = totals[0] + totals[1]
            res["lookups"].setdefault(name, {"lookup": li, "width": width, "looking_entries": len(ctl.looking_tables)})[case] = {
                "selected_rows": rows, "whole_call_ms": spread(whole[1:]), "device_ms": spread(device[1:]),
                "ns_per_selected_row": round(spread(whole[1:], 6)["median"] * 1e6 / rows, 3),
                "kernel_launches": int(info.group(5)), "sort_scan_calls": int(info.group(6)), "mismatching_tuples": n}
    # the yardstick: the constraint check of the CPU table
    only = [traces[T.CPU]] + [None] * (len(traces) - 1)
    only_dev = [dev[T.CPU]] + [None] * (len(traces) - 1)
    for key, tabs in (("check_constraints_cpu_table_host_columns_ms", only), ("check_constraints_cpu_table_resident_ms", only_dev)):
        whole = []
        for _ in range(a.reps + 1):
            with Stderr():
                t0 = time.perf_counter()
                report = be.check_constraints(airset, tabs, params, tables=[T.CPU])
                whole.append((time.perf_counter() - t0) * 1e3)
            assert report == [], report[:3]
        res[key] = spread(whole[1:])
    with Stderr():
        be.close()
    line = json.dumps(res)
    if a.json:
        open(a.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
