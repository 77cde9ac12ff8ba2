#!/usr/bin/env python3
"""Times ola_check_constraints on the 94 x 2^22 CPU table (padding rows: neither kernel's time depends on the data of a valid trace):

  * check_constraints_kernel alone (device time between two events around its launch, printed by the library under OLA_TIMING=1),
    for the shipped instantiation and for OLA_CHECK_NEXT=neighbour;
  * the whole call from host columns (wall clock: upload through the pinned ring, check kernel, permutation and CTL Z columns);
  * the yardstick: the interpreter quotient_kernel's time per LDE point on the same table in the same process
    (OLA_AIR_KERNELS=interpreter, ola_gpu_phase_stats' quotient phase of a whole proof whose other tables have 8 rows).

    python tools/bench_check_constraints.py [--log-n 22] [--reps 5]         -> one JSON line"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Stderr:
    """what the library writes to fd 2 inside the block"""

    def __enter__(self):
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read().decode(errors="replace")
        self.f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    os.environ["OLA_TIMING"] = "1"                     # read when the context is created
    import numpy as np
    from olavm_amd.air import ola_tables as T, tracegen
    from olavm_amd.backend import Backend
    airset = T.ola_stark(range_bits=4, limb_bits=2)
    traces, params, compress = tracegen.empty_program_instance(log_n=3, log_n_cpu=a.log_n)
    cpu = traces[0]
    assert cpu.shape == (94, 1 << a.log_n)
    n = cpu.shape[1]
    only = [cpu] + [None] * 11
    with Stderr():
        be = Backend(device=0)
    pat = re.compile(r"check_constraints_kernel: table 0, .*?: ([0-9.]+) ms")
    res = {"table": "cpu 94 x 2^%d" % a.log_n}
    for variant in ("memory", "neighbour"):
        if variant == "neighbour":
            os.environ["OLA_CHECK_NEXT"] = "neighbour"
        kernel, whole = [], []
        for _ in range(a.reps + 1):                    # the first call allocates
            with Stderr() as err:
                t0 = time.perf_counter()
                report = be.check_constraints(airset, only, params, tables=[0])
                whole.append((time.perf_counter() - t0) * 1e3)
            assert report == [], report[:3]
            kernel.append(float(pat.search(err.text).group(1)))
        os.environ.pop("OLA_CHECK_NEXT", None)
        k = sorted(kernel[1:])[len(kernel[1:]) // 2]
        res["next_from_" + variant] = {"kernel_ms": round(k, 4), "kernel_ns_per_row": round(k * 1e6 / n, 4),
                                       "whole_call_ms": round(sorted(whole[1:])[len(whole[1:]) // 2], 2), "kernel_ms_all": [round(x, 4) for x in kernel[1:]]}
    # the yardstick
    os.environ["OLA_AIR_KERNELS"] = "interpreter"
    be.proof_stats(True)
    q = []
    for _ in range(2):
        with Stderr():
            be.prove_with_traces(airset.blob(), traces, params, compress)
            ms, points, _ = be.phase_stats()["quotient"]
        q.append((ms, points))
    os.environ.pop("OLA_AIR_KERNELS")
    ms, points = min(q)
    res["interpreter_quotient"] = {"phase_ms": round(ms, 3), "points": int(points), "ns_per_point": round(ms * 1e6 / points, 4)}
    res["check_vs_quotient_per_point"] = round(res["next_from_memory"]["kernel_ns_per_row"] / res["interpreter_quotient"]["ns_per_point"], 3)
    with Stderr():
        be.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
