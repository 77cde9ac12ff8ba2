"""include/ola_host.hpp `ola_host::check_constraints` through tests/host_check_constraints.cpp: the program compiles warning-free against
the in-tree library (CPU), and on the GPU prints the report the Python layer gives for the same instance."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(out_dir):
    exe = os.path.join(str(out_dir), "host_check_constraints")
    lib = os.path.join(ROOT, "olavm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "host_check_constraints.cpp"), "-o", exe, "-L" + lib, "-lola_gpu", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_host_check_program_compiles_and_explains_itself(tmp_path):
    from olavm_amd.backend import load_library
    load_library()
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_host_layer_gives_the_python_layers_report(tmp_path):
    from olavm_amd.air import miniexec as M, ola_tables as T
    from olavm_amd.backend import Backend
    airset = T.ola_stark(range_bits=4, limb_bits=2)
    traces, params, _ = M.instance(M.mixed_program())
    traces = [t.copy() for t in traces]
    traces[0][7, 9] ^= np.uint64(1)            # cpu
    traces[8][0, 1] += np.uint64(5)            # tape
    blob = airset.blob()
    words = [blob.size] + [int(x) for x in blob] + [len(params)] + [int(x) for x in params] + [len(traces)]
    for t in traces:
        words += [int(t.shape[1]).bit_length() - 1, t.size] + [int(x) for x in np.ascontiguousarray(t).reshape(-1)]
    path = os.path.join(str(tmp_path), "instance.bin")
    np.array(words, dtype="<u8").tofile(path)
    be = Backend(device=0)
    want = be.check_constraints_raw(blob, traces, params, cap=4096)[0]
    only_tape = be.check_constraints_raw(blob, traces, params, tables=[8], cap=4096)[0]
    be.close()
    assert any(e[0] == 0 for e in want) and any(e[0] == 8 for e in want) and only_tape and all(e[0] == 8 for e in only_tape)
    exe = build(tmp_path)
    for args, expect in (([], want), ([str(1 << 8)], only_tape)):
        r = subprocess.run([exe, path] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [tuple(int(x) for x in line.split()) for line in r.stdout.strip().split("\n")]
        assert got == expect
