"""Runs tests/host_verify_api_check.cpp -- ola_host::prove_with_traces, then ola_host::verify_proof, then one flipped bit, and the opening
level, against the C++ mirror of the reference's interfaces (include/ola_host.hpp) -- on the GPU, and holds what the program reports to
the oracle's verifier on the same bytes."""
import os
import re
import subprocess

import pytest

from olavm_amd.air import ola_tables as T
from tests.test_gpu_host_api import write_fixture
from tests.test_gpu_verify import oracle_says

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(out_dir):
    """as tests/host_api_build.py builds its program: g++, warning-free, against the in-tree library"""
    exe = os.path.join(str(out_dir), "host_verify_api_check")
    lib = os.path.join(ROOT, "olavm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "host_verify_api_check.cpp"), "-o", exe, "-L" + lib, "-lola_gpu", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_cpp_host_layer_proves_verifies_and_reports_a_flipped_bit_as_the_oracle_does(tmp_path, oracle):
    from olavm_amd.air import miniexec as M
    from olavm_amd.backend import VERIFY_REASONS
    s = T.ola_stark(range_bits=4, limb_bits=2)
    blob = s.blob()
    traces, params, compress = M.instance(M.mixed_program())
    logs = [int(t.shape[1]).bit_length() - 1 for t in traces]
    fixture, proof_path, bad_path = tmp_path / "fixture.bin", tmp_path / "proof.bin", tmp_path / "tampered.bin"
    write_fixture(fixture, [[0], blob, logs, params, compress, [t.n_params for t in s.tables]] + list(traces))
    r = subprocess.run([build(tmp_path), str(fixture), str(proof_path), str(bad_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    proof, bad = open(proof_path, "rb").read(), open(bad_path, "rb").read()
    assert oracle.verify_all_proof(blob, proof, params) == (0, "")
    m = re.search(r"tampered: reason (\d+) table (-?\d+) query (-?\d+) oracle_or_layer (-?\d+) message (.*)", r.stdout)
    ok, reason, table = oracle_says(*oracle.verify_all_proof(blob, bad, params))
    assert not ok and VERIFY_REASONS[int(m.group(1))] == reason and int(m.group(2)) == (-1 if table is None else table), r.stdout
