"""The batch size of the proof-of-work search (olavm_amd/csrc/pow_batch.h) for proof_of_work_bits 1..40, on the host:
tests/host_pow_batch_check.cpp in a program of its own, built plain and with -fsanitize=address,undefined and run directly.  The sizes of
37..40 bits, whose workgroup count did not fit a launch, are never searched on a device by the suite; what reaches the device is
tests/test_gpu_configs.py's searches of 1, 8, 12 and 20 bits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_every_batch_of_1_to_40_bits_fits_a_grid(tmp_path, flags):
    exe = tmp_path / "host_pow_batch_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), os.path.join(ROOT, "tests", "host_pow_batch_check.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "bits 1..40: every batch fits a grid" in r.stdout


def test_the_library_uses_the_helper():
    """one definition: both launch sites of the search take their size from pow_batch.h"""
    csrc = os.path.join(ROOT, "olavm_amd", "csrc")
    merkle, fri = open(os.path.join(csrc, "merkle.hip")).read(), open(os.path.join(csrc, "fri.hip")).read()
    assert '#include "pow_batch.h"' in merkle and "pow_batch(bits)" in merkle and "pow_batch(bits)" in fri
    assert "4 << bits" not in merkle and "4 << bits" not in fri
