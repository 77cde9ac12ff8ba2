"""The AIR-set parser (olavm_amd/csrc/airset_host.h) on the host: parse_airset returns only sets whose constraint programs,
permutation pairs and lookup columns stay inside their tables, for every entry point at once.  tests/host_airset_check.cpp in a
program of its own, built plain and with -fsanitize=address,undefined and run directly; and the one definition of the op word's
layout and of the opcodes' meaning in the library's sources."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "olavm_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_blobs_parse_and_every_index_out_of_range_is_refused(tmp_path, flags):
    from olavm_amd.air import ola_tables as T
    from tests.test_gpu_stark import mini_set
    blobs = [T.ola_stark(range_bits=4, limb_bits=2).blob(), T.ola_stark().blob(), mini_set(4).blob()]
    words = [len(blobs)]
    for b in blobs:
        words += [b.size] + [int(x) for x in b]
    path = tmp_path / "blobs.bin"
    np.array(words, dtype="<u8").tofile(str(path))
    exe = tmp_path / "host_airset_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe), os.path.join(ROOT, "tests", "host_airset_check.cpp")])
    r = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"mutations: ops (\d+) pairs (\d+) lookups (\d+) dimensions (\d+) framing (\d+)\n0 failed", r.stdout)
    assert m, r.stdout
    ops, pairs, lookups, dims, framing = map(int, m.groups())
    assert ops > 0 and pairs > 0 and lookups > 0 and dims == 3 * 12 and framing == 3


def _function(text, head):
    """the text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    start = text.index(head)
    return text[start:text.index("\n}\n", start)]


def test_the_op_word_and_the_opcodes_have_one_definition():
    """one decoder (air_op), one device interpreter (air_interpret), and the verifier's own evaluation over the extension field"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("check.hip", "stark.hip", "verify_host.h", "airset_host.h", "air_interp.cuh")}
    for f in ("check.hip", "stark.hip", "verify_host.h", "air_interp.cuh"):
        assert not re.search(r">>\s*(16|32|48)\) & 0xffff", src[f]), f
    for f in ("check.hip", "verify_host.h", "air_interp.cuh"):
        assert "air_op(" in src[f], f
    assert len(re.findall(r">>\s*(16|32|48)\) & 0xffff", src["airset_host.h"])) == 3 and ">> 48" in _function(src["airset_host.h"], "GL_HD AirOp air_op(")
    assert "case AOP_ADD" not in src["check.hip"] and "case AOP_ADD" not in src["stark.hip"]
    assert src["air_interp.cuh"].count("case AOP_ADD") == 1
    assert src["verify_host.h"].count("case AOP_ADD") == 1 and "case AOP_ADD" in _function(src["verify_host.h"], "inline void eval_vanishing_poly(")
    assert "AOP_" not in _function(src["check.hip"], "static void launch_check_constraints(")
    for f in ("check.hip", "stark.hip"):
        assert "air_interpret(" in src[f], f
    assert not any("dev_lincol_fast" in s for s in src.values())
    # parse_airset validates before it returns, and nothing else makes an HAirSet
    assert "validate_airset(s);\n    return s;" in _function(src["airset_host.h"], "inline HAirSet parse_airset(")
