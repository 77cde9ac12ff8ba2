#!/usr/bin/env python3
"""Writes tests/golden/ref_verified/wide_program_keccak.proof: the GPU prover's AllProof of tests/make_ref_verdict.instance() under
KeccakGoldilocksConfig (OLA_HASH_KECCAK).  The oracle has no Keccak configuration, so this proof comes from the device;
tests/make_ref_verdict_keccak.py has the reference, run from its source, judge it, and tests/test_gpu_keccak.py pins it.
usage: python tools/prove_fixture_keccak.py [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from olavm_amd.air import ola_tables as T  # noqa: E402
from olavm_amd.backend import Backend  # noqa: E402
from tests.make_ref_verdict import instance  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_verified", "wide_program_keccak.proof")
traces, params, compress = instance()
be = Backend(device=0, hasher="keccak")
raw = bytes(be.prove_with_traces(T.ola_stark().blob(), traces, params, compress))
be.close()
open(out, "wb").write(raw)
print("wrote", out, len(raw), "bytes")
