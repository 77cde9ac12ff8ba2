"""The paths that an environment switch selects once per process: the canonical-arithmetic transform passes
(OLA_NTT2_TFORM=0: the A/B control, and the only path of transforms of 2^29 points and more) and the kernels that the opening
proof's newer ones replaced (OLA_EVAL_WIDE=0, OLA_FOLD16=0, OLA_LEAF_EXT_STAGED=0, OLA_MERKLE_FUSED_LEVELS, OLA_POW_DEFER=0), and
the wide evaluation's steps per workgroup (OLA_EVAL_WIDE_KH), which the occupancy rule raises above 32 only from 2^22 rows on, and
the pool's blocks handed out filled with 0xFF bytes (OLA_POOL_POISON=1), which turns a word that a kernel reads and nobody wrote
into a wrong result.
DESIGN.md and PARITY.md call every one of them bit-exact; here each runs in a child process (tests/alt_path_child.py) with the
switch in its environment and its words / bytes are compared with the CPU oracle's.

One child at a time.  A child that times out, aborts or dies of a signal ends the whole run (pytest.exit): nothing more is
started on a GPU that may have faulted, and nothing is tried again.

CHILD_TIMEOUT: measured on the MI355X (wall time of the whole child process: Python start, library load, context, the oracle
side of the transform jobs): transforms:14 .. transforms:18 2.5, 2.4, 2.5, 2.9 and 3.5 s, open:* 2.1 - 2.3 s, prove 2.2 s.  Ten times
the slowest is 35 s; the limit is the floor of 60 s.

The expected bytes of the opening jobs come from the oracle PROVER, once per module and hasher (measured on an 8-core host
without a GPU: 0.9 s under Blake3, 5.5 s under Poseidon for the 2^15-row instance), not from the default path."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import alt_path_child as child, transform_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 60
FATAL_STATUS = (-6, -11, 134, 139, 124, 137)


def run_child(job, env, tmp_path):
    out = tmp_path / "out.json"
    e = dict(os.environ)
    e.update(env)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.alt_path_child", job, str(out)], cwd=ROOT, env=e, timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as x:
        pytest.exit("child %s %s did not finish in %d s; nothing more is started on the GPU\n%s" % (job, env, CHILD_TIMEOUT, x.stderr), returncode=3)
    if r.returncode in FATAL_STATUS:
        pytest.exit("child %s %s ended with status %d; nothing more is started on the GPU\n%s" % (job, env, r.returncode, r.stderr[-4000:]), returncode=3)
    assert r.returncode == 0, "child %s %s: status %d\n%s" % (job, env, r.returncode, r.stderr[-4000:])
    print("child %s %s: %.1f s" % (job, env, time.perf_counter() - t0))
    return json.loads(out.read_text())


# ------------------------------------------------------------------------------------------------ canonical-arithmetic passes
@pytest.mark.parametrize("L", TC.SIZES)
def test_canonical_passes_match_oracle(L, tmp_path):
    """ntt2_pass_kernel: the whole matrix of test_gpu_transform_matrix.py at 2^L.  The T-form passes are the ones
    ola_gpu_ntt_pass_times records, so an empty report says that the canonical passes ran."""
    got = run_child("transforms:%d" % L, {"OLA_NTT2_TFORM": "0"}, tmp_path)
    assert got["ops"] == TC.operations(L)
    assert got["pass_kernels"] == [], "the T-form passes ran"
    assert not got["mismatches"], "(operation, L, column, first differing index): %s" % got["mismatches"][:12]


# ------------------------------------------------------------------------------------------------ opening proof
@pytest.fixture(scope="module")
def open_expected(oracle):
    memo = {}

    def get(hasher):
        if hasher not in memo:
            memo[hasher] = child.open_expected(oracle, hasher)
        return memo[hasher]
    return get


@pytest.mark.parametrize("hasher,env", [("poseidon", {"OLA_EVAL_WIDE": "0"}), ("poseidon", {"OLA_FOLD16": "0"}),
                                        ("blake3", {"OLA_LEAF_EXT_STAGED": "0"}), ("blake3", {"OLA_MERKLE_FUSED_LEVELS": "1"}),
                                        ("blake3", {"OLA_MERKLE_FUSED_LEVELS": "3"})],
                         ids=["eval_wide_0", "fold16_0", "leaf_ext_staged_0", "merkle_fused_levels_1", "merkle_fused_levels_3"])
def test_opening_proof_fallback_bytes_match_oracle(oracle, open_expected, hasher, env, tmp_path):
    """2^15 rows is the smallest size at which every switch changes the path: eval_points_kernel instead of the wide
    evaluation (log_n >= 15), fold_kernel on the first layer (2^18 coefficients of which at least 4096 are non-zero), one
    launch per Blake3 leaf of the 2^14-leaf FRI layer, one or three Merkle levels per launch above 256 nodes."""
    got = run_child("open:" + hasher, env, tmp_path)
    o_open, o_fri, o_next = open_expected(hasher)
    assert bytes.fromhex(got["open"]) == o_open, "opening set bytes differ"
    assert bytes.fromhex(got["fri"]) == o_fri, "FRI proof bytes differ"
    assert got["challenge"] == o_next, "the transcripts end in different states"


# ------------------------------------------------------------------------------------------------ wide evaluation, long loops
@pytest.fixture(scope="module")
def openeval_expected():
    memo = {}

    def get(log_n):
        if log_n not in memo:
            memo[log_n] = child.openeval_expected(log_n)
        return memo[log_n]
    return get


@pytest.mark.parametrize("log_n,kh", [(15, 2), (18, 64), (18, 512), (15, 512)])
def test_wide_evaluation_steps_per_workgroup_match_the_integer_reference(openeval_expected, log_n, kh, tmp_path):
    """eval_points_wide_kernel's load, step and split loop at lengths the occupancy rule (olavm_amd/csrc/eval_plan.h) reaches only
    at 2^22 rows and more: 2 steps at 2^15 rows (64 splits), 64 and 512 at 2^18 (nhi = 512: the whole 1024-product sum in one
    workgroup), 512 at 2^15 (clamped to nhi = 128) -- on columns whose 32-bit halves are at their maximum, at a random zeta,
    zeta = (p-1, p-1) and a zeta of order 3.  The hi-table limbs of a chosen zeta cannot all be at their maximum: the 2^64 bound of
    the sums stays with the device self-test."""
    got = run_child("openeval:%d" % log_n, {"OLA_EVAL_WIDE_KH": str(kh)}, tmp_path)
    want = openeval_expected(log_n)
    assert got["coeffs_kept"] and got["sets"] == list(child.OPENEVAL_SETS)
    for name in child.OPENEVAL_SETS:
        assert bytes.fromhex(got["open"][name]) == want[name][0], "opening set bytes differ at the challenge set %s" % name
        assert [tuple(r) for r in got["final"][name]] == want[name][1], "final polynomial differs at the challenge set %s" % name


@pytest.mark.parametrize("log_n", [12, 16])
def test_stepped_opening_on_poisoned_pool_blocks(oracle, log_n, tmp_path):
    """OLA_POOL_POISON=1: the stepped opening of the stress columns where every block of the pool starts as all-ones words.  The
    pool gives a call sequence the same blocks in the same roles, and the driver's fresh blocks are zero, so without the switch a
    kernel that reads what nobody wrote reads zeros run after run.  What depends on it here: fold_pairs_kernel<4> writes nz / 16 outputs
    and leaves the rest of the layer's planes to a memset (2^12 rows: the first fold; 2^16 rows: the first two); those words enter
    no word of the final polynomial, only the NEXT layer's committed values -- so the caps are compared, with the oracle's
    transform and tree over the integer reference's folded polynomials."""
    got = run_child("openeval:%d" % log_n, {"OLA_POOL_POISON": "1"}, tmp_path)
    want = child.openeval_expected(log_n, oracle)
    assert got["coeffs_kept"] and got["sets"] == list(child.OPENEVAL_SETS)
    for name in child.OPENEVAL_SETS:
        assert bytes.fromhex(got["open"][name]) == want[name][0], "opening set bytes differ at the challenge set %s" % name
        assert [tuple(r) for r in got["final"][name]] == want[name][1], "final polynomial differs at the challenge set %s" % name
        wrong = [i for i, (g, w) in enumerate(zip(got["caps"][name], want[name][2])) if g != w]
        assert len(got["caps"][name]) == len(want[name][2]) and not wrong, "the caps of the layers %s differ at the challenge set %s" % (wrong, name)


# ------------------------------------------------------------------------------------------------ proof of work in line
@pytest.fixture(scope="module")
def prove_expected(oracle):
    return child.prove_expected(oracle)


def test_pow_in_line_proof_bytes_match_oracle(prove_expected, tmp_path):
    """OLA_POW_DEFER=0: every table's proof-of-work witness is searched where the reference searches it, not after the other
    tables' openings were queued."""
    got = run_child("prove", {"OLA_POW_DEFER": "0"}, tmp_path)
    assert [bytes.fromhex(p) for p in got["proofs"]] == prove_expected
