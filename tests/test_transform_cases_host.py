"""The helpers of the transform matrix on the CPU: the restated pass plans, the stress columns, the oracle as an inverse pair
on them, and the child of tests/test_gpu_fallback_paths.py as far as it goes without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import transform_cases as TC
from tests.oracle_lib import EDGE, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = 0xFFFFFFFFFFFFFFFF


def test_pass_plan_is_the_planners_table():
    assert {L: TC.pass_plan(L) for L in TC.SIZES} == {14: [7, 7], 15: [7, 8], 16: [8, 8], 17: [5, 6, 6], 18: [6, 6, 6]}
    for L in range(14, 29):
        plan = TC.pass_plan(L)
        assert sum(plan) == L and len(plan) == (L + 7) // 8
        assert plan == sorted(plan) and plan[-1] - plan[0] <= 1 and 5 <= plan[0] and plan[-1] <= 8
    assert TC.pass_bits(17) == [(12, 5), (6, 6), (0, 6)]
    # the inverse middle passes of width 7 and 8, which the matrix leaves to the tests of 2^20 and more
    assert TC.pass_plan(20) == [6, 7, 7] and TC.pass_plan(23) == [7, 8, 8]
    assert all(TC.pass_plan(L)[1:-1] in ([], [6]) for L in TC.SIZES)


def test_predicted_kernels_follow_the_planners_rules():
    k = lambda *a: "ntt2t_pass_kernel<%d,%d,%s,8,%d>" % a
    assert TC.predicted_kernels(14, "evaluate") == {k(7, 0, "false", 0), k(7, 2, "false", 2)}
    assert TC.predicted_kernels(15, "lde8") == {k(7, 0, "false", 1), k(8, 1, "false", 2)}
    assert TC.predicted_kernels(17, "coset_evaluate") == {k(5, 0, "false", 1), k(6, 0, "false", 1), k(6, 2, "false", 2)}
    # the inverse cases also run the forward transform they invert; an inverse first pass has no load multiplier
    assert TC.predicted_kernels(17, "coset_interpolate") == {k(5, 0, "true", 0), k(6, 0, "true", 1), k(6, 2, "true", 2)} | TC.predicted_kernels(17, "coset_evaluate")
    assert TC.operations(14)[-1] == "lde_rates" and "lde_rates" not in TC.operations(15)


@pytest.mark.parametrize("L", TC.SIZES)
def test_stress_columns_shape_and_contents(L):
    n = 1 << L
    c = TC.stress_columns(L, TC.stress_rng(L))
    assert c.shape == (11, n) and c.dtype == np.uint64
    assert np.array_equal(c, TC.stress_columns(L, TC.stress_rng(L)))          # a function of L alone
    assert (c[0] == ONES).all() and (c[1] == P - 1).all()
    j = np.arange(n, dtype=np.uint64)
    k = 2
    for lo, R in TC.pass_bits(L):
        for b in (lo, lo + R - 1):
            bit = ((j >> np.uint64(b)) & np.uint64(1)).astype(bool)
            assert (c[k][bit] == ONES).all() and (c[k][~bit] == 0).all() and bit.sum() == n // 2
            k += 1
    assert k == 2 + 2 * len(TC.pass_plan(L))
    assert np.array_equal(c[k], np.resize(EDGE, n))
    assert (c[k + 1] >= P).all()
    assert k + 2 < 11 and (c[k + 2:] < P).all() and len({r.tobytes() for r in c[k + 2:]}) == 11 - k - 2


def test_bitrev_perm_and_canon():
    assert TC.bitrev_perm(3).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]
    r = TC.bitrev_perm(15)
    assert np.array_equal(r[r], np.arange(1 << 15))
    assert TC.canon(np.array([0, P - 1, P, ONES], dtype=np.uint64)).tolist() == [0, P - 1, 0, ONES - P]


@pytest.mark.parametrize("L", TC.SIZES)
def test_oracle_round_trips_the_stress_columns(oracle, L):
    """interpolate(evaluate(x)) is the canonical form of x, words >= p included, plain and on the cosets 7 and 49."""
    for x in TC.stress_columns(L, TC.stress_rng(L)):
        ev = oracle.evaluate_poly(x)
        assert ev.max() < P
        assert np.array_equal(oracle.interpolate_poly(ev), TC.canon(x))
        assert np.array_equal(ev, oracle.evaluate_poly(TC.canon(x)))
    for shift in TC.SHIFTS:
        for x in TC.stress_columns(L, TC.stress_rng(L))[[0, 2, 9]]:
            ev = oracle.evaluate_poly_with_offset(x, shift, 1)
            assert np.array_equal(oracle.interpolate_poly_with_offset(ev, shift), TC.canon(x))


@pytest.mark.parametrize("job", ["transforms:14", "open:blake3", "prove"])
def test_child_dry_run_builds_inputs_and_oracle_side_without_the_gpu_library(job, tmp_path):
    out = tmp_path / "dry.json"
    r = subprocess.run([sys.executable, "-m", "tests.alt_path_child", "--dry", job, str(out)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(out.read_text())
    assert got["job"] == job and got["dry"] is True and got["gpu_library_loaded"] is False
    assert got["oracle_sha256"]
    if job == "transforms:14":
        assert got["ops"] == TC.operations(14) and sorted(got["oracle_sha256"]) == sorted(TC.operations(14))


def test_child_dry_run_of_the_opening_evaluation_job(tmp_path):
    """openeval:15 without a GPU: the inputs and the integer reference's side, which is a function of the size alone."""
    from tests import alt_path_child as child, opening_cases as OC
    out = tmp_path / "dry.json"
    r = subprocess.run([sys.executable, "-m", "tests.alt_path_child", "--dry", "openeval:15", str(out)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(out.read_text())
    assert got["job"] == "openeval:15" and got["dry"] is True and got["gpu_library_loaded"] is False
    assert got["sets"] == list(child.OPENEVAL_SETS) and sorted(got["reference_sha256"]) == sorted(child.OPENEVAL_SETS)
    assert len(set(got["reference_sha256"].values())) == 3
    batches, sets = child.openeval_inputs(15)
    assert [b.shape for b in batches] == [(c, 1 << 15) for c in OC.MAIN_COLS] and all(b.dtype == np.uint64 and b.max() < P for b in batches)
    assert [len(c[3]) for c in sets] == [3, 3, 3]


@pytest.mark.parametrize("log_n", [3, 15, 18])
def test_opening_stress_columns_are_what_the_table_says(log_n):
    from tests import opening_cases as OC
    n, h = 1 << log_n, (log_n + 1) // 2
    t, z, q = OC.stress_batches(log_n, OC.MAIN_COLS)
    assert (t[0] == P - 1).all() and (t[1] == 0xFFFFFFFEFFFFFFFF).all() and (t[2] == 0xFFFFFFFF).all() and t.max() < P
    for col, k in zip(list(t[3:8]) + list(q), [0, (1 << h) - 1, 1 << h, n - (1 << h), n - 1, (1 << h) - 1, 1 << h, n - (1 << h), n - 1]):
        assert col[k] == 1 and col.sum() == 1
    assert np.array_equal(t[8], np.arange(n, dtype=np.uint64)) and (z[1] == P - 1).all() and z[0].max() < P
    assert all(np.array_equal(a, b) for a, b in zip((t, z, q), OC.stress_batches(log_n, OC.MAIN_COLS)))
    names = [c[0] for c in OC.challenge_sets(log_n, 2)]
    assert names == ["random", "base_zeta", "x_zeta", "minus_ones", "order3_zeta", "non_canonical"]
    assert pow(OC.U3, 3, P) == 1 and OC.U3 != 1


def test_child_refuses_an_unknown_job(tmp_path):
    r = subprocess.run([sys.executable, "-m", "tests.alt_path_child", "--dry", "nonsense", str(tmp_path / "x.json")], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "unknown job" in r.stderr
