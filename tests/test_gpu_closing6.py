"""The 6-bit closing passes of the large transforms against the oracle, word for word.

A 6-bit closing pass (ntt2t.cuh) loads its tile a 512-byte row per wave, passes it through the exchange buffer to a thread map in
which each wave has one second-round index, and applies its round twiddles as shifts by that wave's constants.  The planner
(ntt2.hip: ntt2t_widths) gives the closing pass 6 bits at 2^17 .. 2^22 and 2^25 .. 2^28; OLA_NTT2_CLOSE6=0 selects the even split
everywhere, OLA_NTT2_CLOSE6=2 runs 2^14 as 8+6 too.  The switch is read once per process, so the other plans run in a child.

Sizes: 2^20 (7+7+6, three passes; 6+7+7 under OLA_NTT2_CLOSE6=0) and 2^14 (two passes: 7+7 by default, 8+6 under
OLA_NTT2_CLOSE6=2 -- a strided pass that feeds the closing pass directly).  Operations (tests/closing6_cases.py): evaluate and
interpolate (natural-order closing pass, forward and inverse), the leaf-order coset LDE with blowup_log = 1 (bit-reversed closing
pass with per-coset powers, two cosets), coset evaluate at shift 7.  Columns 1, 8 and 9: the edge of the eight-column block of a
workgroup.  Inputs: any u64, and a tiling of the words at the limits of the field and of the 32-bit halves.  The matrix of
test_gpu_transform_matrix.py runs the same kernels at 2^17 and 2^18 on its stress columns.

Measured on the MI355X: a 2^20 case 0.35 s (the LDE 1.0 s), a 2^14 case under 0.05 s, the children 4.8 s (2^20: process start,
24 transforms, and the oracle's side where this process has not computed it yet) and 2.1 s.  The oracle's words of a case are
computed once on nine columns; the 1- and 8-column runs compare with their first rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import closing6_cases as CC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 60
FATAL_STATUS = (-6, -11, 134, 139, 124, 137)

_want = {}   # (L, op, kind) -> the oracle's words on the nine columns: computed once, shared with the child cases


def want_for(oracle, L, op, kind):
    if (L, op, kind) not in _want:
        w = CC.expected(oracle, op, L, CC.inputs(L, kind))
        w.setflags(write=False)
        _want[(L, op, kind)] = w
    return _want[(L, op, kind)]


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    b.ntt_pass_times(True)
    yield b
    b.close()


def widths(kernels, closing):
    """{R} of the closing-pass (MODE 1 or 2) or of the strided (MODE 0) kernels among the names ola_gpu_ntt_pass_times reports"""
    out = set()
    for k in kernels:
        r, mode = k[k.index("<") + 1:].split(",")[:2]
        if (mode != "0") == closing:
            out.add(int(r))
    return out


@pytest.mark.parametrize("kind", CC.KINDS)
@pytest.mark.parametrize("op", CC.OPS)
@pytest.mark.parametrize("L", [14, 20])
def test_closing_pass_matches_oracle(be, oracle, L, op, kind):
    cols, want = CC.inputs(L, kind), want_for(oracle, L, op, kind)
    be.ntt_pass_times()
    for ncols in CC.COLUMNS:
        got = CC.device(be, op, cols[:ncols])
        assert got.shape == want[:ncols].shape
        bad = np.argwhere(got != want[:ncols])
        assert bad.size == 0, "%s of %d columns at 2^%d: first differing (column, index) %s" % (op, ncols, L, bad[0])
    assert widths(be.ntt_pass_times(), True) == {6 if L == 20 else 7}, "not the planned closing pass"


def run_child(L, env, tmp_path):
    out = tmp_path / "out.json"
    e = dict(os.environ)
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.closing6_cases", str(L), str(out)], cwd=ROOT, env=e, timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as x:
        pytest.exit("child %d %s did not finish in %d s; nothing more is started on the GPU\n%s" % (L, env, CHILD_TIMEOUT, x.stderr), returncode=3)
    if r.returncode in FATAL_STATUS:
        pytest.exit("child %d %s ended with status %d; nothing more is started on the GPU\n%s" % (L, env, r.returncode, r.stderr[-4000:]), returncode=3)
    assert r.returncode == 0, "child %d %s: status %d\n%s" % (L, env, r.returncode, r.stderr[-4000:])
    return json.loads(out.read_text())


@pytest.mark.parametrize("L,switch,strided,closing", [(20, "0", {6, 7}, {7}), (14, "2", {8}, {6})], ids=["2p20-even-split", "2p14-8+6"])
def test_other_plans_give_the_same_words(oracle, L, switch, strided, closing, tmp_path):
    """OLA_NTT2_CLOSE6=0 at 2^20 (the even split 6+7+7: the switch itself) and OLA_NTT2_CLOSE6=2 at 2^14 (8+6: two passes), every
    case of the module in one child process: the planned kernels ran and every output array is the oracle's."""
    got = run_child(L, {"OLA_NTT2_CLOSE6": switch}, tmp_path)
    assert widths(got["pass_kernels"], True) == closing and widths(got["pass_kernels"], False) == strided
    wrong = [CC.key(op, kind, n) for kind in CC.KINDS for op in CC.OPS for n in CC.COLUMNS
             if got["sha256"][CC.key(op, kind, n)] != CC.digest(want_for(oracle, L, op, kind)[:n])]
    assert not wrong, "outputs that differ from the oracle's words: %s" % wrong
