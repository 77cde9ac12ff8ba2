"""The cases of tests/test_gpu_closing6.py: what runs on the 6-bit closing passes of the large transforms (ntt2t.cuh), and the same
cases as a child process whose environment selects another pass plan (OLA_NTT2_CLOSE6 is read once per process):

    python -m tests.closing6_cases L OUT.json

runs every (operation, input kind, column count) at 2^L on the device and writes the SHA-256 of each output array and the pass
kernels ola_gpu_ntt_pass_times saw; the parent compares the digests with the oracle's words."""
import hashlib
import json
import sys

import numpy as np

from tests import transform_cases as TC
from tests.oracle_lib import P

# natural-order closing pass forward and inverse; bit-reversed closing pass with per-coset powers (two cosets); a single coset
OPS = ("evaluate", "interpolate", "lde_leaf1", "coset_evaluate7")
KINDS = ("random", "tiled")
COLUMNS = (1, 8, 9)          # a lone column, one full eight-column block of a workgroup, a block and one column
EDGE = np.array([0, 1, P - 1, P, 2**32 - 1, 2**32, 0xFFFFFFFF00000000, 2**64 - 1], dtype=np.uint64)


def inputs(L, kind):
    """Nine columns of 2^L words: any u64 (random), or the words at the limits of the field and of the 32-bit halves, tiled with
    a period and a phase that differ from column to column and drift from row to row of a 64-word tile."""
    n = 1 << L
    if kind == "random":
        return np.random.default_rng(9600 + L).integers(0, 1 << 64, size=(9, n), dtype=np.uint64, endpoint=False)
    j = np.arange(n, dtype=np.int64)
    return np.stack([EDGE[(j * (2 * c + 1) + (j >> 6) * (c % 3) + c) % 8] for c in range(9)])


def device(be, op, cols):
    from olavm_amd.backend import OLA_NTT_COSET_LDE, OLA_NTT_COSET_LDE_LEAF_ORDER, OLA_NTT_EVALUATE, OLA_NTT_INTERPOLATE
    if op == "evaluate":
        return be.ntt(OLA_NTT_EVALUATE, cols)
    if op == "interpolate":
        return be.ntt(OLA_NTT_INTERPOLATE, cols)
    if op == "lde_leaf1":
        return be.ntt(OLA_NTT_COSET_LDE_LEAF_ORDER, cols, shift=7, blowup_log=1)
    assert op == "coset_evaluate7"
    return be.ntt(OLA_NTT_COSET_LDE, cols, shift=7, blowup_log=0)


def expected(oracle, op, L, cols):
    """The oracle's words for `op` on every column of `cols`, in the device's output order."""
    if op == "evaluate":
        return TC.reference(oracle, "evaluate", L, cols)[("evaluate", None)]
    if op == "interpolate":
        return TC.reference(oracle, "interpolate", L, cols)[("interpolate", None)]
    if op == "lde_leaf1":
        return TC.reference(oracle, "lde8", L, cols, blowups=(1,))[("coset_lde", 1)][:, TC.bitrev_perm(L + 1)]
    assert op == "coset_evaluate7"
    return TC.reference(oracle, "coset_evaluate", L, cols, shifts=(7,))[("coset_lde", 7)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


def key(op, kind, ncols):
    return "%s/%s/%d" % (op, kind, ncols)


def main(argv):
    if len(argv) != 2:
        print("usage: python -m tests.closing6_cases L OUT.json", file=sys.stderr)
        return 2
    L, out_path = int(argv[0]), argv[1]
    from olavm_amd.backend import Backend
    be = Backend(device=0)
    be.ntt_pass_times(True)
    out = {"L": L, "sha256": {}}
    for kind in KINDS:
        cols = inputs(L, kind)
        for op in OPS:
            for ncols in COLUMNS:
                out["sha256"][key(op, kind, ncols)] = digest(device(be, op, cols[:ncols]))
    out["pass_kernels"] = sorted(be.ntt_pass_times())
    be.close()
    with open(out_path, "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
