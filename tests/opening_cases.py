"""Inputs of the opening-phase tests (tests/test_gpu_opening_edges.py and the `openeval` job of tests/alt_path_child.py): coefficient
columns that sit on the edges of the evaluation kernels' arithmetic and indexing, and opening points / FRI challenges that no
transcript would draw."""
import numpy as np

from tests.opening_reference import P, ext_pow

MAIN_COLS, MAIN_NPERM = (9, 5, 4), 2
U3 = pow(7, (P - 1) // 3, P)                     # of multiplicative order 3
KINDS = ("p-1", "halves_max", "low_ones", "impulse_0", "impulse_seam-1", "impulse_seam", "impulse_n-seam", "impulse_n-1", "ramp", "random")


def stress_column(log_n, kind, rng):
    n = 1 << log_n
    h = (log_n + 1) // 2                          # z^k = lo[k mod 2^h] hi[k >> h] in the kernels' power tables
    if kind == "p-1":
        return np.full(n, P - 1, dtype=np.uint64)
    if kind == "halves_max":
        return np.full(n, 0xFFFFFFFEFFFFFFFF, dtype=np.uint64)
    if kind == "low_ones":
        return np.full(n, 0x00000000FFFFFFFF, dtype=np.uint64)
    if kind.startswith("impulse_"):
        k = {"0": 0, "seam-1": (1 << h) - 1, "seam": 1 << h, "n-seam": n - (1 << h), "n-1": n - 1}[kind[8:]]
        c = np.zeros(n, dtype=np.uint64)
        c[k] = 1
        return c
    if kind == "ramp":
        return np.arange(n, dtype=np.uint64)      # k mod p = k
    return rng.integers(0, P, size=n, dtype=np.uint64)


def stress_batches(log_n, cols):
    """coefficient columns of the trace, zs and quotient batches: the kinds in turn over all the columns, a function of the shape"""
    rng = np.random.default_rng(9100 + log_n)
    out, k = [], 0
    for c in cols:
        out.append(np.stack([stress_column(log_n, KINDS[(k + i) % len(KINDS)], rng) for i in range(c)]))
        k += c
    return out


def challenge_sets(log_n, nlayers):
    """[(name, zeta, alpha, betas)]; the same beta for every layer"""
    rng = np.random.default_rng(9200 + log_n)
    r = [tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in range(3)]
    sets = [("random", r[0], r[1], r[2]),
            ("base_zeta", (3, 0), (0, 1), (1, 0)),
            ("x_zeta", (0, 1), (1, 0), (0, 0)),
            ("minus_ones", (P - 1, P - 1), (0, 0), (P - 1, P - 1)),
            ("order3_zeta", (U3, 0), (P - 1, 0), (0, 1)),
            ("non_canonical", (3 + P, 5 + P), (2 + P, P), (P, 1 + P))]
    for _, zeta, _, _ in sets:
        assert ext_pow((zeta[0] % P, zeta[1] % P), 1 << log_n) != (1, 0), "zeta is in the subgroup"
    return [(name, zeta, alpha, [beta] * nlayers) for name, zeta, alpha, beta in sets]
