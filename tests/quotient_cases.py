"""Inputs of the quotient tests (tests/test_gpu_quotient.py; tests/test_quotient_reference.py checks that the traces called valid here
satisfy their AIRs): tables of the miniature ola_stark at the sizes the quotient kernels branch on, challenge sets no transcript
would draw, and traces of generic values."""
import functools

import numpy as np

from tests import zcolumn_cases as ZC
from tests.zcolumn_reference import P

MINI = dict(range_bits=4, limb_bits=2)
BETAS = dict(bitwise_beta=5, program_beta=6)       # small parameters: they have a second word, + p, below 2^64
MAXW = ZC.MAXW
NAMES = ("cpu", "memory", "bitwise", "cmp", "rangecheck", "poseidon", "poseidon_chunk", "storage_access", "tape", "sccall", "program", "prog_chunk")
POWER_OF_TWO_Q = ("bitwise", "cmp", "rangecheck", "poseidon_chunk", "tape", "sccall", "program")        # q = 1, 2, 4: no degree check
EDGE_WORDS = (P - 1, 0xFFFFFFFEFFFFFFFF, 0x00000000FFFFFFFF)


@functools.lru_cache(maxsize=None)
def airset():
    from olavm_amd.air import ola_tables as T
    s = T.ola_stark(**MINI)
    assert tuple(t.name for t in s.tables) == NAMES
    return s


def table_params(name):
    return {"bitwise": [BETAS["bitwise_beta"]], "program": [BETAS["program_beta"]]}.get(name, [])


# ---- valid traces: {source: {table name: trace}} ---------------------------------------------------------------------------
def _executed(prog):
    from olavm_amd.air import miniexec as M
    return dict(zip(NAMES, M.instance(prog, **BETAS, **MINI)[0]))


def _rows512():
    """every table at 512 rows: an executed program's table where one reaches the size in well under a second, the table's own
    generator on made-up operations where that is quicker, the generators' padding rows for the rest"""
    from olavm_amd.air import miniexec as M, ola_tables as T, tracegen as TG
    rng = np.random.default_rng(512)
    out = {"cpu": _executed(M.fibonacci(60))["cpu"], "program": _executed(M.fibonacci(28))["program"]}
    out["memory"] = M.memory_trace(M.execute(M.memory_program(100))[1]["mem"])[0]
    top = 1 << (4 * MINI["limb_bits"])
    out["bitwise"] = TG.bitwise_trace(BETAS["bitwise_beta"], MINI["limb_bits"],
                                      [(("AND", "OR", "XOR")[i % 3], int(rng.integers(0, top)), int(rng.integers(0, top))) for i in range(300)], looked_by_cpu=True)
    out["cmp"] = TG.generate_cmp_trace(TG.cmp_rows(rng, 300))
    out["rangecheck"] = TG.generate_rc_trace([(int(rng.integers(0, 1 << (2 * MINI["range_bits"]))),) + tuple(int(i % 4 == k) for k in range(4)) for i in range(300)],
                                             MINI["range_bits"])
    out["poseidon"] = TG.poseidon_padding_trace(512, 256)                                   # 256 full permutations, 256 rows of the zero input
    out["poseidon_chunk"] = TG.flag_padding_trace(T.NUM_POSEIDON_CHUNK_COLS, 512, T.COL_POSEIDON_CHUNK_IS_PADDING_LINE)
    tree = M.StorageTree()                                                                  # a write and a read of one slot: 2 x 256 tree levels
    out["storage_access"] = M.storage_trace([tree.access((1, 2, 3, 4), (5, 6, 7, 8))[0], tree.access((1, 2, 3, 4))[0]])
    out["tape"] = M.tape_trace([c for a in range(200) for c in ((a, 2 * a, "TSTORE", 1000 + 7 * a), (a, 2 * a + 1, "TLOAD", 1000 + 7 * a))])
    out["sccall"] = TG.flag_padding_trace(T.NUM_COL_SCCALL, 512, T.COL_SCCALL_IS_PADDING)
    out["prog_chunk"] = TG.flag_padding_trace(T.NUM_PROG_CHUNK_COLS, 512, T.COL_PROG_CHUNK_IS_PADDING_LINE)
    assert all(t.shape[1] == 512 for t in out.values()), {k: t.shape for k, t in out.items()}
    return out


@functools.lru_cache(maxsize=None)
def valid(source):
    """the traces of one source, made once; treat as read-only"""
    from olavm_amd.air import miniexec as M, tracegen as TG
    if source == "padding2":       # two rows wherever the generators make two; the fixed tables have their own least sizes
        return dict(zip(NAMES, TG.empty_program_instance(log_n=1, live=np.random.default_rng(2), **BETAS, **MINI)[0]))
    if source == "hash":           # memory, Poseidon, Poseidon-chunk and program-chunk rows of an execution; the program table at 256 rows
        return _executed(M.hash_program())
    if source == "hash40":         # 64 live Poseidon-chunk rows
        rows, side, _ = M.execute(M.hash_program(40))
        return {"poseidon_chunk": M.poseidon_chunk_trace(side["psdn"])[0]}
    if source == "tape":           # live tape rows
        return {"tape": _executed(M.tape_program())["tape"]}
    if source == "fib28":          # the CPU table at exactly 256 rows
        return {"cpu": _executed(M.fibonacci(28))["cpu"]}
    assert source == "rows512"
    return _rows512()


# (source, table, challenge sets): None = every set
THREE_SETS = ("random", "alphas_one_minus_one", "non_canonical")           # where the integer reference takes a second or more per set
VALID = ([("padding2", n, None) for n in NAMES] + [("hash", n, None) for n in NAMES] +
         [("hash40", "poseidon_chunk", None), ("tape", "tape", None), ("fib28", "cpu", THREE_SETS)] +
         [("rows512", n, THREE_SETS if n in ("cpu", "poseidon") else None) for n in NAMES])


# ---- challenge sets ----------------------------------------------------------------------------------------------------------
ALPHAS = {"alphas_zero": (0, 0), "alphas_one_minus_one": (1, P - 1), "alphas_zero_one": (0, 1)}
GRAND_PRODUCT = ("first_word_only", "beta_one", "minus_ones")              # (0, 1), (1, 0), (p - 1, p - 1): tests/zcolumn_cases.py
SETS = ("random",) + tuple(ALPHAS) + GRAND_PRODUCT + ("non_canonical",)


def challenge_set(name, tab, seed):
    """-> dict(ctl = [2] pairs, perm = [q][2] pairs or None, alphas = [2], raw_params: the parameters go in as word + p).
    non_canonical: every word >= p."""
    q = tab.quotient_degree_factor
    kind = name if name in GRAND_PRODUCT + ("non_canonical",) else "random"
    ctl = ZC.challenges(kind, 2, seed)
    flat = ZC.challenges(kind, 2 * q, seed + 1000)
    perm = [flat[2 * i:2 * i + 2] for i in range(q)] if tab.permutation_pairs else None
    a = ZC.challenges("random", 1, seed + 2000)[0]
    alphas = ALPHAS.get(name, a)
    if name == "non_canonical":
        alphas = (P + a[0] % ((1 << 32) - 1), MAXW)
    return dict(ctl=ctl, perm=perm, alphas=list(alphas), raw_params=name == "non_canonical")


def reduced(cs):
    return dict(ctl=ZC.reduce(cs["ctl"]), perm=None if cs["perm"] is None else [ZC.reduce(p) for p in cs["perm"]], alphas=[a % P for a in cs["alphas"]],
                raw_params=False)


# ---- generic values: nothing is divisible, and with q a power of two nothing needs to be -----------------------------------------
def generic_trace(table, n, values, seed):
    """uniform words, or (values = "edge") one of EDGE_WORDS per cell; the columns the lookup filters read are zero or one-hot per row"""
    from tests.test_gpu_stark import _random_rows_with_binary_filters
    s = airset()
    rng = np.random.default_rng(7700 + 31 * table + seed)
    tr = _random_rows_with_binary_filters(rng, s, table, n)
    if values == "edge":
        keep = ZC.filter_columns(s, table)
        edge = np.array(EDGE_WORDS, dtype=np.uint64)[rng.integers(0, 3, size=tr.shape)]
        edge[keep] = tr[keep]
        tr = edge
    return tr


def generic_zs(count, n, values, seed):
    rng = np.random.default_rng(7800 + seed)
    if values == "edge":
        return np.array(EDGE_WORDS, dtype=np.uint64)[rng.integers(0, 3, size=(count, n))]
    return rng.integers(0, P, size=(count, n), dtype=np.uint64)
