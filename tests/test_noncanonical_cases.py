"""tests/noncanonical_cases.py by itself (CPU): the patterns of words >= p on a hand-made table set, the link-bytes model of
olavm_amd/csrc/upload.h on tables whose answer is written out by hand, and the oracle's indifference to representatives -- what
tests/test_gpu_noncanonical_traces.py expects of the GPU prover is the oracle's proof of the CANONICAL trace."""
import numpy as np
import pytest

from olavm_amd.air import miniexec as M, ola_tables as T
from tests import noncanonical_cases as NC

P = NC.P
BIG = P - 5                                                       # a canonical word no pattern may touch


def rng():
    return np.random.default_rng(2024)


@pytest.fixture(scope="module")
def handmade():
    """table 0: 4 columns x 8192 rows -- bytes, 32-bit words, field-sized words, and field-sized words around rows 4095 / 4096;
    table 1: the memory table's width x 16 rows with zeros in the two `p - x` columns and elsewhere; table 2: 2 x 8."""
    r = np.random.default_rng(1)
    t0 = np.stack([r.integers(0, 256, 8192, dtype=np.uint64), r.integers(0, 1 << 32, 8192, dtype=np.uint64), r.integers(1 << 33, P, 8192, dtype=np.uint64), r.integers(0, 1000, 8192, dtype=np.uint64)])
    t0[1, 77] = (1 << 32) - 1                                     # 2^32 - 1 + p overflows: not eligible
    t0[1, 78] = (1 << 32) - 2                                     # the largest eligible word
    t0[3, 4090:4097] = BIG
    t0[3, 8191] = BIG
    t1 = r.integers(0, 7, (T.NUM_MEM_COLS, 16), dtype=np.uint64)
    t1[NC.COL_MEM_DIFF_ADDR_COND, ::2] = 0
    t1[NC.COL_MEM_RC_VALUE, 1::3] = 0
    t1[0, :] = 0
    t2 = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [BIG] * 8], dtype=np.uint64)
    return [t0, t1, t2]


def test_the_memory_columns_are_the_tables_own():
    assert (NC.MEMORY_TABLE, NC.COL_MEM_DIFF_ADDR_COND, NC.COL_MEM_RC_VALUE) == (T.MEMORY, T.COL_MEM_DIFF_ADDR_COND, T.COL_MEM_RC_VALUE)
    assert T.ola_stark(range_bits=4, limb_bits=2).tables[NC.MEMORY_TABLE].ncols == T.NUM_MEM_COLS
    assert P == (1 << 64) - (1 << 32) + 1 and NC.ELIGIBLE_MAX + P == (1 << 64) - 1


def test_patterns_on_a_handmade_table_set(handmade):
    before = [t.copy() for t in handmade]
    sh_all, m_all = NC.shift_words(handmade, "all", rng())
    for t, s, m in zip(handmade, sh_all, m_all):
        eligible = t <= NC.ELIGIBLE_MAX
        assert not (m & ~eligible).any()
        assert np.array_equal(s[~m], t[~m]) and np.array_equal(s[m], t[m] + np.uint64(P))
        # every column with an eligible word has one shifted, its first eligible one among them; about a third of them overall
        assert np.array_equal(m.any(axis=1), eligible.any(axis=1))
        for c in np.nonzero(eligible.any(axis=1))[0]:
            assert m[c, eligible[c].argmax()]
    assert not m_all[0][2].any() and not m_all[2][1].any()        # field-sized columns stay
    assert not m_all[0][1, 77] and handmade[0][1, 78] + np.uint64(P) == np.uint64((1 << 64) - 1)
    frac = m_all[0][:2].mean()
    assert abs(frac - 1 / 3) < 0.02, frac
    assert (sh_all[1][0][m_all[1][0]] == np.uint64(P)).all() and m_all[1][0].any()      # zeros become the literal word p
    for name, keep in (("odd_columns", lambda m: m[0::2]), ("even_columns", lambda m: m[1::2]),
                       ("first_half", lambda m: m[:, m.shape[1] // 2:]), ("second_half", lambda m: m[:, :m.shape[1] // 2])):
        _, masks = NC.shift_words(handmade, name, rng())
        for m, ma in zip(masks, m_all):
            assert not keep(m).any()                              # nothing outside the named region
            rest = ma.copy()
            keep(rest)[...] = False
            assert np.array_equal(m, rest)                        # inside it: the same third
    assert all(np.array_equal(a, b) for a, b in zip(before, handmade))           # the caller's tables are left alone
    with pytest.raises(ValueError):
        NC.shift_words(handmade, "every_other_word", rng())
    with pytest.raises(AssertionError):
        NC.shift_words(sh_all, "all", rng())                      # starts from canonical traces only
    with pytest.raises(AssertionError):
        NC.shift_words([handmade[0][2:3]], "all", rng())          # no eligible word: an empty mask is refused


def test_single_patterns_pick_the_named_row(handmade):
    want_rows = {"0": (0, 0, 0), "4095": (4095, None, None), "4096": (4096, None, None), "n/2-1": (4095, 7, 3), "n/2": (4096, 8, 4),
                 "n-1": (8191, 15, 7)}
    assert sorted(want_rows) == sorted(NC.SINGLE_ROWS)
    for name, rows in want_rows.items():
        sh, masks = NC.shift_words(handmade, "single(%s)" % name, rng())
        for t, m, row in zip(handmade, masks, rows):
            if row is None:                                       # the table is shorter than the row: skipped
                assert not m.any()
                continue
            assert (m.sum(axis=1) <= 1).all()
            for c in range(t.shape[0]):
                below = np.nonzero(t[c, :row + 1] <= NC.ELIGIBLE_MAX)[0]
                assert list(np.nonzero(m[c])[0]) == ([below[-1]] if below.size else []), (name, c)
    # column 3 of table 0 holds field-sized words in rows 4090..4096 and 8191: the nearest eligible row below is taken
    for name, row in (("4095", 4089), ("4096", 4089), ("n-1", 8190)):
        _, masks = NC.shift_words(handmade, "single(%s)" % name, rng())
        assert list(np.nonzero(masks[0][3])[0]) == [row] and list(np.nonzero(masks[0][0])[0]) == [NC.SINGLE_ROWS[name](8192)]
        assert not masks[0][2].any()


def test_zeros_to_p_touches_nothing_else(handmade):
    sh, masks = NC.shift_words(handmade, "zeros_to_p", rng())
    assert not masks[0].any() and not masks[2].any()
    m = masks[1]
    cols = [NC.COL_MEM_DIFF_ADDR_COND, NC.COL_MEM_RC_VALUE]
    others = [c for c in range(m.shape[0]) if c not in cols]
    assert not m[others].any() and (handmade[1][0] == 0).all()    # column 0 is all zeros and stays
    assert np.array_equal(m[cols], handmade[1][cols] == 0) and m[cols[0]].sum() >= 8 and m[cols[1]].sum() >= 5
    assert set(np.unique(sh[1][m])) == {np.uint64(P)}
    with pytest.raises(AssertionError):                           # no zero there: refused rather than a canonical trace under this name
        NC.shift_words([handmade[0], np.ones((T.NUM_MEM_COLS, 8), dtype=np.uint64)], "zeros_to_p", rng())


# ------------------------------------------------------------------------------------------------------------------ link_bytes_model
N17, N18 = 1 << 17, 1 << 18


def model_tables():
    """With 1 MB pieces (2^17 words): table 0, 2^17 rows, one piece per column -- bytes | halves | field-sized | a 2^8 in the last word
    | a 2^32 in the last word; table 1, 2^18 rows, one column of two pieces: the first packed, the second wide; table 2: one column
    of 2048 rows."""
    r = np.random.default_rng(3)
    t0 = np.stack([r.integers(0, 256, N17, dtype=np.uint64), r.integers(0, 1 << 32, N17, dtype=np.uint64), r.integers(1 << 40, P, N17, dtype=np.uint64), r.integers(0, 256, N17, dtype=np.uint64),
                   r.integers(0, 1 << 32, N17, dtype=np.uint64)])
    t0[0, -1], t0[1, -1] = 255, (1 << 32) - 1
    t0[3, -1], t0[4, -1] = 1 << 8, 1 << 32
    t1 = r.integers(0, 1 << 32, (1, N18), dtype=np.uint64)
    t1[0, N17 - 1], t1[0, -1] = (1 << 32) - 1, P                  # the last word of the second piece is the literal word p
    t2 = r.integers(0, 256, (1, 2048), dtype=np.uint64)
    return [t0, t1, t2]


def test_link_bytes_model_on_tables_worked_out_by_hand():
    t0, t1, t2 = model_tables()
    #                 bytes   halves      field      2^8 last    2^32 last
    want0 = N17 * 1 + N17 * 4 + N17 * 8 + N17 * 4 + N17 * 8
    want1 = N17 * 4 + N17 * 8                                     # a packed first piece, a wide second one
    want2 = 2048 * 8                                              # a piece of one column, but below 4096 rows: never packed
    got, narrow = NC.link_bytes_model([t0, t1, t2], piece_mb=1)
    assert got == want0 + want1 + want2 == 4866048
    assert [list(x) for x in narrow] == [[True, True, False, True, False], [False], [False]]
    # the columns one by one
    for c, w in enumerate((1, 4, 8, 4, 8)):
        assert NC.link_bytes_model([t0[c:c + 1]], piece_mb=1)[0] == N17 * w
    # 16 MB pieces: the 1 MB columns of table 0 are pieces of their own (512 KB and more), the 2 MB column of table 1 is ONE piece now
    got, narrow = NC.link_bytes_model([t0, t1, t2])
    assert got == want0 + N18 * 8 + want2 and [list(x) for x in narrow] == [[True, True, False, True, False], [False], [False]]
    # without bytes: 4 per word where it was 1
    assert NC.link_bytes_model([t0, t1, t2], piece_mb=1, pack8=False)[0] == want0 + N17 * 3 + want1 + want2
    # no own pieces for columns shorter than a slot: the five of table 0 share one, table 1's single column is still a piece of its own
    t1n = t1.copy()
    t1n[0, -1] = 0
    got, narrow = NC.link_bytes_model([t0, t1n, t2], solo_kb=0)
    assert got == 5 * N17 * 8 + N18 * 4 + want2 and [list(x) for x in narrow] == [[False] * 5, [True], [False]]
    # two columns per 1 MB piece of a 2^16-row table, the third is left a piece to itself and travels as bytes
    t3 = np.stack([t0[0, :1 << 16]] * 3)
    got, narrow = NC.link_bytes_model([t3], piece_mb=1, solo_kb=0)
    assert got == 2 * (1 << 16) * 8 + (1 << 16) and list(narrow[0]) == [False, False, True]
    assert NC.link_bytes_model([t3], piece_mb=1)[0] == 3 * (1 << 16)             # 512 KB columns: each its own piece
    assert NC.link_bytes_model([t3], piece_mb=1, solo_kb=1024)[0] == 2 * (1 << 16) * 8 + (1 << 16)
    # packing off: every word as it is, no column narrow
    total = sum(t.size * 8 for t in (t0, t1, t2))
    got, narrow = NC.link_bytes_model([t0, t1, t2], piece_mb=1, pack=False)
    assert got == total and not any(x.any() for x in narrow)
    # columns given one by one are the same table
    assert NC.link_bytes_model([[c.copy() for c in t0], t1, t2], piece_mb=1)[0] == want0 + want1 + want2
    # a word >= p in a packed column makes its piece wide, wherever it stands in the last 4096-word block
    for row in (N17 - 4096, N17 - 1):
        s = t0[:1].copy()
        s[0, row] += np.uint64(P)
        assert NC.link_bytes_model([s], piece_mb=1) [0] == N17 * 8


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.fixture(scope="module")
def mini_blob():
    return T.ola_stark(range_bits=4, limb_bits=2).blob()


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("program", ["mixed", "memory"])
def test_the_oracle_does_not_care_about_representatives(oracle, mini_blob, program, hasher):
    traces, params, compress = M.instance(M.mixed_program() if program == "mixed" else M.memory_program())
    with oracle.hasher(hasher):
        want = oracle.prove_with_traces(mini_blob, traces, params, compress)
        for pattern in ("all", "zeros_to_p"):
            shifted, _ = NC.shift_words(traces, pattern, rng())
            assert oracle.prove_with_traces(mini_blob, shifted, params, compress) == want, pattern


def test_the_oracle_reduces_parameters_and_compress_words(oracle, mini_blob):
    traces, params, compress = M.instance(M.mixed_program(), bitwise_beta=5, program_beta=9)
    assert params == [5, 9]
    want = oracle.prove_with_traces(mini_blob, traces, params, compress)
    params_p, compress_p = NC.shift_parameters(params, compress)
    assert params_p != params and compress_p != compress
    got = oracle.prove_with_traces(mini_blob, traces, params_p, compress_p)
    assert got == want
    assert oracle.verify_all_proof(mini_blob, got, params_p) == (0, "")
    assert oracle.verify_all_proof(mini_blob, got, params) == (0, "")


def test_full_size_instance_reaches_the_paths_the_patterns_are_named_for():
    """tests/make_ref_verdict.instance() under 1 MB pieces: the 2^18-row bitwise table's columns are two pieces each.  `second_half`
    leaves packed first pieces in front of wide second ones, `all` widens both -- strictly between the canonical trace's bytes and
    `all`'s.  (Depends on the instance and the seed only; the GPU module asserts the same figures against upload_stats().)"""
    from tests import make_ref_verdict
    traces = make_ref_verdict.instance()[0]
    assert traces[T.BITWISE].shape[1] == 1 << 18 and traces[T.RANGECHECK].shape[1] == 1 << 16
    figures = {}
    for pattern in (None, "first_half", "second_half", "all", "odd_columns", "single(n/2)", "single(n-1)"):
        shifted = traces if pattern is None else NC.shift_words(traces, pattern, np.random.default_rng(NC.SEED))[0]
        figures[pattern] = NC.link_bytes_model(shifted, piece_mb=1)
    assert figures[None][0] < figures["second_half"][0] < figures["all"][0]
    assert figures[None][0] < figures["first_half"][0] < figures["all"][0]
    canonical_narrow = figures[None][1]
    assert canonical_narrow[T.BITWISE].sum() > 4 and canonical_narrow[T.RANGECHECK].sum() > 4
    assert not figures["all"][1][T.BITWISE].any()                 # every column has a word >= p in both of its pieces
    # narrow and non-narrow columns alternate in the bitwise table's chunks
    odd = figures["odd_columns"][1][T.BITWISE]
    assert not odd[1::2].any() and np.array_equal(odd[0::2], canonical_narrow[T.BITWISE][0::2]) and odd[0::2].any()
    # one word at the seam or at the very end costs its whole piece's packing: as much as a third of the half's words
    for pattern in ("single(n/2)", "single(n-1)"):
        assert figures[None][0] < figures[pattern][0] == figures["second_half"][0] and not figures[pattern][1][T.BITWISE].any()
    # under the default 16 MB pieces the columns are single pieces: every pattern that touches a packed column widens all of it
    assert NC.link_bytes_model(traces)[0] < NC.link_bytes_model(NC.shift_words(traces, "second_half", np.random.default_rng(NC.SEED))[0])[0]
