"""ola_generate_tape_trace / ola_generate_poseidon_chunk_trace / ola_generate_prog_chunk_trace (include/ola_gpu.h): the three narrow
tables the host still assembled, word for word against miniexec.tape_trace, poseidon_chunk_trace and prog_chunk_and_poseidon -- on the
nine executed examples and on hand-made inputs at the sizes where the code changes path: no record at all, one, the padding boundary,
more than one workgroup and more than one scan block, equal tape addresses whose order only a stable sort keeps, words >= p, host and
device memory on either side, the refusals of the validation pass, each followed by a correct table from the same context, and a proof that
takes the three generated tables as resident tables."""
import numpy as np
import pytest

from olavm_amd.air import miniexec as M, ola_tables as T, tracegen as TG
from olavm_amd.air.dsl import P
from tests.test_gpu_tablegen import dev_table, to_dev, to_host

pytestmark = pytest.mark.gpu

OLA_E_INVALID_ARG = -1


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    yield b
    b.close()


def log2(n):
    return int(n).bit_length() - 1


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for c in range(want.shape[0]):
        assert np.array_equal(got[c], want[c]), "column %d" % c


# ---- inputs in the generators' formats from miniexec's side lists
def tape_cells(side_tape):
    """(address, index, op, value) in execution order -> 3 x n words"""
    return np.array([[c[0] for c in side_tape], [T.op_mask(c[2]) for c in side_tape], [c[3] for c in side_tape]], dtype=np.uint64).reshape(3, -1)


def call_records(calls, first_row):
    """miniexec's POSEIDON calls -> 5 x n words; the blocks of call c sit at Poseidon-table rows first_row + (blocks before c) ..."""
    rec, row = [], first_row
    for c in calls:
        rec.append((c["clk"], c["src"], c["len"], c["dst"], row))
        row += len(c["chunks"])
    return np.array(rec, dtype=np.uint64).reshape(-1, 5).T.copy()


def hashed_calls(rng, lens):
    """POSEIDON calls over random words, built as miniexec.execute builds them (the capacity chained through a call's blocks)"""
    calls = []
    for i, blocks in enumerate(lens):
        src, chunks, cap = 1000 * (i + 1), [], [0, 0, 0, 0]
        for k in range(blocks):
            vals = [int(x) for x in rng.integers(0, P, 8, dtype=np.uint64)]
            row = M.poseidon_row(vals + cap, filters=(1, 0, 0, 0))
            chunks.append((src + 8 * k, vals, cap, row))
            cap = row[16:28][8:12]
        calls.append({"clk": 7 + 3 * i, "src": src, "len": 8 * blocks, "dst": 50000 + 4 * i, "chunks": chunks})
    return calls


def poseidon_table_of(rows, first_row=0):
    """a Poseidon table holding `rows` from row first_row on (ZERO-hash rows elsewhere)"""
    pt = TG.poseidon_padding_trace(TG.next_pow2(max(first_row + len(rows), 8)))
    for i, r in enumerate(rows):
        pt[:, first_row + i] = np.array(r, dtype=np.uint64)
    return pt


class Prog:
    code_addr = (11, 22, 33, 44)


@pytest.fixture(scope="module")
def executed():
    """name -> (miniexec's tape, Poseidon-chunk, program-chunk and Poseidon tables, tape cells, call records, padded listing, code
    address, result line).  The tables are built as miniexec.instance builds them, without the tables this file does not look at; the
    Poseidon table's storage rows, which lie behind the rows used here, are left out with them."""
    out = {}
    for name, (make, kw) in M.EXAMPLES.items():
        prog = make()
        result_line = bool(kw.get("prove_program_hash"))
        listing = prog.words()[0]
        listing = listing + [0] * (-len(listing) % 8)
        tree = M.StorageTree()
        if result_line:
            tree.set(prog.code_addr, M.program_hash(listing))
        side = M.execute(prog, tree=tree)[1]
        pchunk, builtin_rows = M.poseidon_chunk_trace(side["psdn"])
        chunk, psdn = M.prog_chunk_and_poseidon(prog, listing, extra_rows=builtin_rows, result_line=result_line)
        out[name] = (M.tape_trace(side["tape"]), pchunk, chunk, psdn, tape_cells(side["tape"]), call_records(side["psdn"], len(listing) // 8),
                     np.array(listing, dtype=np.uint64), np.array(prog.code_addr, dtype=np.uint64), result_line)
    return out


@pytest.mark.parametrize("name", sorted(M.EXAMPLES))
def test_executed_examples_word_for_word(be, executed, name):
    tape, pchunk, chunk, psdn, cells, calls, listing, code_addr, result_line = executed[name]
    same(be.generate_tape_trace(cells), tape)
    same(be.generate_poseidon_chunk_trace(calls, psdn), pchunk)
    same(be.generate_prog_chunk_trace(listing, code_addr, psdn, result_line=result_line), chunk)
    if name == "tape":
        assert cells.shape[1] > 0
    if name == "hash":
        assert calls.shape[1] > 0


# ---- the tape table
def random_tape(rng, n):
    """n cells over about n / 3 addresses: a TSTORE of each address first, then TLOADs of the same value -- but with values and ops that
    differ at equal addresses wherever the rule allows, so that a sort that is not stable shows"""
    addrs = rng.integers(0, max(n // 3, 1), n)
    return [(int(a), i, "TSTORE" if i % 5 == 0 else "TLOAD", int(rng.integers(0, P, dtype=np.uint64))) for i, a in enumerate(addrs)]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, (1 << 12) + 3])
def test_tape_sizes(be, n):
    rng = np.random.default_rng(100 + n)
    cells = random_tape(rng, n)
    want = M.tape_trace(cells)
    got = be.generate_tape_trace(tape_cells(cells))
    same(got, want)
    assert got.shape == (6, TG.next_pow2(max(n, 8)))
    if n == 0:
        same(be.generate_tape_trace(None), TG.tape_padding_trace(8))
        same(got, TG.tape_padding_trace(8))


def test_tape_one_address_written_once_and_read_many_times(be):
    # 300 cells of one address (and a few of a second one in between): execution order is the only order there is
    cells = [(5, i, "TSTORE" if i == 0 else "TLOAD", 1000 + i) for i in range(300)]
    for i in (17, 130, 299):
        cells[i] = (2, i, "TLOAD", 77 + i)
    want = M.tape_trace(cells)
    got = be.generate_tape_trace(tape_cells(cells))
    same(got, want)
    assert [int(x) for x in got[T.COL_TAPE_VALUE, :3]] == [94, 207, 376] and int(got[T.COL_TAPE_VALUE, 3]) == 1000
    assert [int(x) for x in got[T.COL_TAPE_VALUE, 3:300]] == [1000 + i for i in range(300) if i not in (17, 130, 299)]
    # every address 0: no bit to sort by, the cells stay as they came
    zero = [(0, i, "TLOAD", 9 + i) for i in range(11)]
    same(be.generate_tape_trace(tape_cells(zero)), M.tape_trace(zero))


def test_tape_words_not_below_p(be):
    rng = np.random.default_rng(5)
    cells = random_tape(rng, 600)
    words = tape_cells(cells)
    lifted = words.copy()
    room = lifted < np.uint64((1 << 64) - P)
    lifted = np.where(room, lifted + np.uint64(P), lifted)
    assert (lifted[0] >= np.uint64(P)).all() and (lifted[1] >= np.uint64(P)).all()
    same(be.generate_tape_trace(lifted), M.tape_trace(cells))
    # an address that is p + 3 sorts as 3, behind 2 and before 4
    mixed = np.array([[4, P + 3, 2], [T.op_mask("TSTORE")] * 3, [40, 30, 20]], dtype=np.uint64)
    got = be.generate_tape_trace(mixed)
    assert [int(x) for x in got[T.COL_TAPE_ADDR, :4]] == [2, 3, 4, 4] and [int(x) for x in got[T.COL_TAPE_VALUE, :4]] == [20, 30, 40, 40]


@pytest.mark.parametrize("dev_in,dev_out", [(False, False), (False, True), (True, False), (True, True)])
def test_host_and_device_memory(be, dev_in, dev_out):
    rng = np.random.default_rng(9)
    cells = random_tape(rng, 700)
    calls = hashed_calls(rng, [2, 1, 3])
    listing = [int(x) for x in rng.integers(0, P, 24, dtype=np.uint64)]
    chunk, psdn = M.prog_chunk_and_poseidon(Prog, listing, extra_rows=[ch[3] for c in calls for ch in c["chunks"]], result_line=True)
    want = [M.tape_trace(cells), M.poseidon_chunk_trace(calls)[0], chunk]
    ins = [tape_cells(cells), call_records(calls, 3), np.array(listing, dtype=np.uint64), np.array(Prog.code_addr, dtype=np.uint64), psdn]
    if dev_in:
        ins = [to_dev(a) for a in ins]
    outs = [dev_table(w.shape[0], log2(w.shape[1])) if dev_out else None for w in want]
    got = [be.generate_tape_trace(ins[0], out=outs[0]),
           be.generate_poseidon_chunk_trace(ins[1], ins[4], out=outs[1]),
           be.generate_prog_chunk_trace(ins[2], ins[3], ins[4], result_line=True, out=outs[2])]
    for g, o, w in zip(got, outs, want):
        if dev_out:
            assert g == log2(w.shape[1])
            g = to_host(o)
        same(g, w)


# ---- the Poseidon-chunk table
@pytest.mark.parametrize("lens", [[], [1], [1, 2, 5], [5, 1, 1, 2], [1] * 100 + [3] * 25], ids=["none", "one_block", "mixed", "mixed2", "300_rows"])
def test_poseidon_chunk_shapes(be, lens):
    rng = np.random.default_rng(len(lens))
    calls = hashed_calls(rng, lens)
    want, prow = M.poseidon_chunk_trace(calls)
    first = 5                                        # the calls' blocks do not start at row 0 of the Poseidon table
    got = be.generate_poseidon_chunk_trace(call_records(calls, first), poseidon_table_of(prow, first))
    same(got, want)
    rows = sum(1 + l for l in lens)
    assert got.shape == (53, TG.next_pow2(max(rows, 8))) and int((got[T.COL_POSEIDON_CHUNK_IS_PADDING_LINE] == 0).sum()) == rows
    if not lens:
        same(be.generate_poseidon_chunk_trace(None, poseidon_table_of([])), want)


def test_poseidon_chunk_words_not_below_p(be):
    rng = np.random.default_rng(3)
    calls = hashed_calls(rng, [2, 1])
    want, prow = M.poseidon_chunk_trace(calls)
    rec, psdn = call_records(calls, 0), poseidon_table_of(prow)
    room = psdn < np.uint64((1 << 64) - P)
    same(be.generate_poseidon_chunk_trace(rec + np.uint64(P), np.where(room, psdn + np.uint64(P), psdn)), want)


def test_poseidon_chunk_refusals_leave_the_context_working(be):
    from olavm_amd.backend import OlaGpuError
    rng = np.random.default_rng(4)
    calls = hashed_calls(rng, [1, 2])
    want, prow = M.poseidon_chunk_trace(calls)
    rec, psdn = call_records(calls, 0), poseidon_table_of(prow)             # 8 rows, 3 of them live
    bad = []
    for word, value in ((2, 0), (2, 12), (2, P + 12), (4, 7), (4, 8), (4, P + 7)):      # len 0, len 12, a psdn_row that runs off the table
        r = rec.copy()
        r[word, 1] = value
        bad.append(r)
    for i, r in enumerate(bad):
        out = np.full((53, 8), 7, dtype=np.uint64)
        with pytest.raises(OlaGpuError) as e:
            be.generate_poseidon_chunk_trace(r, psdn, out=out)
        assert e.value.code == OLA_E_INVALID_ARG and (out == 7).all(), i
        same(be.generate_poseidon_chunk_trace(rec, psdn), want)
    # the last row of the table is still inside it
    edge = rec.copy()
    edge[4, 0] = 7
    got = be.generate_poseidon_chunk_trace(edge, psdn)
    assert [int(x) for x in got[T.COL_POSEIDON_CHUNK_HASH_RANGE.start:T.COL_POSEIDON_CHUNK_HASH_RANGE.stop, 1]] == [int(x) for x in psdn[16:28, 7]]


# ---- the program-chunk table
@pytest.mark.parametrize("result_line", [False, True])
@pytest.mark.parametrize("n_words", [8, 16, 8 * 257])
def test_prog_chunk_sizes(be, n_words, result_line):
    rng = np.random.default_rng(n_words)
    listing = [int(x) for x in rng.integers(0, P, n_words, dtype=np.uint64)]
    want, psdn = M.prog_chunk_and_poseidon(Prog, listing, result_line=result_line)
    got = be.generate_prog_chunk_trace(np.array(listing, dtype=np.uint64), Prog.code_addr, psdn, result_line=result_line)
    same(got, want)
    assert got.shape == (40, TG.next_pow2(max(n_words // 8, 8))) and int(got[T.COL_PROG_CHUNK_IS_RESULT_LINE].sum()) == int(result_line)
    if n_words == 16:                                # words >= p, and a Poseidon table higher than the listing needs
        tall = poseidon_table_of([psdn[:, i] for i in range(2)] + [psdn[:, 0]] * 20)
        lifted = np.array(listing, dtype=np.uint64)
        lifted = np.where(lifted < np.uint64((1 << 64) - P), lifted + np.uint64(P), lifted)
        same(be.generate_prog_chunk_trace(lifted, np.array(Prog.code_addr, dtype=np.uint64) + np.uint64(P), tall, result_line=result_line), want)


def test_prog_chunk_refusals_leave_the_context_working(be):
    from olavm_amd.backend import OlaGpuError
    listing = list(range(1, 17))
    want, psdn = M.prog_chunk_and_poseidon(Prog, listing)
    out = np.full((40, 8), 7, dtype=np.uint64)
    for words, table in ((listing[:12], psdn), (list(range(8 * 9)), psdn)):      # no whole chunks; more chunks than the table has rows
        with pytest.raises(OlaGpuError) as e:
            be.generate_prog_chunk_trace(np.array(words, dtype=np.uint64), Prog.code_addr, table, out=out)
        assert e.value.code == OLA_E_INVALID_ARG and (out == 7).all()
        same(be.generate_prog_chunk_trace(np.array(listing, dtype=np.uint64), Prog.code_addr, psdn), want)


# ---- the generated tables as resident tables of a proof
@pytest.mark.parametrize("name", ["tape", "hash"])
def test_generated_tables_prove_as_resident_tables(be, name):
    """the three tables generated into device memory, from a device-resident Poseidon table, go into prove_with_traces in place of the
    host's and give its bytes"""
    make, kw = M.EXAMPLES[name]
    prog = make()
    blob = T.ola_stark(range_bits=4, limb_bits=2).blob()
    traces, params, compress = M.instance(prog, **kw)
    want = bytes(be.prove_with_traces(blob, traces, params, compress))
    listing = prog.words()[0]
    listing = listing + [0] * (-len(listing) % 8)
    side = M.execute(prog)[1]
    psdn = to_dev(traces[T.POSEIDON])
    outs = {t: dev_table(traces[t].shape[0], log2(traces[t].shape[1])) for t in (T.TAPE, T.POSEIDON_CHUNK, T.PROG_CHUNK)}
    be.generate_tape_trace(tape_cells(side["tape"]), out=outs[T.TAPE])
    be.generate_poseidon_chunk_trace(call_records(side["psdn"], len(listing) // 8), psdn, out=outs[T.POSEIDON_CHUNK])
    be.generate_prog_chunk_trace(np.array(listing, dtype=np.uint64), prog.code_addr, psdn, out=outs[T.PROG_CHUNK])
    resident = list(traces)
    for t, table in outs.items():
        same(to_host(table), traces[t])
        resident[t] = table
    assert bytes(be.prove_with_traces(blob, resident, params, compress)) == want
