"""The quotient phase of olavm_amd/csrc/stark.hip -- lagrange_coeffs_kernel and the selectors' extension, the host-built descriptor
(Z_H^-1 per coset in bit-reversed coset order, the alpha powers and their limb forms, the challenge slots), quotient_kernel (the
interpreter) and the twelve generated kernels over airq.cuh, launch_bitrev_rows, ntt_coset_interpolate, the trim_to_len degree check
and the split into chunks -- through ola_quotient at challenges, alphas and parameters the CALLER chooses: every word of every chunk
equals Python integers (tests/quotient_reference.py, pinned to the oracle prover's quotient caps by tests/test_quotient_reference.py)
and is canonical.  No transcript is involved.  Every comparison runs twice, with the generated kernel (air_kernels_available says it
is there) and under OLA_AIR_KERNELS=interpreter.

Valid traces (tests/quotient_cases.py VALID; Z columns of tests/zcolumn_reference.py at the case's challenges), rows per table:
  source    cpu  memory bitwise cmp rangecheck poseidon poseidon_chunk storage_access tape sccall program prog_chunk
  q           6       7       2   2          2        6              2              3    4      1       2          3
  padding2    2       2      64   2         16        2              2              2    2      2       2          2    generators' padding
  hash      128      64      64   2         64        8              8              8    8      8     256          8    an executed program
  hash40                                                            64                                                 (64 live rows)
  tape                                                                                   8                             (live rows)
  fib28     256                                                                                                        exactly AIRQ_THREADS
  rows512   512     512     512 512        512      512            512            512  512    512     512        512
2 rows: one workgroup of n threads per coset; 8 .. 128: the same, 64 and 128 more than the interpreter's one wavefront; 256: exactly
AIRQ_THREADS; 512: two workgroups per coset, the next row wraps round only in the second.  At 512 rows the CPU, memory and program
tables are an executed program's, bitwise, cmp, rangecheck, storage_access and tape come from their generators on made-up operations,
poseidon is 256 golden permutations and 256 zero rows, and poseidon_chunk, sccall and prog_chunk are padding rows (a live 512-row
table of theirs takes an execution of many seconds; sccall has no generator).  The fixed tables, bitwise and rangecheck, have no
fewer than 64 and 16 rows; a storage access has 256 rows, so storage_access below 256 is padding.  No table could not run at 512.
Challenge sets, all eight on every case but the CPU table at 256 and 512 rows and the Poseidon table at 512 (random,
alphas_one_minus_one, non_canonical: the CPU table's 78 lookup columns cost 0.8 s and 1.5 s of integers per set, the Poseidon
table's program 4.4 s once): random; alphas (0, 0), (1, p - 1), (0, 1); lookup and permutation challenges (0, 1), (1, 0),
(p - 1, p - 1) -- a set under which a permutation denominator vanishes has no Z columns and is left out for that table, counted in
the test --; non_canonical: alphas, challenges and parameters all >= p, the chunks those of the reduced words.

Generic values (q a power of two: bitwise, cmp, rangecheck, poseidon_chunk, tape, sccall, program): uniform rows with binary filters
and uniform Z columns, and rows and Z columns of p - 1, 0xFFFFFFFEFFFFFFFF and 0x00000000FFFFFFFF, at 8 and 512 rows under random
challenges; cmp at 2^13 rows, where size_bits = 14 takes the scratch-buffer interpolation and the tiled bit reversal.

The slowest reference case is the 512-row Poseidon table: 4.4 s on one core of the build machine's CPU for its 5177-node program on
4096 points, once, then 0.4 s per challenge set; the 512-row CPU table takes 0.5 s and 1.5 s per set.  The whole module, references
included, takes 25 s on the MI355X machine's host; its slowest case, the 512-row CPU table, 4.0 s."""
import numpy as np
import pytest

from tests import quotient_cases as QC, quotient_reference as QR

pytestmark = pytest.mark.gpu
P = QR.P
OLA_E_INVALID_ARG, OLA_E_QUOTIENT_DEGREE = -1, -4
FORMS = ("generated", "interpreter")


@pytest.fixture(scope="module")
def be():
    from olavm_amd.backend import Backend
    b = Backend(device=0)
    assert all(b.air_kernels_available(QC.airset().blob(), 12)), "a table without its generated kernel: the default form would be the interpreter"
    yield b
    b.close()


def assert_columns_equal(got, want, what):
    want = np.array(want, dtype=np.uint64).reshape(len(want), got.shape[1])
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        cols, rows = np.nonzero(got != want)
        first = [(int(c), int(r), int(got[c, r]), int(want[c, r])) for c, r in list(zip(cols, rows))[:4]]
        raise AssertionError("%s: %d words differ, (chunk, coefficient, got, want): %s" % (what, len(cols), first))
    assert int(got.max(initial=0)) < P, what


def use_form(monkeypatch, form):
    """OLA_AIR_KERNELS is read per call"""
    if form == "interpreter":
        monkeypatch.setenv("OLA_AIR_KERNELS", "interpreter")
    else:
        monkeypatch.delenv("OLA_AIR_KERNELS", raising=False)


def device_chunks(be, monkeypatch, table, trace_batch, zs, cs, params, n, form):
    use_form(monkeypatch, form)
    zb = be.commit(np.array(zs, dtype=np.uint64))
    try:
        pr = [int(v) + (P if cs["raw_params"] else 0) for v in params]
        return be.quotient(QC.airset().blob(), table, trace_batch, zb, cs["perm"], cs["ctl"], cs["alphas"], pr, n)
    finally:
        zb.free()


def both_forms(be, monkeypatch, table, trace_batch, zs, cs, params, n, want, what):
    """-> what went wrong, one line per kernel form: the interpreter runs whatever the generated kernel gave"""
    from olavm_amd.backend import OlaGpuError
    wrong = []
    for form in FORMS:
        try:
            assert_columns_equal(device_chunks(be, monkeypatch, table, trace_batch, zs, cs, params, n, form), want, what + ", " + form)
        except (AssertionError, OlaGpuError) as e:
            wrong.append(str(e) if form in str(e) else "%s, %s: %s" % (what, form, e))
    return wrong


@pytest.fixture(scope="module")
def references(oracle):
    """(source, table name) -> quotient_reference.Quotient of the valid trace: its points, selectors and program values serve all
    challenge sets and both kernel forms"""
    cache = {}

    def get(source, name):
        if (source, name) not in cache:
            cache[source, name] = QR.Quotient(oracle, QC.airset(), QC.NAMES.index(name), QC.valid(source)[name], QC.table_params(name))
        return cache[source, name]
    return get


@pytest.mark.parametrize("source,name,sets", QC.VALID, ids=lambda x: x if isinstance(x, str) else ("all" if x is None else "three"))
def test_valid_traces_at_caller_chosen_challenges(be, monkeypatch, references, source, name, sets):
    s, t = QC.airset(), QC.NAMES.index(name)
    tab, trace = s.tables[t], QC.valid(source)[name]
    n, ref = trace.shape[1], references(source, name)
    tb = be.commit(trace)
    no_z, wrong = [], []
    for k, set_name in enumerate(sets or QC.SETS):
        cs = QC.challenge_set(set_name, tab, 100 * t + k)
        what = "%s of %s, %d rows, %s" % (name, source, n, set_name)
        try:
            zs = QR.z_columns(s, t, trace, cs["perm"], cs["ctl"])
        except ZeroDivisionError:
            assert tab.permutation_pairs and set_name in QC.GRAND_PRODUCT, what
            no_z.append(set_name)
            continue
        want = ref.chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
        assert len(want) == 2 * tab.quotient_degree_factor
        if set_name == "non_canonical":
            words = [w for pair in cs["ctl"] + [p for ps in cs["perm"] or [] for p in ps] for w in pair] + cs["alphas"]
            assert min(words) >= P
            red = QC.reduced(cs)
            assert want == ref.chunks(QR.z_columns(s, t, trace, red["perm"], red["ctl"]), red["perm"], red["ctl"], red["alphas"])
        wrong += both_forms(be, monkeypatch, t, tb, zs, cs, QC.table_params(name), n, want, what)
    tb.free()
    assert not wrong, "%d comparisons failed:\n" % len(wrong) + "\n".join(wrong)
    assert len(no_z) <= 2, no_z                     # (0, 1) with cells of p - 1, (1, 0) with cells of 0: never all three


@pytest.mark.parametrize("values", ["random", "edge"])
@pytest.mark.parametrize("log_n", [3, 9])
@pytest.mark.parametrize("name", QC.POWER_OF_TWO_Q)
def test_generic_values_in_every_operation(be, monkeypatch, oracle, name, log_n, values):
    generic(be, monkeypatch, oracle, name, log_n, values)


def test_scratch_buffer_interpolation_at_two_to_the_13_rows(be, monkeypatch, oracle):
    """cmp, q = 2: size_bits = 14"""
    generic(be, monkeypatch, oracle, "cmp", 13, "random")


def generic(be, monkeypatch, oracle, name, log_n, values):
    s, t, n = QC.airset(), QC.NAMES.index(name), 1 << log_n
    tab = s.tables[t]
    assert tab.quotient_degree_factor in (1, 2, 4)
    trace = QC.generic_trace(t, n, values, log_n)
    zs = QC.generic_zs(tab.num_permutation_batches() + s.num_ctl_zs(t), n, values, 50 * t + log_n)
    cs = QC.challenge_set("random", tab, 300 + 10 * t + log_n)
    params = [int(x) for x in np.random.default_rng(t).integers(0, P, size=tab.n_params, dtype=np.uint64)]
    want = QR.compute_quotient_polys(oracle, s, t, trace, zs, cs["perm"], cs["ctl"], cs["alphas"], params)
    tb = be.commit(trace)
    wrong = both_forms(be, monkeypatch, t, tb, zs, cs, params, n, want, "%s, 2^%d rows of %s values" % (name, log_n, values))
    tb.free()
    assert not wrong, "\n".join(wrong)
    assert any(any(c) for c in want)


# ---- refusals, each followed by a correct quotient from the same context -----------------------------------------------------------
def after_a_refusal(be, monkeypatch, references, form):
    """cmp of the executed program, random challenges"""
    s, t = QC.airset(), QC.NAMES.index("cmp")
    trace = QC.valid("hash")["cmp"]
    cs = QC.challenge_set("random", s.tables[t], 9)
    zs = QR.z_columns(s, t, trace, cs["perm"], cs["ctl"])
    tb = be.commit(trace)
    got = device_chunks(be, monkeypatch, t, tb, zs, cs, [], trace.shape[1], form)
    tb.free()
    assert_columns_equal(got, references("hash", "cmp").chunks(zs, cs["perm"], cs["ctl"], cs["alphas"]), "after a refusal, " + form)


def refused_for_its_degree(be, monkeypatch, references, oracle, name, trace, zs, cs, params):
    from olavm_amd.backend import OlaGpuError
    s, t = QC.airset(), QC.NAMES.index(name)
    with pytest.raises(QR.QuotientDegreeError, match=QR.DEGREE_MESSAGE):
        QR.compute_quotient_polys(oracle, s, t, trace, zs, cs["perm"], cs["ctl"], cs["alphas"], params)
    tb = be.commit(trace)
    for form in FORMS:
        with pytest.raises(OlaGpuError, match=QR.DEGREE_MESSAGE) as e:
            device_chunks(be, monkeypatch, t, tb, zs, cs, params, trace.shape[1], form)
        assert e.value.code == OLA_E_QUOTIENT_DEGREE, (name, form)
        after_a_refusal(be, monkeypatch, references, form)
    tb.free()


@pytest.mark.parametrize("name", [n for n in QC.NAMES if n not in QC.POWER_OF_TWO_Q])
def test_random_rows_fail_the_degree_check_where_there_is_one(be, monkeypatch, references, oracle, name):
    """q = 3, 6, 7: keep < size"""
    s, t = QC.airset(), QC.NAMES.index(name)
    tab = s.tables[t]
    assert tab.quotient_degree_factor in (3, 6, 7) and not tab.permutation_pairs
    trace = QC.generic_trace(t, 8, "random", 1)
    zs = QC.generic_zs(s.num_ctl_zs(t), 8, "random", t)
    refused_for_its_degree(be, monkeypatch, references, oracle, name, trace, zs, QC.challenge_set("random", tab, 400 + t), [])


@pytest.mark.parametrize("name,source,column", [("cpu", "hash", 12), ("memory", "rows512", 2), ("poseidon", "hash", 9)])
@pytest.mark.parametrize("row", ["0", "n-1"])
def test_one_changed_cell_fails_the_degree_check(be, monkeypatch, references, oracle, name, source, column, row):
    s, t = QC.airset(), QC.NAMES.index(name)
    bad = QC.valid(source)[name].copy()
    r = 0 if row == "0" else bad.shape[1] - 1
    bad[column, r] = (int(bad[column, r]) + 1) % P
    cs = QC.challenge_set("random", s.tables[t], 500 + t)
    refused_for_its_degree(be, monkeypatch, references, oracle, name, bad, QR.z_columns(s, t, bad, cs["perm"], cs["ctl"]), cs, [])


def test_a_z_commitment_of_another_shape_and_missing_challenges_are_refused(be, monkeypatch, references):
    from olavm_amd.backend import OlaGpuError
    s, t = QC.airset(), QC.NAMES.index("rangecheck")
    tab, trace = s.tables[t], QC.valid("hash")["rangecheck"]
    n = trace.shape[1]
    cs = QC.challenge_set("random", tab, 600)
    zs = np.array(QR.z_columns(s, t, trace, cs["perm"], cs["ctl"]), dtype=np.uint64)
    want = references("hash", "rangecheck").chunks(zs, cs["perm"], cs["ctl"], cs["alphas"])
    tb = be.commit(trace)
    for form in FORMS:
        for wrong in (zs[:-1], np.concatenate([zs, zs[:1]]), zs[:, :n // 2], np.concatenate([zs, zs], axis=1)):
            with pytest.raises(OlaGpuError, match="Z commitment does not match the table") as e:
                device_chunks(be, monkeypatch, t, tb, wrong, cs, [], n, form)
            assert e.value.code == OLA_E_INVALID_ARG
            assert_columns_equal(device_chunks(be, monkeypatch, t, tb, zs, cs, [], n, form), want, "after a refused Z commitment, " + form)
        assert tab.permutation_pairs
        with pytest.raises(OlaGpuError, match="perm_challenges required") as e:
            device_chunks(be, monkeypatch, t, tb, zs, dict(cs, perm=None), [], n, form)
        assert e.value.code == OLA_E_INVALID_ARG
        assert_columns_equal(device_chunks(be, monkeypatch, t, tb, zs, cs, [], n, form), want, "after missing challenges, " + form)
    tb.free()
