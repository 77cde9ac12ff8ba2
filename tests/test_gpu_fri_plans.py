"""FRI reduction plans with an arity per layer (FriReductionStrategy::Fixed and MinSize, ola_gpu_set_fri_reduction) on the device.

1. The kernels at challenges the CALLER chooses, through ola_open .. ola_fri_commit_finish under Fixed plans: every word of the final
   polynomial and every layer's cap against Python integers (tests/opening_reference.py's composed quotients, folded layer by layer with
   the plan's arities; the caps from the oracle's transform and tree, or tests/keccak_ref.py's tree, with leaves of 2 * arity words:
   tests/fri_plan_reference.py).  Shapes, the smallest at which a path exists (N = 8 n values in the first layer):
     2^12 rows  the first layer is exactly 4096 non-zero coefficients: the smallest input of fold_pairs_kernel<2 | 3 | 4> (arity 2 folds in fold_kernel), and
                4096 / 8192 / 16384 leaves for arity 8 / 4 / 2 (the staged leaf kernels need 1024); plans [3,3] [2,2,2] [1,1,1,1]
                [3,4] [4,3] [1,4,2,3] and [] (no layer: the final polynomial is the composed quotient)
     2^11 rows  [3,3]: below the threshold, fold_kernel folds every arity
     2^16 rows  [4,3,3]: fold_pairs_kernel<4> on 65536, fold_pairs_kernel<3> on exactly 4096, fold_kernel on 512; staged leaves on the first
                two layers -- also in a child process under OLA_POOL_POISON=1, where a word behind nz_out that nobody wrote is 0xFF..FF
   Challenge sets: random, beta = 1, beta = 0, beta = (p-1, p-1), and words >= p whose results must equal the run with the reduced
   words.  Columns: the stress columns of tests/opening_cases.py (all p - 1, random, ...).  Hashers: Poseidon, Blake3 and Keccak at 2^12;
   OLA_LEAF_EXT_STAGED=0 and OLA_FOLD16=0 in a child process each give the default path's words.
2. Pinned to the oracle, which folds with constant arities: ola_open_and_prove under fri_arity_bits 1, 2, 3 equals its bytes, and
   Fixed with the list ConstantArityBits would give returns the default context's bytes.
3. Whole proofs: the committed MinSize proof of tests/make_ref_verdict_minsize.py is what ola_prove_with_traces returns, the verifier
   gives the reference's recorded verdicts on it and its nineteen corruptions, each strategy refuses the other's proof with a shape
   reason; the miniature programs under MinSize(None), MinSize(Some(3)) and Fixed; the stepped ABI under MinSize; multi-rank refusal."""
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from olavm_amd.air import miniexec as M, ola_tables as T
from tests import fri_plan_child as child, fri_plan_reference as FP, opening_cases as OC, opening_reference as R, tracegen

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "ref_verified")
P = R.P
OLA_E_INVALID_ARG = -1
CHILD_TIMEOUT = 120
FATAL_STATUS = (-6, -11, 134, 139, 124, 137)
MINI = dict(range_bits=4, limb_bits=2)

SETS = ("random", "base_zeta", "x_zeta", "minus_ones", "non_canonical")       # beta: random, 1, 0, (p-1, p-1), words >= p
PLANS_12 = ([3, 3], [2, 2, 2], [1, 1, 1, 1], [3, 4], [4, 3], [1, 4, 2, 3], [])
KERNEL_CASES = ([("poseidon", 12, plan, s) for plan in PLANS_12 for s in SETS] +
                [(h, 12, plan, s) for h in ("blake3", "keccak") for plan in PLANS_12 for s in ("random", "minus_ones")] +
                [("poseidon", 11, [3, 3], s) for s in SETS] +
                [("blake3", 16, [4, 3, 3], s) for s in SETS] + [("poseidon", 16, [4, 3, 3], "random")])


def plan_id(plan):
    return "-".join(map(str, plan)) or "none"


# ------------------------------------------------------------------------------------------------ the reference, computed once
_composed = {}


def composed(log_n, name):
    """the composed quotients of the stress columns at the set's zeta and alpha (the plan does not enter)"""
    if (log_n, name) not in _composed:
        coeffs = [c.tolist() for c in OC.stress_batches(log_n, OC.MAIN_COLS)]
        zeta, alpha, _ = {s[0]: s[1:] for s in OC.challenge_sets(log_n, 0)}[name]
        _composed[(log_n, name)] = R.composed_quotients(*coeffs, OC.MAIN_NPERM, zeta, alpha)[0]
    return _composed[(log_n, name)]


def reference_layers(log_n, name, plan):
    beta = {s[0]: s[3] for s in OC.challenge_sets(log_n, 1)}[name][0]
    out = [(composed(log_n, name), (1 << log_n) << 3)]
    for ab in plan:
        out.append(R.fold(out[-1][0], out[-1][1], R.ext(beta), 1 << ab))
    return out


def reference_caps(oracle, hasher, layers, plan):
    if hasher == "keccak":
        from tests import keccak_ref
        return FP.layer_caps(oracle, layers, plan, merkle=lambda leaves, h: keccak_ref.MerkleTree(leaves, h).cap())
    with oracle.hasher(hasher):
        return FP.layer_caps(oracle, layers, plan)


def assert_equals_reference(oracle, hasher, log_n, name, plan, final, caps):
    layers = reference_layers(log_n, name, plan)
    want = FP.final_poly(layers)
    assert len(final) == len(want) == 1 << (log_n - sum(plan))
    wrong = [(k, g, w) for k, (g, w) in enumerate(zip(final, want)) if tuple(g) != tuple(w)]
    assert not wrong, "final polynomial, %d words differ, (index, got, want): %s" % (len(wrong), wrong[:4])
    want_caps = reference_caps(oracle, hasher, layers, plan)
    assert len(caps) == len(want_caps) == len(plan)
    wrong = [i for i, (g, w) in enumerate(zip(caps, want_caps)) if not np.array_equal(np.asarray(g, dtype=np.uint64), w)]
    assert not wrong, "the caps of the layers %s differ (plan %s)" % (wrong, plan)


# ------------------------------------------------------------------------------------------------ 1. kernels at caller-chosen betas
@pytest.fixture(scope="module")
def committed(oracle):
    """the stress batches of one (hasher, log_n) on the device at a time"""
    from olavm_amd.backend import Backend
    live = {}

    def drop():
        for be, batches in live.values():
            for b in batches:
                b.free()
            be.close()
        live.clear()

    def get(hasher, log_n):
        if (hasher, log_n) not in live:
            drop()
            be = Backend(device=0, hasher=hasher)
            live[(hasher, log_n)] = (be, child.commit_stress(be, oracle, log_n)[0])
        return live[(hasher, log_n)]
    yield get
    drop()


@pytest.mark.parametrize("hasher,log_n,plan,name", [pytest.param(*c, id="%s-2p%d-%s-%s" % (c[0], c[1], plan_id(c[2]), c[3])) for c in KERNEL_CASES])
def test_final_polynomial_and_layer_caps_equal_the_integer_reference(committed, oracle, hasher, log_n, plan, name):
    be, batches = committed(hasher, log_n)
    zeta, alpha, betas = {s[0]: s[1:] for s in OC.challenge_sets(log_n, len(plan))}[name]
    final, caps = child.run_steps(be, batches, OC.MAIN_NPERM, plan, zeta, alpha, betas)
    assert_equals_reference(oracle, hasher, log_n, name, plan, final, caps)
    if name == "non_canonical":             # every returned word equals the run with the reduced words
        final_r, caps_r = child.run_steps(be, batches, OC.MAIN_NPERM, plan, R.ext(zeta), R.ext(alpha), [R.ext(b) for b in betas])
        assert final == final_r and all(np.array_equal(a, b) for a, b in zip(caps, caps_r))


def run_child(log_n, hasher, plan, names, env, tmp_path):
    out = tmp_path / "out.json"
    e = dict(os.environ)
    e.update(env)
    t0 = time.perf_counter()
    args = [sys.executable, "-m", "tests.fri_plan_child", str(log_n), hasher, ",".join(map(str, plan)) or "-", ",".join(names), str(out)]
    try:
        r = subprocess.run(args, cwd=ROOT, env=e, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as x:
        pytest.exit("child %s %s did not finish in %d s; nothing more is started on the GPU\n%s" % (args[3:7], env, CHILD_TIMEOUT, x.stderr), returncode=3)
    if r.returncode in FATAL_STATUS:
        pytest.exit("child %s %s ended with status %d; nothing more is started on the GPU\n%s" % (args[3:7], env, r.returncode, r.stderr[-4000:]), returncode=3)
    assert r.returncode == 0, "child %s %s: status %d\n%s" % (args[3:7], env, r.returncode, r.stderr[-4000:])
    print("child %s %s: %.1f s" % (args[3:7], env, time.perf_counter() - t0))
    return json.loads(out.read_text())


def test_unwritten_words_behind_the_folds_outputs_show_under_a_poisoned_pool(oracle, tmp_path):
    """2^16 rows, [4,3,3] under OLA_POOL_POISON=1: every block of the pool starts as all-ones words, so a fold that leaves the zero tail
    behind its nz_out outputs to a memset that is missing changes the next layer's cap.  (Checked once by hand: with the two memsets of
    fri_fold skipped for arities 2, 4 and 8 this test fails at the cap of layer 2, the layer committed after fold_pairs_kernel<3>, while
    the same shape in this process, on blocks the driver handed out zeroed, still passes; with the memsets it passes.)"""
    names = ("random", "x_zeta")
    got = run_child(16, "blake3", [4, 3, 3], names, {"OLA_POOL_POISON": "1"}, tmp_path)
    for name in names:
        assert_equals_reference(oracle, "blake3", 16, name, [4, 3, 3], [tuple(x) for x in got[name]["final"]], got[name]["caps"])


@pytest.mark.parametrize("switch", ["OLA_LEAF_EXT_STAGED", "OLA_FOLD16"])
def test_switches_select_the_plain_kernels_for_every_arity(committed, oracle, switch, tmp_path):
    """=0 goes on meaning "the plain kernels": the words are those of the default path (and of the reference)"""
    names = ("random", "minus_ones")
    got = run_child(12, "blake3", [3, 3], names, {switch: "0"}, tmp_path)
    be, batches = committed("blake3", 12)
    for name in names:
        zeta, alpha, betas = {s[0]: s[1:] for s in OC.challenge_sets(12, 2)}[name]
        final, caps = child.run_steps(be, batches, OC.MAIN_NPERM, [3, 3], zeta, alpha, betas)
        assert [tuple(x) for x in got[name]["final"]] == final
        assert all(np.array_equal(np.asarray(a, dtype=np.uint64), b) for a, b in zip(got[name]["caps"], caps)) and len(got[name]["caps"]) == len(caps) == 2
        assert_equals_reference(oracle, "blake3", 12, name, [3, 3], final, caps)


# ------------------------------------------------------------------------------------------------ 2. pinned to the oracle
def rand_field(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("log_n", [12, 15])
@pytest.mark.parametrize("arity_bits", [1, 2, 3])
def test_constant_arities_2_4_8_give_the_oracles_bytes(oracle, hasher, log_n, arity_bits):
    """the kernels are chosen by a layer's arity, so constant configurations run them too: ConstantArityBits(1 | 2 | 3, 5)"""
    from olavm_amd.backend import Backend, Challenger
    cols, nperm = (3, 2, 2), 1
    rng = np.random.default_rng(4000 + log_n)
    n = 1 << log_n
    tv, zv, qc = rand_field(rng, (cols[0], n)), rand_field(rng, (cols[1], n)), rand_field(rng, (cols[2], n))
    be = Backend(device=0, hasher=hasher, fri_arity_bits=arity_bits, fri_final_poly_bits=5)
    cfg = (3, 4, 16, arity_bits, 5, 28)
    try:
        gt, gz, gq = be.commit(tv), be.commit(zv), be.commit(qc, from_coeffs=True)
        ch = Challenger(hasher=hasher)
        with oracle.hasher(hasher):
            ot, oz, oq = oracle.batch(tv), oracle.batch(zv), oracle.batch(qc, from_coeffs=True)
            och = oracle.challenger()
            for b, ob in ((gt, ot), (gz, oz), (gq, oq)):
                ch.observe_cap(b.cap())
                och.observe_cap(ob.cap())
            same = ch.clone()
            g_open, g_fri = be.open_and_prove(gt, gz, gq, nperm, ch)
            _, o_open, o_fri = oracle.open_and_prove(ot, oz, oq, nperm, och, cfg)
            assert oracle.fri_arity_bits(log_n, cfg) == FP.arity_bits(("constant_arity_bits",), log_n, fri_arity_bits=arity_bits)
        assert g_open == o_open, "opening set bytes differ"
        assert g_fri == o_fri, "FRI proof bytes differ"
        # Fixed with exactly that list: the same bytes, and the same transcript afterwards
        be.set_fri_reduction(("fixed", FP.arity_bits(("constant_arity_bits",), log_n, fri_arity_bits=arity_bits)))
        f_open, f_fri = be.open_and_prove(gt, gz, gq, nperm, same)
        assert (f_open, f_fri) == (g_open, g_fri) and same.get() == ch.get()
    finally:
        be.close()


def test_fixed_with_the_default_plan_gives_the_default_bytes():
    from olavm_amd.backend import Backend, Challenger
    log_n, cols, nperm = 13, (5, 3, 2), 1
    rng = np.random.default_rng(77)
    n = 1 << log_n
    be = Backend(device=0)
    try:
        gt, gz, gq = be.commit(rand_field(rng, (cols[0], n))), be.commit(rand_field(rng, (cols[1], n))), be.commit(rand_field(rng, (cols[2], n)), from_coeffs=True)
        ch = Challenger()
        for b in (gt, gz, gq):
            ch.observe_cap(b.cap())
        a, b = ch.clone(), ch.clone()
        want = be.open_and_prove(gt, gz, gq, nperm, ch)
        be.set_fri_reduction(("fixed", [4, 4]))
        assert be.open_and_prove(gt, gz, gq, nperm, a) == want
        be.set_fri_reduction(("constant_arity_bits",))
        assert be.open_and_prove(gt, gz, gq, nperm, b) == want
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------ 3. whole proofs
def span_place(span):
    import re
    m = re.match(r"table (\d+): ", span)
    table = int(m.group(1)) if m else int(re.match(r"compress_challenges\[(\d+)\]", span).group(1))
    q = re.search(r"fri\.query\[(\d+)\]\.(?:initial_trees_proof|step)\[(\d+)\]", span)
    return (table, int(q.group(1)), int(q.group(2))) if q else (table, None, None)


REFERENCE = {"Err verifier.rs:295": ("QUOTIENT_IDENTITY",), "Err verifier.rs:52": ("POW",), "Err verifier.rs:218": ("FRI_CONSISTENCY",),
             "Err merkle_proofs.rs:71": ("MERKLE_INITIAL", "MERKLE_COMMIT")}
SHAPE_REASONS = ("SHAPE_CAP_HEIGHT", "SHAPE_QUERY_ROUNDS", "SHAPE_INITIAL_PROOFS", "SHAPE_LEAF_LEN", "SHAPE_INITIAL_PATH_LEN", "SHAPE_STEPS", "SHAPE_EVALS_LEN",
                 "SHAPE_STEP_PATH_LEN", "SHAPE_FINAL_POLY_LEN")


@pytest.fixture(scope="module")
def mini():
    return T.ola_stark(**MINI).blob(), M.instance(M.fibonacci(5), **MINI)


def still_works(be, mini):
    blob, (traces, params, compress) = mini
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    res = be.verify_all_proof(blob, proof)
    assert res and res.kernel_launches == 2, res


def test_committed_minsize_proof_its_verdicts_and_the_other_strategys_refusal(mini):
    from olavm_amd.backend import Backend
    from tests.make_ref_verdict import instance
    raw = open(os.path.join(DIR, "wide_program_blake3_minsize.proof"), "rb").read()
    rec = json.load(open(os.path.join(DIR, "wide_program_blake3_minsize.json")))
    default_raw = open(os.path.join(DIR, "wide_program_blake3.proof"), "rb").read()
    blob = T.ola_stark().blob()
    traces, params, compress = instance()
    ms, df = Backend(device=0, hasher="blake3", fri_reduction=("min_size", None)), Backend(device=0, hasher="blake3")
    try:
        got = bytes(ms.prove_with_traces(blob, traces, params, compress))
        print("proof bytes: MinSize(None) %d, ConstantArityBits(4, 5) %d" % (len(got), len(default_raw)))
        assert got == raw, "ola_prove_with_traces under MinSize(None) does not return the committed proof"
        # strictly shorter: by the reference's estimate every table's FRI part is smaller or equal, and no layer cap is added
        assert len(raw) < len(default_raw) and (rec["proof_bytes"], len(default_raw)) == (len(raw), 586616)
        for shape, layers in zip(rec["trace_shapes"], rec["fri_layers"]):
            db = shape[1].bit_length() - 1
            plan, const = FP.arity_bits(("min_size", None), db), FP.arity_bits(("constant_arity_bits",), db)
            assert len(plan) == layers <= len(const) and FP.relative_proof_size(db, 3, 28, plan) <= FP.relative_proof_size(db, 3, 28, const)
        assert sorted(set(rec["fri_layers"])) == [0, 1, 2, 3]
        res = ms.verify_all_proof(blob, raw)
        assert res and res.reason == "OK" and (res.table, res.query, res.oracle_or_layer) == (None, None, None), res
        assert res.query_jobs == 28 * 12 and res.merkle_jobs == 28 * sum(3 + l for l in rec["fri_layers"]) and res.kernel_launches == 2
        assert len(rec["tampered"]) == 19
        for t in rec["tampered"]:
            bad = bytearray(raw)
            bad[t["byte"]] ^= 1 << t["bit"]
            res = ms.verify_all_proof(blob, bytes(bad))
            table, query, which = span_place(t["span"])
            assert not res and res.reason in REFERENCE[t["reference"]], (t, res)         # where the reference's verifier stopped
            assert res.table == table, (t, res)
            if query is not None:
                assert (res.query, res.oracle_or_layer) == (query, which), (t, res)
                assert res.reason == ("FRI_CONSISTENCY" if t["reference"] == "Err verifier.rs:218" else "MERKLE_COMMIT" if ".step[" in t["span"] else "MERKLE_INITIAL")
            else:
                assert (res.query, res.oracle_or_layer) == (None, None), (t, res)
        # each strategy's verifier refuses the other's proof at a shape check, nothing faults, and both contexts go on working
        res = df.verify_all_proof(blob, raw)
        assert not res and res.reason in SHAPE_REASONS, res
        res = ms.verify_all_proof(blob, default_raw)
        assert not res and res.reason in SHAPE_REASONS, res
        assert df.verify_all_proof(blob, default_raw) and ms.verify_all_proof(blob, raw)
        still_works(df, mini)
        still_works(ms, mini)
    finally:
        ms.close()
        df.close()


@pytest.mark.parametrize("strategy", [("min_size", None), ("min_size", 3), ("fixed", [3])], ids=["min_size", "min_size_3", "fixed_3"])
def test_executed_programs_and_the_padding_instance_under_each_strategy(oracle, strategy):
    """A Fixed plan serves every table of a proof, as in the reference: [3] fits tables of 16 rows and more (3 <= degree_bits + 3 - 4), so
    under it an instance with a smaller table is refused with the reference's words and the context goes on -- that is all ten of them
    (the reference's own `final_poly_len` underflows there); a two-table set of 16-row tables is what Fixed([3]) proves."""
    from olavm_amd.backend import Backend, OlaGpuError
    be = Backend(device=0, fri_reduction=strategy)
    try:
        blob = T.ola_stark(**MINI).blob()
        instances = {name: M.instance(make(), **MINI, **kw) for name, (make, kw) in M.EXAMPLES.items()}
        instances["padding"] = tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(3))
        assert len(instances) == 10
        proven = 0
        for name, (traces, params, compress) in instances.items():
            bits = [t.shape[1].bit_length() - 1 for t in traces]
            fits = all(FP.arity_bits(strategy, d) == [] or sum(FP.arity_bits(strategy, d)) <= min(d, d + 3 - 4) for d in bits)
            if not fits:
                assert strategy[0] == "fixed"
                with pytest.raises(OlaGpuError) as e:
                    be.prove_with_traces(blob, traces, params, compress)
                assert e.value.code == OLA_E_INVALID_ARG and "FRI total reduction arity is too large." in str(e.value), name
                continue
            proof = bytes(be.prove_with_traces(blob, traces, params, compress))
            res = be.verify_all_proof(blob, proof, params)
            assert res, (name, res)
            assert be.verify_all_proof(blob, proof), name
            proven += 1
        # every one of the ten has a table of two or four rows, which no layer of arity 8 fits: MinSize plans no layer there, Fixed is refused
        assert proven == (10 if strategy[0] == "min_size" else 0)
        if strategy[0] == "fixed":
            # a set whose tables take the list exactly (16 rows each: 3 <= 4 + 3 - 4): proven, accepted, and not the default strategy's proof
            from olavm_amd.air import AirSet
            cmp_t, rc_t = tracegen.cmp_rangecheck_instance(np.random.default_rng(11), 16, 4)
            assert (cmp_t.shape[1], rc_t.shape[1]) == (16, 16)
            two = AirSet([T.cmp_table(), T.rangecheck_table(4)], [T.ctl_cmp_rangecheck(0, 1)]).blob()
            proof = bytes(be.prove_with_traces(two, [cmp_t, rc_t]))
            res = be.verify_all_proof(two, proof)
            assert res and res.merkle_jobs == 28 * (3 + 1) * 2, res
            be.set_fri_reduction(None)
            res = be.verify_all_proof(two, proof)
            assert not res and res.reason in SHAPE_REASONS, res
            assert oracle.verify_all_proof(two, bytes(be.prove_with_traces(two, [cmp_t, rc_t]))) == (0, "")
            be.set_fri_reduction(strategy)
        # a plan too large for the small tables: refused, then a correct proof from the same context
        be.set_fri_reduction(("fixed", [4, 4, 4]))
        traces, params, compress = instances["fibonacci"]
        with pytest.raises(OlaGpuError) as e:
            be.prove_with_traces(blob, traces, params, compress)
        assert e.value.code == OLA_E_INVALID_ARG and "FRI total reduction arity is too large." in str(e.value)
        with pytest.raises(OlaGpuError) as e:
            be.set_fri_reduction(("fixed", [4, 5]))            # refused: the previous strategy stays
        assert e.value.code == OLA_E_INVALID_ARG
        with pytest.raises(OlaGpuError):
            be.prove_with_traces(blob, traces, params, compress)
        be.set_fri_reduction(strategy if strategy[0] == "min_size" else ("min_size", None))
        proof = bytes(be.prove_with_traces(blob, traces, params, compress))
        assert be.verify_all_proof(blob, proof, params)
        # the oracle's verifier has no MinSize; under the default strategy the library's bytes are the oracle's to judge again
        be.set_fri_reduction(None)
        proof = bytes(be.prove_with_traces(blob, traces, params, compress))
        assert oracle.verify_all_proof(blob, proof, params) == (0, "")
    finally:
        be.close()


def ext_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    v = np.frombuffer(buf, dtype="<u8", count=2 * k, offset=at + 4).reshape(k, 2)
    return v, at + 4 + 16 * k


def field_vec(buf, at):
    (k,) = struct.unpack_from("<I", buf, at)
    return np.frombuffer(buf, dtype="<u8", count=k, offset=at + 4), at + 4 + 8 * k


@pytest.mark.parametrize("log_n", [12, 16])
def test_steps_under_minsize_reassemble_the_fused_proof_and_verify(log_n):
    from olavm_amd.backend import Backend, Challenger
    cols, nperm = (7, 4, 2), 1
    be = Backend(device=0, fri_reduction=("min_size", None))
    try:
        rng = np.random.default_rng(7100 + log_n)
        n = 1 << log_n
        gt, gz, gq = be.commit(rand_field(rng, (cols[0], n))), be.commit(rand_field(rng, (cols[1], n))), be.commit(rand_field(rng, (cols[2], n)), from_coeffs=True)
        ch = Challenger()
        for b in (gt, gz, gq):
            ch.observe_cap(b.cap())
        mine, verifier = ch.clone(), ch.clone()
        want_open, want_fri = be.open_and_prove(gt, gz, gq, nperm, ch)
        zeta = mine.get(2)
        got_open, fri = be.open(gt, gz, gq, nperm, zeta)
        assert got_open == want_open and fri.arity_bits == FP.arity_bits(("min_size", None), log_n) == {12: [4], 16: [4, 4]}[log_n]
        local, at = ext_vec(got_open, 0)
        nxt, at = ext_vec(got_open, at)
        zs_local, at = ext_vec(got_open, at)
        zs_next, at = ext_vec(got_open, at)
        ctl_last, at = field_vec(got_open, at)
        q_local, at = ext_vec(got_open, at)
        for v in (local, zs_local, q_local, nxt, zs_next):
            mine.observe(v)
        mine.observe(np.stack([ctl_last, np.zeros_like(ctl_last)], axis=1))
        fri.begin(mine.get(2))
        caps, beta = [], None
        for _ in fri.arity_bits:
            cap = fri.next_layer(beta)
            caps.append(cap)
            mine.observe_cap(cap)
            beta = mine.get(2)
        final_poly = fri.finish(beta)
        assert final_poly.shape == (fri.final_poly_len, 2) == (1 << (log_n - sum(fri.arity_bits)), 2)
        mine.observe(final_poly)
        witness = be.pow(mine.get(4), bits=16)
        xs = np.array([int(mine.get()) % (n << 3) for _ in range(28)], dtype=np.uint64)
        queries = fri.query(xs)
        fri.free()
        out = struct.pack("<I", len(caps))
        for cap in caps:
            out += struct.pack("<I", cap.shape[0]) + cap.astype("<u8").tobytes()
        head = len(out)
        out += queries
        out += struct.pack("<I", final_poly.shape[0]) + final_poly.astype("<u8").tobytes()
        out += struct.pack("<Q", int(witness))
        assert out == want_fri and mine.get() == ch.get()
        trio = np.stack([gt.cap(), gz.cap(), gq.cap()])
        res = be.verify_opening(trio, cols, log_n, nperm, want_open + want_fri, verifier.clone())
        assert res and res.reason == "OK", res
        if log_n == 16:
            # one evaluation of the second layer of query 0, not the one the first layer's fold is compared with: the path of that layer
            # no longer verifies, and if the flipped one is the compared one the consistency check fails -- at layer 1 either way
            at = head + 4 + 4                                                  # query count, then query 0: number of initial proofs
            for c in cols:
                at += 4 + 8 * c + 1 + 32 * (log_n + 3 - 4)                     # row, path
            at += 4                                                            # number of steps
            at += 4 + 16 * 16 + 1 + 32 * (log_n + 3 - 4 - 4)                   # step 0: 16 evaluations, path
            (k,) = struct.unpack_from("<I", want_fri, at)
            assert k == 16
            bad = bytearray(want_fri)
            bad[at + 4 + 16 * 5] ^= 1
            res = be.verify_opening(trio, cols, log_n, nperm, want_open + bytes(bad), verifier.clone())
            assert not res and res.reason in ("FRI_CONSISTENCY", "MERKLE_COMMIT") and (res.query, res.oracle_or_layer) == (0, 1), res
            # the default strategy plans [4, 4, 4] for 2^16 rows: a shape refusal
            be.set_fri_reduction(None)
            res = be.verify_opening(trio, cols, log_n, nperm, want_open + want_fri, verifier.clone())
            assert not res and res.reason in SHAPE_REASONS, res
        for b in (gt, gz, gq):
            b.free()
    finally:
        be.close()


def test_multi_rank_contexts_keep_constant_arities(mini):
    """The coset partition's first FRI layer is tested for arity 16: a context of two ranks (here two logical ranks on one GPU) refuses
    Fixed and MinSize with a stated reason, keeps its strategy and goes on proving; so does a one-device context that is given a shard."""
    from olavm_amd.backend import Backend, OlaGpuError
    with pytest.raises(OlaGpuError) as e:
        Backend(devices=[0, 0], fri_reduction=("min_size", None))
    assert e.value.code == OLA_E_INVALID_ARG and "single-device contexts" in str(e.value)
    be = Backend(devices=[0, 0])
    try:
        for strategy in (("min_size", None), ("fixed", [4, 3])):
            with pytest.raises(OlaGpuError) as e:
                be.set_fri_reduction(strategy)
            assert e.value.code == OLA_E_INVALID_ARG and "single-device contexts" in str(e.value)
        be.set_fri_reduction(("constant_arity_bits",))
        blob, (traces, params, compress) = mini
        proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    finally:
        be.close()
    one = Backend(device=0)
    try:
        assert bytes(one.prove_with_traces(blob, traces, params, compress)) == proof
        assert one.verify_all_proof(blob, proof)
    finally:
        one.close()
