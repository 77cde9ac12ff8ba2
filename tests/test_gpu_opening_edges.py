"""The opening evaluations (eval_points_kernel, eval_points_wide_kernel, eval_reduce_kernel), the composition and division
(compose_kernel .. finalize_kernel) and the FRI folds (fold_kernel, fold_pairs_kernel<4>) through the stepped ABI at opening points and
challenges the CALLER chooses -- base-field, (0, 1), small order, zero alpha and beta, non-canonical words -- on coefficient
columns that sit on the edges of the kernels' limb arithmetic and index decomposition, bit for bit against Python integers
(tests/opening_reference.py).  No transcript, proof of work or query is involved.

What is compared: every opened column of every span, and every word of the final polynomial.  The final polynomial depends on the
first n >> 4^layers words of each fold's output only; the rest of a fold's output (zero by construction: fold_pairs_kernel leaves it
to a memset) enters nothing but that layer's committed values.  So for the shapes of CAP_CHECKED the caps that next_layer returns
are compared as well, with the oracle's transform and Merkle tree over the reference's folded polynomials -- that is the only
assertion here that sees a fold's whole output.  Elsewhere the caps stay with the proof-byte comparisons of the other modules.
Whether unwritten words there are noticed without help depends on what the pool hands out (it gives a call sequence the same
blocks in the same roles, and the driver's fresh blocks are zero): with the memsets removed the caps of 2^16 rows differ here, those
of 2^12 rows do not.  tests/test_gpu_fallback_paths.py runs the same steps under OLA_POOL_POISON=1, where both do.

Per shape the three batches are committed once and every challenge set runs on them.  The sizes are the smallest at which a
path exists:
  2^3   no FRI layer: the final polynomial is the composed quotient itself
  2^8   one chunk of eval_points_kernel
  2^11  the first fold in fold_kernel (fewer than 4096 non-zero coefficients) and its nz bookkeeping
  2^12  the first fold in fold_pairs_kernel<4> with nz_out < out_len, the second in fold_kernel
  2^14  four chunks of eval_points_kernel
  2^15  the smallest launch of eval_points_wide_kernel (h = 8, one lo block)
  2^16  fold_pairs_kernel<4> twice
  2^17  h = 9, two lo blocks: blockIdx.x % nlo_blocks and / nlo_blocks
  2^18  more than 16 chunks: eval_reduce_kernel sums on the device
Columns (9, 5, 4) give the wide kernel the groups 4 + 4 + 1 and its surplus-column path, the narrow kernel 8 + 1, and three Zs
opened at g^-1 through the one-point instantiation; (4, 1, 1) with one permutation Z has no third batch."""
import numpy as np
import pytest

from tests import opening_cases as OC, opening_reference as R

pytestmark = pytest.mark.gpu
P = R.P
OLA_E_INVALID_ARG, OLA_E_ZETA_IN_SUBGROUP = -1, -6
ALL = ("random", "base_zeta", "x_zeta", "minus_ones", "order3_zeta", "non_canonical")
SHAPES = [(log_n, OC.MAIN_COLS, OC.MAIN_NPERM, ALL) for log_n in (3, 8, 11, 12, 14, 15, 16, 17)]
SHAPES += [(15, (4, 1, 1), 1, ALL), (15, (1, 3, 2), 0, ALL), (18, (5, 2, 1), 1, ("random", "order3_zeta"))]
CAP_CHECKED = {12: ALL, 16: ("random", "x_zeta")}      # fold_pairs_kernel<4> once / twice with a zero tail behind its outputs
CASES = [pytest.param(s[:3], name, id="2p%d-%s-nperm%d-%s" % (s[0], "x".join(map(str, s[1])), s[2], name)) for s in SHAPES for name in s[3]]


class Committed:
    """the three batches of one shape on the device, and their coefficients as lists of ints"""

    def __init__(self, oracle, shape):
        from olavm_amd.backend import Backend
        self.log_n, self.cols, self.nperm = shape
        trace_c, zs_c, quot_c = OC.stress_batches(self.log_n, self.cols)
        self.be = Backend(device=0)
        self.batches = (self.be.commit(np.stack([oracle.evaluate_poly(c) for c in trace_c])),
                        self.be.commit(np.stack([oracle.evaluate_poly(c) for c in zs_c])),
                        self.be.commit(quot_c, from_coeffs=True))
        for b, want in zip(self.batches, (trace_c, zs_c, quot_c)):          # the coefficients are the intended ones, before anything else
            assert np.array_equal(b.coeffs(), want)
        self.coeffs = [c.tolist() for c in (trace_c, zs_c, quot_c)]
        self.sets = {s[0]: s[1:] for s in OC.challenge_sets(self.log_n, len(R.fri_arity_bits(self.log_n)))}

    def run(self, zeta, alpha, betas):
        """be.open -> begin -> next_layer ... -> finish -> free: (opening-set bytes, final polynomial as a list of pairs, layer caps)"""
        opened, fri = self.be.open(*self.batches, self.nperm, zeta)
        try:
            assert fri.arity_bits == R.fri_arity_bits(self.log_n) and len(betas) == len(fri.arity_bits)
            fri.begin(alpha)
            beta, caps = None, []
            for b in betas:
                caps.append(fri.next_layer(beta))
                beta = b
            final = fri.finish(beta)
            assert final.shape == (fri.final_poly_len, 2)
        finally:
            fri.free()
        return opened, [tuple(r) for r in final.tolist()], caps

    def close(self):
        for b in self.batches:
            b.free()
        self.be.close()


@pytest.fixture(scope="module")
def committed(oracle):
    live = {}

    def get(shape):
        if shape not in live:
            for c in live.values():
                c.close()
            live.clear()
            live[shape] = Committed(oracle, shape)
        return live[shape]
    yield get
    for c in live.values():
        c.close()


def assert_equals_reference(st, opened, final, zeta, alpha, betas, caps=None, oracle=None):
    want = R.open_set(*st.coeffs, st.nperm, zeta)
    got = R.decode_open_set(opened)
    for span in R.SPANS:
        assert len(got[span]) == len(want[span]), span
        wrong = [(span, col, g, w) for col, (g, w) in enumerate(zip(got[span], want[span])) if g != w]
        assert not wrong, "(span, column, got, want): %s" % wrong[:4]
    assert opened == R.open_set_bytes(want)
    layers = R.fri_layers(*st.coeffs, st.nperm, zeta, alpha, betas)
    want_final = R.final_poly(*st.coeffs, st.nperm, zeta, alpha, betas, layers=layers)
    assert len(final) == len(want_final)
    wrong = [(k, g, w) for k, (g, w) in enumerate(zip(final, want_final)) if g != w]
    assert not wrong, "final polynomial, %d words differ, (index, got, want): %s" % (len(wrong), wrong[:4])
    if caps is not None:
        want_caps = R.layer_caps(oracle, layers)
        assert len(caps) == len(want_caps)
        wrong = [i for i, (g, w) in enumerate(zip(caps, want_caps)) if not np.array_equal(g, w)]
        assert not wrong, "the caps of the layers %s differ" % wrong


@pytest.mark.parametrize("shape,name", CASES)
def test_openings_and_final_polynomial_equal_the_integer_reference(committed, oracle, shape, name):
    st = committed(shape)
    zeta, alpha, betas = st.sets[name]
    opened, final, caps = st.run(zeta, alpha, betas)
    check_caps = shape[1] == OC.MAIN_COLS and name in CAP_CHECKED.get(shape[0], ())
    assert_equals_reference(st, opened, final, zeta, alpha, betas, caps if check_caps else None, oracle)
    if name == "non_canonical":             # every returned byte equals the run with the reduced words
        opened_r, final_r, caps_r = st.run(R.ext(zeta), R.ext(alpha), [R.ext(b) for b in betas])
        assert opened == opened_r and final == final_r and all(np.array_equal(a, b) for a, b in zip(caps, caps_r))


@pytest.mark.parametrize("log_n", [8, 15])
def test_refused_opening_points_leave_the_context_usable(committed, log_n):
    """zeta in the subgroup is the reference's own refusal (prover.rs:508-511); zeta = 0 is this library's: its division by
    X - zeta goes through powers of 1 / zeta (finalize_kernel), and ext_inv(0) = 0 would make every quotient zero without an error."""
    from olavm_amd.backend import OlaGpuError
    st = committed((log_n, OC.MAIN_COLS, OC.MAIN_NPERM))
    g = R.root_of_unity(log_n)
    for zeta in ((1, 0), (g, 0), (1 + P, 0)):
        with pytest.raises(OlaGpuError) as e:
            st.be.open(*st.batches, st.nperm, zeta)
        assert e.value.code == OLA_E_ZETA_IN_SUBGROUP, (zeta, str(e.value))
    for zeta in ((0, 0), (P, 0), (P, P)):
        with pytest.raises(OlaGpuError) as e:
            st.be.open(*st.batches, st.nperm, zeta)
        assert e.value.code == OLA_E_INVALID_ARG and "zeta is zero" in str(e.value), (zeta, str(e.value))
    zeta, alpha, betas = st.sets["random"]
    opened, final, _ = st.run(zeta, alpha, betas)
    assert_equals_reference(st, opened, final, zeta, alpha, betas)
