"""The oracle's verdicts as the library's report states them: the words of the oracle's verifier mapped to the OLA_VERIFY_* reason names
(olavm_amd.backend.VERIFY_REASONS), and the comparison of a VerifyResult with an oracle verdict.  Shared by tests/test_gpu_verify.py and
tests/test_gpu_configs.py."""
import re

# the oracle's words (oracle/stark.cpp:456-529, oracle/fri.cpp:250-323) -> the reason of the report
WORDS = [("malformed proof bytes", "MALFORMED"), ("wrong number of table proofs", "MALFORMED"), ("empty FRI proof", "EMPTY_FRI"),
         ("opening width", "SHAPE_OPENING_WIDTH"), ("zs width", "SHAPE_ZS_WIDTH"), ("ctl_zs_last width", "SHAPE_CTL_ZS_LAST_WIDTH"),
         ("quotient width", "SHAPE_QUOTIENT_WIDTH"), ("Mismatch between evaluation and opening of quotient polynomial", "QUOTIENT_IDENTITY"),
         ("cap height", "SHAPE_CAP_HEIGHT"), ("number of query rounds", "SHAPE_QUERY_ROUNDS"), ("initial proofs", "SHAPE_INITIAL_PROOFS"),
         ("leaf len", "SHAPE_LEAF_LEN"), ("initial merkle proof len", "SHAPE_INITIAL_PATH_LEN"), ("steps", "SHAPE_STEPS"),
         ("evals len", "SHAPE_EVALS_LEN"), ("step merkle proof len", "SHAPE_STEP_PATH_LEN"), ("final poly len", "SHAPE_FINAL_POLY_LEN"),
         ("Invalid proof of work witness.", "POW"), ("Invalid Merkle proof (initial tree).", "MERKLE_INITIAL"),
         ("FRI consistency check failed", "FRI_CONSISTENCY"), ("Invalid Merkle proof (commit phase).", "MERKLE_COMMIT"),
         ("Final polynomial evaluation is invalid.", "FINAL_POLY"), ("Cross-table lookup verification failed.", "CTL")]


def oracle_says(rc, msg):
    """(accepted, reason, table) of an oracle verdict"""
    if rc == 0:
        return True, "OK", None
    m = re.match(r"table (\d+): (.*)", msg)
    table, words = (int(m.group(1)), m.group(2)) if m else (None, msg)
    reason = [r for w, r in WORDS if w == words]
    assert len(reason) == 1, msg
    return False, reason[0], table


def agrees(res, rc, msg):
    """the product's result against the oracle's verdict: acceptance, reason, table, and the message starts with the oracle's words"""
    ok, reason, table = oracle_says(rc, msg)
    assert (bool(res), res.reason, res.table) == (ok, reason, table), (res, msg)
    if not ok:
        assert res.message.startswith(msg.split(": ", 1)[1] if table is not None else msg), (res.message, msg)
