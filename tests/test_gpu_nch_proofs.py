"""Whole proofs at StarkConfig::num_challenges 1 and 3, under Poseidon and Blake3.  The CPU oracle's interface has no way to set the
challenge count, so these are CONSISTENCY checks of the library against itself; what ties the pieces to something else is
tests/test_gpu_nch_zcolumns.py and tests/test_gpu_nch_quotient.py (every Z word and every quotient word against Python integers),
tests/test_codegen_host_nch.py and the two-challenge suite around them.

For the nine executed miniature programs, the padding instance and a two-table set:
  ola_verify_all_proof accepts the proof; one flipped bit in a Z opening, a quotient opening and a sibling of the quotient tree is
  refused at its table; a default-configuration context refuses the proof at a shape check, and a context of the other count refuses
  the default's; ola_prove_single_table table by table, and the per-scope calls (ola_perm_z, ola_ctl_z, ola_quotient, commitments,
  ola_open_and_prove with the transcript on the host), reassemble to the whole proof's bytes.
At three challenges the same bytes come from device-resident tables, OLA_LEAN=1, two aliased ranks, ola_prove_from_records and a
child process under OLA_AIR_KERNELS=crosscheck; ola_check_constraints with supplied [3][2] challenges reports nothing on a valid
instance and three OLA_CHECK_LOOKUP entries, kinds 0, 1, 2, for one dropped looked row."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from olavm_amd.air import AirSet, fastexec as F, miniexec as M, ola_tables as T
from tests import tracegen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "integration", "pin"))
MINI = dict(range_bits=4, limb_bits=2)
PROGRAMS = ["fibonacci", "mixed", "memory", "hash", "call", "tape", "storage", "heap", "storage_heavy"]   # tests/test_gpu_stark.py's list
INSTANCES = PROGRAMS + ["padding", "two_tables"]


@pytest.fixture(scope="module")
def backends():
    from olavm_amd.backend import Backend
    made = {}

    def get(hasher, nch, devices=None):
        key = (hasher, nch, None if devices is None else tuple(devices))
        if key not in made:
            kw = dict(devices=devices) if devices else dict(device=0)
            made[key] = Backend(hasher=hasher, num_challenges=nch, **kw)
        return made[key]
    yield get
    for b in made.values():
        b.close()


@functools.lru_cache(maxsize=None)
def instance(name):
    """-> (AirSet, traces, params, compress)"""
    if name == "two_tables":
        cmp_t, rc_t = tracegen.cmp_rangecheck_instance(np.random.default_rng(11), 6, 4)
        return AirSet([T.cmp_table(), T.rangecheck_table(4)], [T.ctl_cmp_rangecheck(0, 1)]), [cmp_t, rc_t], None, None
    s = T.ola_stark(**MINI)
    if name == "padding":
        return (s,) + tuple(tracegen.empty_program_instance(log_n=3, live=np.random.default_rng(5)))
    factory, kwargs = M.EXAMPLES[name]
    return (s,) + tuple(M.instance(factory(), **kwargs))


def cap_bytes(cap):
    return struct.pack("<I", cap.shape[0]) + np.ascontiguousarray(cap, dtype="<u8").tobytes()


def reassembled(be, hasher, s, traces, params, compress):
    """-> (AllProof bytes from ola_prove_single_table table by table, the same from the per-scope calls)"""
    from olavm_amd.backend import Challenger
    nch, blob = be.num_challenges, s.blob()
    batches = [be.commit(t) for t in traces]
    ch = Challenger(hasher=hasher)
    for b in batches:
        ch.observe_cap(b.cap())
    ctl = [(ch.get(), ch.get()) for _ in range(nch)]
    ch_whole = ch.clone()
    head = struct.pack("<I", len(traces))
    tail = struct.pack("<I", len(traces)) + b"".join(struct.pack("<Q", int(c)) for c in (compress if compress is not None else [0] * len(traces)))
    by_table, by_scope, poff = b"", b"", 0
    for t, tr in enumerate(traces):
        shape = be.table_shape(blob, t)
        pr = [] if params is None else params[poff:poff + shape["n_params"]]
        poff += shape["n_params"]
        by_table += be.prove_single_table(blob, t, tr, batches[t], ctl, pr, ch_whole)
        ch.compact()
        perm = [[(ch.get(), ch.get()) for _ in range(nch)] for _ in range(shape["permutation_batch_size"])] if shape["perm_zs"] else None
        n = tr.shape[1]
        zp = be.perm_z(blob, t, tr, perm) if perm else np.zeros((0, n), dtype=np.uint64)
        zc = be.ctl_z(blob, t, tr, ctl)
        assert (zp.shape[0], zc.shape[0]) == (s.tables[t].num_permutation_batches(nch), s.num_ctl_zs(t, nch))
        zs = be.commit(np.concatenate([zp, zc]))
        ch.observe_cap(zs.cap())
        alphas = [ch.get() for _ in range(nch)]
        chunks = be.quotient(blob, t, batches[t], zs, perm, ctl, alphas, pr, n)
        assert chunks.shape == (nch * shape["quotient_degree_factor"], n)
        qb = be.commit(chunks, from_coeffs=True)
        ch.observe_cap(qb.cap())
        openings, fri = be.open_and_prove(batches[t], zs, qb, shape["perm_zs"], ch)
        by_scope += cap_bytes(batches[t].cap()) + cap_bytes(zs.cap()) + cap_bytes(qb.cap()) + openings + fri
        assert np.array_equal(ch.state(), ch_whole.state()), t
        zs.free()
        qb.free()
    for b in batches:
        b.free()
    return head + by_table + tail, head + by_scope + tail


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("name", INSTANCES)
def test_proofs_verify_corruptions_are_placed_and_the_pieces_reassemble(backends, name, nch, hasher):
    import compare_with_dump as CD
    s, traces, params, compress = instance(name)
    blob, be, default = s.blob(), backends(hasher, nch), backends(hasher, 2)
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    res = be.verify_all_proof(blob, proof, params)
    assert res and res.reason == "OK", res
    spans = {n_.split(" (")[0]: (a, b) for n_, a, b in CD.parse_all_proof(proof)}
    # the widths the count decides
    for t, tab in enumerate(s.tables):
        nz = tab.num_permutation_batches(nch) + s.num_ctl_zs(t, nch)
        a, b = spans["table %d: openings.permutation_ctl_zs" % t]
        assert b - a == 16 * nz
        a, b = spans["table %d: openings.quotient_polys" % t]
        assert b - a == 16 * nch * tab.quotient_degree_factor
        a, b = spans["table %d: fri.query[0].initial_trees_proof[2].leaf" % t]
        assert b - a == 8 * nch * tab.quotient_degree_factor
    # one flipped bit: refused at its table
    last = len(s.tables) - 1
    deepest = max(range(len(traces)), key=lambda t: traces[t].shape[1])          # a table whose quotient tree has sibling paths
    for span, table, reason in (("table %d: openings.permutation_ctl_zs" % last, last, None), ("table 1: openings.quotient_polys", 1, None),
                                ("table %d: fri.query[0].initial_trees_proof[2].path" % deepest, deepest, "MERKLE_INITIAL")):
        a, b = spans[span]
        assert b > a, span
        bad = bytearray(proof)
        bad[a + (b - a) // 2] ^= 1
        r = be.verify_all_proof(blob, bytes(bad), params)
        assert not r and r.table == table and reason in (None, r.reason), (span, r)
    # the other configuration's verifier stops at a shape check, both ways
    r = default.verify_all_proof(blob, proof, params)
    assert not r and r.reason.startswith("SHAPE") and r.table == 0, r
    r = be.verify_all_proof(blob, bytes(default.prove_with_traces(blob, traces, params, compress)), params)
    assert not r and r.reason.startswith("SHAPE") and r.table == 0, r
    by_table, by_scope = reassembled(be, hasher, s, traces, params, compress)
    assert by_table == proof, "ola_prove_single_table, table by table"
    assert by_scope == proof, "the per-scope entry points"


def on_device(t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda()


@pytest.mark.parametrize("hasher", ["poseidon", "blake3"])
def test_three_challenges_same_bytes_from_every_proving_mode(backends, monkeypatch, hasher):
    s, traces, params, compress = instance("mixed")
    blob, be = s.blob(), backends(hasher, 3)
    proof = bytes(be.prove_with_traces(blob, traces, params, compress))
    dev = [on_device(t) for t in traces]
    assert bytes(be.prove_with_traces(blob, dev, params, compress)) == proof, "device-resident tables"
    monkeypatch.setenv("OLA_AIR_KERNELS", "interpreter")
    assert bytes(be.prove_with_traces(blob, traces, params, compress)) == proof, "interpreter kernel"
    monkeypatch.delenv("OLA_AIR_KERNELS")
    monkeypatch.setenv("OLA_LEAN", "1")
    assert bytes(be.prove_with_traces(blob, traces, params, compress)) == proof, "OLA_LEAN=1"
    monkeypatch.delenv("OLA_LEAN")
    factory, kwargs = M.EXAMPLES["mixed"]
    rec = F.instance(factory(), records_only=True, **MINI, **kwargs)[3]
    assert be.prove_from_records(blob, rec, result_line=bool(kwargs.get("prove_program_hash")), **MINI) == proof, "ola_prove_from_records"
    # two aliased ranks: tables large enough to go on the coset partition
    big = tracegen.empty_program_instance(log_n=12, live=np.random.default_rng(12))
    two = backends(hasher, 3, devices=[0, 0])
    two.proof_stats(enable=True)
    got = bytes(two.prove_with_traces(blob, *big))
    assert two.proof_stats()["peer_exchanges"] > 0
    assert got == bytes(be.prove_with_traces(blob, *big)), "two aliased ranks"
    assert be.verify_all_proof(blob, got, big[1])


def test_three_challenges_crosscheck_in_a_child_process():
    """OLA_AIR_KERNELS=crosscheck: every table's generated kernel and quotient_kernel<3> on the same inputs, compared on the device"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from olavm_amd.backend import Backend\n"
            "from olavm_amd.air import miniexec as M, ola_tables as T\n"
            "s = T.ola_stark(range_bits=4, limb_bits=2)\n"
            "traces, params, compress = M.instance(M.mixed_program())\n"
            "be = Backend(device=0, num_challenges=3)\n"
            "assert all(be.air_kernels_available(s.blob(), 12))\n"
            "proof = bytes(be.prove_with_traces(s.blob(), traces, params, compress))\n"
            "assert be.verify_all_proof(s.blob(), proof, params)\n"
            "be.close(); print('crosscheck ok', len(proof))\n" % ROOT)
    env = dict(os.environ, OLA_AIR_KERNELS="crosscheck")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "crosscheck ok" in r.stdout, r.stderr[-2000:]


def test_three_challenges_check_constraints_reports_a_dropped_looked_row_three_times(backends):
    s, traces, params, _ = instance("mixed")
    be = backends("poseidon", 3)
    supplied = [(3, 5), (7, 11), (13, 17)]
    assert be.check_constraints(s, traces, params) == []
    assert be.check_constraints(s, traces, params, ctl_challenges=supplied) == []
    found = None
    for li, ctl in enumerate(s.ctls):
        f = ctl.looked_table.filter_column
        if f is None or len(f.terms) != 1 or f.terms[0][1] != 1 or f.constant != 0:
            continue
        t, c = ctl.looked_table.table, f.terms[0][0]
        rows = np.nonzero(traces[t][c] == 1)[0]
        if not len(rows):
            continue
        bad = list(traces)
        bad[t] = traces[t].copy()
        bad[t][c, int(rows[0])] = 0
        got = [d for d in be.check_constraints(s, bad, params, ctl_challenges=supplied) if d["section"] == "LOOKUP"]
        if {d["index"] for d in got} == {li}:
            found = got
            break
    assert found, "no lookup whose looked filter can be dropped alone"
    assert [d["kind"] for d in found] == [0, 1, 2] and len({(d["table"], d["looking_rows"], d["looked_rows"]) for d in found}) == 1
    assert found[0]["looking_rows"] - found[0]["looked_rows"] == 1
