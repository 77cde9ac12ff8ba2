#!/usr/bin/env python3
"""Why does my trace not prove?  Runs the native trace generator on a named example program and prints what ola_check_constraints
says of the twelve tables: per failing constraint the table, the emit's ordinal and kind, its source location in the reference
(tests/golden/air_emit_kinds.json), the first failing row and the number of failing rows; failing permutation batches and
cross-table lookups with the rows each side selects and, from ola_check_lookup, the tuples the two sides carry unequally often.

    python tools/check_trace.py fibonacci                       # a valid trace: nothing to report
    python tools/check_trace.py wide --reference-quirks         # the reference generators' own rows: bitwise limbs, no-row memory table

Programs: the examples of olavm_amd/air/miniexec.py (EXAMPLES) and `wide` (32-bit operands; full-size fixed tables).  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from olavm_amd.air import fastexec, miniexec as M, ola_tables as T
    from olavm_amd.backend import Backend, format_lookup_report
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("program", choices=sorted(M.EXAMPLES) + ["wide"])
    ap.add_argument("--reference-quirks", action="store_true", help="generate the rows the reference's generators write (its AIR rejects two of them)")
    ap.add_argument("--hasher", default="poseidon")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON line")
    ap.add_argument("--max-tuples", type=int, default=16, help="mismatching tuples printed per failing cross-table lookup (ola_check_lookup)")
    a = ap.parse_args()
    if a.program == "wide":
        prog, kwargs, airset = M.wide_program(), {"range_bits": 16, "limb_bits": 8}, T.ola_stark()
    else:
        factory, kwargs = M.EXAMPLES[a.program]
        prog, airset = factory(), T.ola_stark(range_bits=kwargs.get("range_bits", 4), limb_bits=kwargs.get("limb_bits", 2))
    traces, params, _ = fastexec.instance(prog, reference_quirks=a.reference_quirks, **kwargs)
    be = Backend(hasher=a.hasher)
    report = be.check_constraints(airset, traces, params)
    # which tuples a failing lookup is missing (one report per lookup: both challenges fail together)
    lookups = {d["index"]: be.check_lookup(airset, traces, d["index"], max_tuples=a.max_tuples) for d in report if d["section"] == "LOOKUP"}
    be.close()
    if a.json:
        print(json.dumps([dict(d, tuples=lookups[d["index"]]) if d["section"] == "LOOKUP" else d for d in report]))
        return 1 if report else 0
    sites = {}
    fixture = os.path.join(ROOT, "tests", "golden", "air_emit_kinds.json")
    if os.path.exists(fixture):
        sites = {i: d["emit_sites"] for i, d in enumerate(json.load(open(fixture))["tables"])}
    print("%s%s: %s" % (a.program, " (reference quirks)" if a.reference_quirks else "",
                        ", ".join("%s 2^%d" % (t.name, tr.shape[1].bit_length() - 1) for t, tr in zip(airset.tables, traces))))
    for d in report:
        if d["section"] == "AIR":
            where = sites.get(d["table"], [])
            print("table %d %s, constraint #%d (%s%s), first at row %d, %d rows" % (
                d["table"], d["table_name"], d["index"], d["kind"], ", " + where[d["index"]] if d["index"] < len(where) else "", d["first_row"], d["rows_failing"]))
        elif d["section"] == "PERMUTATION":
            print("table %d %s, permutation batch %d: the running product does not close" % (d["table"], d["table_name"], d["index"]))
        else:
            print("lookup %d into table %d %s, challenge %d: %d looking rows, %d looked rows" % (
                d["index"], d["table"], d["table_name"], d["kind"], d["looking_rows"], d["looked_rows"]))
            if d["kind"] == max(x["kind"] for x in report if x["section"] == "LOOKUP" and x["index"] == d["index"]):
                rep = lookups[d["index"]]
                if rep["columns"]:
                    print("  data columns of table %d %s: (%s)" % (rep["looked_table"], rep["looked_table_name"], ", ".join(rep["columns"])))
                print("\n".join("  " + line for line in format_lookup_report(rep, a.max_tuples).split("\n")))
    print("%d entries" % len(report) if report else "every constraint, permutation argument and cross-table lookup holds")
    return 1 if report else 0


if __name__ == "__main__":
    sys.exit(main())
