#!/usr/bin/env python3
"""Extract the WHERE / projection golden cases from the reference's QTT files into
tests/golden/qtt_expr.json.

Runs in the build container only, like make_fixtures.py (whose QTT_DIR / OUT_DIR it uses).  The
cases are named below; each is copied as data: its statements, its input records and its expected
output records, nothing else.  The programs these statements lower to are written by hand in
tests/test_expr_ref.py (LOWERED), which fails when a case here has none.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

CASES = {
    "binary-arithmetic.json": ["in projection"],
    "project-filter.json": ["project and filter", "project and negative filter", "Filter on long literal",
                            "Filter on BETWEEN", "Filter on NOT BETWEEN", "Filter on NULL", "Filter on NOT NULL",
                            "Filter on IS DISTINCT FROM", "Filter on IS NOT DISTINCT FROM"],
    "null.json": ["null equals"],
}


def record(r):
    return {"topic": r["topic"], "key": r.get("key"), "value": r.get("value"), "timestamp": r.get("timestamp", 0)}


def main():
    cases = []
    for fname, names in CASES.items():
        tests = {t["name"]: t for t in json.load(open(os.path.join(mf.QTT_DIR, fname)))["tests"]}
        for name in names:
            t = tests[name]
            cases.append({"file": fname, "name": name, "statements": t["statements"],
                          "inputs": [record(r) for r in t["inputs"]], "outputs": [record(r) for r in t["outputs"]]})
    with open(os.path.join(mf.OUT_DIR, "qtt_expr.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_expr_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("expr cases:", len(cases))
    for c in cases:
        print("  kept: %s: %s" % (c["file"], c["name"]))


if __name__ == "__main__":
    sys.exit(main())
