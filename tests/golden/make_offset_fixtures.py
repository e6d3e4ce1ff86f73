#!/usr/bin/env python3
"""Extract the LATEST_BY_OFFSET / EARLIEST_BY_OFFSET golden cases from the reference's QTT files
(latest-offset-udaf.json, earliest-offset-udaf.json) into tests/golden/qtt_offset.json, in the
layout tests/qtt.py's load_cases("offset") reads.

Runs in the build container only, like make_fixtures.py (whose statement / record parsing it
reuses, with the two functions added to the aggregate grammar).  Kept: the non-SESSION cases whose
aggregates use the one-argument or (col, bool) forms.  A case with several aggregates is projected
onto its INT / BIGINT / DOUBLE arguments (the aggregates of a query are independent, so dropping
the others from the SELECT list and ignoring their output fields is sound).  Skipped, and printed
with the reason: the N forms (arrays), SESSION windows, DECIMAL and complex types.  The output
holds data only (inputs and expected rows).
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

FILES = ("latest-offset-udaf.json", "earliest-offset-udaf.json")
OFFSET_RE = re.compile(r"(?is)^(LATEST_BY_OFFSET|EARLIEST_BY_OFFSET)\s*\(\s*(.*?)\s*\)$")
NUMERIC = ("INT32", "INT64", "DOUBLE")

_base_parse_agg = mf.parse_agg


def offset_call(expr):
    """(function, column, ignore_nulls) of a scalar offset aggregate call, None when expr is not
    one; Skip for the N forms."""
    m = OFFSET_RE.match(expr.strip())
    if not m:
        return None
    args = mf.split_top(m.group(2))
    if len(args) == 1:
        ignore = True
    elif len(args) == 2 and args[1].strip().lower() in ("true", "false"):
        ignore = args[1].strip().lower() == "true"
    else:
        raise mf.Skip("N form " + expr.strip())
    if not re.match(r"^[\w`.]+$", args[0].strip()):
        raise mf.Skip("agg arg expr " + args[0])
    return m.group(1).upper(), mf.unq(args[0]), ignore


def parse_agg(expr, colmap):
    oc = offset_call(expr)
    if oc is None:
        return _base_parse_agg(expr, colmap)
    fn, col, ignore = oc
    if col not in colmap:
        raise mf.Skip("agg arg not a value column " + col)
    if colmap[col]["type"] not in NUMERIC:
        raise mf.Skip("agg type " + colmap[col]["type"])
    return {"kind": fn + ("" if ignore else "_NULLS"), "col": col}


def project(test):
    """The test with the offset aggregates over non-numeric columns dropped from the SELECT list
    (kept items keep their output names).  Returns (test, dropped count)."""
    st = test["statements"]
    src = mf.parse_create_source(st[0], "STREAM")
    types = {c["name"]: c["type"] for c in src["cols"]}
    m = re.match(r"(?is)^(\s*CREATE\s+TABLE\s+\w+\s+AS\s+SELECT\s+)(.*?)(\s+FROM\s+.*)$", st[1])
    if not m:
        raise mf.Skip("ctas shape")
    kept, dropped, k = [], 0, 0
    for item in mf.split_top(m.group(2)):
        am = re.match(r"(?is)^(.*?)\s+AS\s+`?(\w+)`?$", item)
        expr = am.group(1) if am else item
        oc = offset_call(expr)
        plain = re.match(r"^[\w`.]+$", expr.strip()) is not None
        if not am and not plain:  # an unaliased expression keeps its KSQL_COL_<i> name
            item = "%s AS KSQL_COL_%d" % (item, k)
            k += 1
        if oc is not None and types.get(oc[1]) not in NUMERIC:
            dropped += 1
            continue
        kept.append(item)
    t = dict(test)
    t["statements"] = [st[0], m.group(1) + ", ".join(kept) + m.group(3)]
    return t, dropped


def main():
    mf.parse_agg = parse_agg
    cases, skipped = [], []
    for fname in FILES:
        path = os.path.join(mf.QTT_DIR, fname)
        for test in json.load(open(path)).get("tests", []):
            name = "%s: %s" % (fname, test["name"])
            try:
                if "expectedException" in test or test.get("properties"):
                    raise mf.Skip("expected exception / properties")
                st = test.get("statements", [])
                if len(st) != 2:
                    raise mf.Skip("statement count")
                if re.search(r"(?i)WINDOW\s+(\w+\s+)?SESSION", st[1]):
                    raise mf.Skip("SESSION window")
                t, dropped = project(test)
                c = mf.extract_agg(path, t, None)
                if not any(a["kind"].startswith(("LATEST", "EARLIEST")) for a in c["desc"]["aggs"]):
                    raise mf.Skip("no INT / BIGINT / DOUBLE offset aggregate left (DECIMAL or complex type)")
                if dropped:
                    c["name"] += " (projected)"
                cases.append(c)
            except mf.Skip as e:
                skipped.append((name, str(e)))
    with open(os.path.join(mf.OUT_DIR, "qtt_offset.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_offset_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("offset cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], [a["kind"] for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
