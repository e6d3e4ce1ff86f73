#!/usr/bin/env python3
"""Extract the N-form LATEST_BY_OFFSET / EARLIEST_BY_OFFSET golden cases from the reference's QTT
files (latest-offset-udaf.json, earliest-offset-udaf.json) into tests/golden/qtt_offset_n.json.

Runs in the build container only, like make_offset_fixtures.py, whose cases these complement: it
keeps the scalar forms and prints these as "skipped ... N form".  Kept here: the non-SESSION cases
with a `(col, N)` or `(col, N, ignoreNulls)` call.  As there, a case with several aggregates is
projected onto its INT / BIGINT / DOUBLE arguments (the aggregates of a query are independent, so
dropping the others from the SELECT list and ignoring their output fields is sound); expected
arrays are converted element by element, as make_topk_fixtures.py converts TOPK's, a null element
staying None.  Skipped, and printed with the reason: the scalar forms, SESSION windows, expected
exceptions (N <= 0), and cases with no numeric N-form aggregate left.  The output holds data only
(inputs and expected rows); an aggregate is {"kind": "LATEST_BY_OFFSET" | "EARLIEST_BY_OFFSET"
[+ "_NULLS"], "k": N, "arg_col": column} and its expected value a list, oldest record first.
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
_base_conv = mf.conv


def offset_call(expr):
    """(function, column, N, ignore_nulls) of an offset aggregate call (N = None: a scalar form),
    None when expr is not one."""
    m = OFFSET_RE.match(expr.strip())
    if not m:
        return None
    args = [a.strip() for a in mf.split_top(m.group(2))]
    n, ignore = None, True
    if len(args) >= 2 and re.match(r"^-?\d+$", args[1]):
        n = int(args[1])
        rest = args[2:]
    else:
        rest = args[1:]
    if len(rest) == 1 and rest[0].lower() in ("true", "false"):
        ignore = rest[0].lower() == "true"
    elif rest:
        raise mf.Skip("offset call shape " + expr.strip())
    if not re.match(r"^[\w`.]+$", args[0]):
        raise mf.Skip("agg arg expr " + args[0])
    return m.group(1).upper(), mf.unq(args[0]), n, ignore


def parse_agg(expr, colmap):
    oc = offset_call(expr)
    if oc is None:
        return _base_parse_agg(expr, colmap)
    fn, col, n, ignore = oc
    if col not in colmap:
        raise mf.Skip("agg arg not a value column " + col)
    if colmap[col]["type"] not in NUMERIC:
        raise mf.Skip("agg type " + colmap[col]["type"])
    # (extract_agg copies "kind" and the column: N rides in the kind until main() splits it off)
    return {"kind": fn + ("" if ignore else "_NULLS") + (":%d" % n if n is not None else ""), "col": col}


def conv(typ, v):
    if isinstance(v, list):  # an ARRAY output value
        return [None if e is None else _base_conv(typ, e) for e in v]
    return _base_conv(typ, v)


def project(test):
    """The test with every offset aggregate that is not a numeric N form dropped from the SELECT
    list (kept items keep their output names).  Returns (test, kept N forms, dropped count)."""
    st = test["statements"]
    src = mf.parse_create_source(st[0], "STREAM")
    types = {c["name"]: c["type"] for c in src["cols"]}
    m = re.match(r"(?is)^(\s*CREATE\s+TABLE\s+\w+\s+AS\s+SELECT\s+)(.*?)(\s+FROM\s+.*)$", st[1])
    if not m:
        raise mf.Skip("ctas shape")
    kept, n_forms, scalar, dropped, k = [], 0, 0, 0, 0
    for item in mf.split_top(m.group(2)):
        am = re.match(r"(?is)^(.*?)\s+AS\s+`?(\w+)`?$", item)
        expr = am.group(1) if am else item
        oc = offset_call(expr)
        plain = re.match(r"^[\w`.]+$", expr.strip()) is not None
        if not am and not plain:  # an unaliased expression keeps its KSQL_COL_<i> name
            item = "%s AS KSQL_COL_%d" % (item, k)
            k += 1
        if oc is not None:
            if oc[2] is None:
                scalar += 1
                continue
            if types.get(oc[1]) not in NUMERIC:
                dropped += 1
                continue
            n_forms += 1
        kept.append(item)
    if not n_forms:
        raise mf.Skip("scalar form (qtt_offset.json)" if scalar and not dropped else
                      "no INT / BIGINT / DOUBLE N-form aggregate left (DECIMAL, STRING or complex type)")
    t = dict(test)
    t["statements"] = [st[0], m.group(1) + ", ".join(kept) + m.group(3)]
    return t, n_forms, dropped + scalar


def main():
    mf.parse_agg = parse_agg
    mf.conv = conv
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
                t, _, dropped = project(test)
                c = mf.extract_agg(path, t, None)
                for a in c["desc"]["aggs"]:
                    if ":" in a["kind"]:
                        a["kind"], n = a["kind"].split(":")
                        a["k"] = int(n)
                if dropped:
                    c["name"] += " (projected)"
                c["sink"] = None  # (khip_sink_encode carries no arrays)
                cases.append(c)
            except mf.Skip as e:
                skipped.append((name, str(e)))
    with open(os.path.join(mf.OUT_DIR, "qtt_offset_n.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_offset_n_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("offset N-form cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], [(a["kind"], a.get("k")) for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
