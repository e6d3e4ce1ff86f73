#!/usr/bin/env python3
"""Extract the CORRELATION golden cases from the reference's QTT file correlation-udaf.json into
tests/golden/qtt_correlation.json.

Runs in the build container only, like make_fixtures.py (whose statement / record parsing it
reuses by import, with a two-argument `correlation(X, Y)` added to the aggregate grammar).  Kept:
the cases over an INT or a BIGINT pair of a stream.  Skipped, and printed with the reason: the DOUBLE
cases (stream and table source), which the device path does not take, and the expectedException
(DELIMITED) case.  The output holds data only (inputs and expected rows); an aggregate is {"kind":
"CORRELATION", "arg_col": x's column, "arg_col2": y's column} and its expected value a double, NaN
kept as NaN (the QTT file writes it as the string "NaN").
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

FILES = ("correlation-udaf.json",)
CORR_RE = re.compile(r"(?is)^CORRELATION\s*\(\s*([\w`.]+)\s*,\s*([\w`.]+)\s*\)$")

_base_parse_agg = mf.parse_agg
_base_conv = mf.conv


def parse_agg(expr, colmap):
    m = CORR_RE.match(expr.strip())
    if not m:
        return _base_parse_agg(expr, colmap)
    x, y = mf.unq(m.group(1)), mf.unq(m.group(2))
    for c in (x, y):
        if c not in colmap:
            raise mf.Skip("agg arg not a value column " + c)
        if colmap[c]["type"] not in ("INT32", "INT64"):
            raise mf.Skip("agg type " + str(colmap[c]["type"]))
    if colmap[x]["type"] != colmap[y]["type"]:
        raise mf.Skip("agg types differ")
    return {"kind": "CORRELATION", "col": x, "col2": y, "type2": colmap[y]["type"]}


def conv(typ, v):
    if typ in ("INT32", "INT64"):  # a CORRELATION result over an integer pair
        if isinstance(v, float):
            return v
        if v == "NaN":
            return float("nan")
    return _base_conv(typ, v)


def add_second_columns(case, test, pending):
    """make_fixtures.extract_agg knows one argument column per aggregate: append each CORRELATION's
    second column to the batch columns (unless an aggregate already reads it) and name it in the spec."""
    d = case["desc"]
    for spec, a in zip(d["aggs"], pending):
        if a.get("kind") != "CORRELATION":
            continue
        names = case.setdefault("_col_names", [None] * len(d["col_types"]))
        names[spec["arg_col"]] = a["col"]
        if a["col2"] not in names:
            names.append(a["col2"])
            d["col_types"].append(a["type2"])
            for row, rec in zip(case["input"], test["inputs"]):
                val = rec.get("value")
                v = None if val is None else {k.upper(): x for k, x in val.items()}.get(a["col2"])
                row["cols"].append(None if v is None else _base_conv(a["type2"], v))
            if case.get("raw"):
                for f in case["raw"]["fields"]:
                    if f["name"] == a["col2"]:
                        f["out"] = len(names) - 1
        spec["arg_col2"] = names.index(a["col2"])
    case.pop("_col_names", None)


def main():
    pending = []

    def recording_parse_agg(expr, colmap):
        a = parse_agg(expr, colmap)
        pending.append(a)
        return {"kind": a["kind"], "col": a["col"]} if a and a.get("kind") == "CORRELATION" else a

    mf.parse_agg = recording_parse_agg
    mf.conv = conv
    cases, skipped = [], []
    for fname in FILES:
        path = os.path.join(mf.QTT_DIR, fname)
        for test in json.load(open(path)).get("tests", []):
            if "expectedException" in test or test.get("properties"):
                skipped.append(("%s: %s" % (fname, test["name"]), "expected exception / properties"))
                continue
            for fmt_tag, t in mf.expand_formats(test):
                name = "%s: %s%s" % (fname, test["name"], " [%s]" % fmt_tag if fmt_tag else "")
                del pending[:]
                try:
                    c = mf.extract_agg(path, t, fmt_tag)
                    add_second_columns(c, t, list(pending))
                    for o in c["outputs"] + c["expected"]:
                        o["values"] = [None if v is None else float(v) for v in o["values"]]
                    cases.append(c)
                except mf.Skip as e:
                    skipped.append((name, str(e)))
    with open(os.path.join(mf.OUT_DIR, "qtt_correlation.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_correlation_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("correlation cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], [(a["kind"], a["arg_col"], a.get("arg_col2")) for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
