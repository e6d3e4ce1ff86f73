#!/usr/bin/env python3
"""Extract the STDDEV_SAMP / STDDEV_SAMPLE golden cases from the reference's QTT file
standarddeviation.json into tests/golden/qtt_stddev.json.

Runs in the build container only, like make_fixtures.py (whose statement / record parsing it
reuses, with the two functions added to the aggregate grammar and their DOUBLE results kept as
doubles).  Kept: `stddev_samp(col)` / `stddev_sample(col)` over an INT / BIGINT column.  Skipped,
and printed with the reason: the DOUBLE argument and the map element (DOUBLE) cases, which the
device path does not take, and the expectedException (DELIMITED) cases.  The output holds data only
(inputs and expected rows); an aggregate is {"kind": "STDDEV_SAMP" | "STDDEV_SAMPLE", "arg_col":
column} and its expected value a double.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

FILES = ("standarddeviation.json",)
STDDEV_RE = re.compile(r"(?is)^(STDDEV_SAMP|STDDEV_SAMPLE)\s*\(\s*(.*?)\s*\)$")

_base_parse_agg = mf.parse_agg
_base_conv = mf.conv


def parse_agg(expr, colmap):
    m = STDDEV_RE.match(expr.strip())
    if not m:
        return _base_parse_agg(expr, colmap)
    arg = m.group(2)
    if not re.match(r"^[\w`.]+$", arg):
        raise mf.Skip("agg arg expr " + arg)
    col = mf.unq(arg)
    if col not in colmap:
        raise mf.Skip("agg arg not a value column " + col)
    if colmap[col]["type"] not in ("INT32", "INT64"):
        raise mf.Skip("agg type " + str(colmap[col]["type"]))
    return {"kind": m.group(1).upper(), "col": col}


def conv(typ, v):
    if isinstance(v, float) and typ in ("INT32", "INT64"):  # a STDDEV result over an integer column
        return v
    return _base_conv(typ, v)


def main():
    mf.parse_agg = parse_agg
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
                try:
                    c = mf.extract_agg(path, t, fmt_tag)
                    for o in c["outputs"] + c["expected"]:
                        o["values"] = [None if v is None else float(v) for v in o["values"]]
                    cases.append(c)
                except mf.Skip as e:
                    skipped.append((name, str(e)))
    with open(os.path.join(mf.OUT_DIR, "qtt_stddev.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_stddev_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("stddev cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], [a["kind"] for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
