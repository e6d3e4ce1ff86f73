#!/usr/bin/env python3
"""Extract the TOPK / TOPKDISTINCT golden cases from the reference's QTT files (topk-group-by.json,
topk-distinct.json) into tests/golden/qtt_topk.json.

Runs in the build container only, like make_fixtures.py (whose statement / record parsing it
reuses, with the two functions added to the aggregate grammar and array values converted element by
element).  Kept: `topk(col, k)` / `topkdistinct(col, k)` over an INT / BIGINT / DOUBLE column, in
every value format the extractor handles.  Skipped, and printed with the reason: the struct forms
`topk(col, other..., k)`, STRING / DECIMAL / BYTES / DATE / TIME / TIMESTAMP arguments and the
expectedException cases (DELIMITED cannot carry an array).  The output holds data only (inputs and
expected rows); an aggregate is {"kind": "TOPK" | "TOPKDISTINCT", "k": k, "arg_col": column} and
its expected value a list (the array, descending).
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

FILES = ("topk-group-by.json", "topk-distinct.json")
TOPK_RE = re.compile(r"(?is)^(TOPK|TOPKDISTINCT)\s*\(\s*(.*?)\s*\)$")
NUMERIC = ("INT32", "INT64", "DOUBLE")

_base_parse_agg = mf.parse_agg
_base_conv = mf.conv


def parse_agg(expr, colmap):
    m = TOPK_RE.match(expr.strip())
    if not m:
        return _base_parse_agg(expr, colmap)
    args = [a.strip() for a in mf.split_top(m.group(2))]
    if len(args) != 2:
        raise mf.Skip("struct form " + expr.strip())
    if not re.match(r"^[\w`.]+$", args[0]) or not re.match(r"^\d+$", args[1]):
        raise mf.Skip("agg arg expr " + m.group(2))
    col = mf.unq(args[0])
    if col not in colmap:
        raise mf.Skip("agg arg not a value column " + col)
    if colmap[col]["type"] not in NUMERIC:
        raise mf.Skip("agg type " + str(colmap[col]["type"]))
    # (extract_agg copies "kind" and the column: k rides in the kind until main() splits it off)
    return {"kind": "%s:%d" % (m.group(1).upper(), int(args[1])), "col": col}


def conv(typ, v):
    if isinstance(v, list):  # an ARRAY output value
        return [None if e is None else _base_conv(typ, e) for e in v]
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
                    for a in c["desc"]["aggs"]:
                        if ":" in a["kind"]:
                            a["kind"], k = a["kind"].split(":")
                            a["k"] = int(k)
                    c["sink"] = None  # (khip_sink_encode carries no arrays)
                    cases.append(c)
                except mf.Skip as e:
                    skipped.append((name, str(e)))
    with open(os.path.join(mf.OUT_DIR, "qtt_topk.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_topk_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("topk cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], [(a["kind"], a.get("k")) for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
