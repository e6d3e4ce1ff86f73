#!/usr/bin/env python3
"""Extract the VALUE_DELIMITER cases of the reference's QTT file delimited.json into
tests/golden/delimited_delimiters.json.

Runs in the build container only, like make_fixtures.py (whose QTT_DIR it reads).  Kept: the cases
whose source statement sets value_delimiter to something other than ','.  Per case the output holds
data only: the value delimiter the source reads and the one the sink writes (the source's unless the
sink statement sets its own; TAB / SPACE spelled out as the character), the value columns' names and
types, the input value strings and the expected output value strings.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "delimited_delimiters.json")
DELIM_RE = re.compile(r"(?i)value_delimiter\s*=\s*'([^']*)'")
COLS_RE = re.compile(r"(?is)^CREATE\s+STREAM\s+\w+\s*\((.*?)\)\s*WITH")
TYPES = {"BIGINT": "INT64", "INT": "INT32", "INTEGER": "INT32", "DOUBLE": "DOUBLE", "VARCHAR": "STRING",
         "STRING": "STRING"}
SPELLED = {"TAB": "\t", "SPACE": " "}


def delimiter(stmt):
    m = DELIM_RE.search(stmt)
    return None if not m else SPELLED.get(m.group(1), m.group(1))


def main():
    cases = []
    for test in json.load(open(os.path.join(mf.QTT_DIR, "delimited.json")))["tests"]:
        stmts = test.get("statements", [])
        if len(stmts) != 2 or "expectedException" in test:
            continue
        din = delimiter(stmts[0])
        if din is None or din == ",":
            continue
        cols = []
        for c in COLS_RE.match(stmts[0]).group(1).split(","):
            words = c.split()
            if words[-1].upper() != "KEY":
                cols.append([words[0].upper(), TYPES[words[1].upper()]])
        cases.append({"name": test["name"], "delimiter_in": din, "delimiter_out": delimiter(stmts[1]) or din,
                      "columns": cols, "inputs": [r["value"] for r in test["inputs"]],
                      "outputs": [r["value"] for r in test["outputs"]]})
    json.dump({"source": "query-validation-tests/delimited.json", "cases": cases}, open(OUT, "w"), indent=1)
    print("%d cases -> %s" % (len(cases), OUT))


if __name__ == "__main__":
    main()
