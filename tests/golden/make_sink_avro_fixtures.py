#!/usr/bin/env python3
"""Extract the QTT aggregate cases whose sink topic has an AVRO value into
tests/golden/qtt_sink_avro.json, in the layout tests/qtt.py's load_cases("sink_avro") reads.

Runs in the build container only, like make_fixtures.py, whose extraction it reuses unchanged but
for one setting: AVRO joins the value formats that get a "sink" block (a CREATE TABLE ... AS SELECT
inherits its source's formats, so these are the cases qtt_agg.json carries with "sink": null
because their source is AVRO).  Kept: stream sources with value_format = AVRO and a KAFKA or JSON
key, EMIT CHANGES.  Every kept and skipped AVRO case is printed.  The output holds data only
(inputs, the AVRO input records, expected rows).
"""
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf  # noqa: E402

KEY_FORMATS = ("KAFKA", "JSON")


def main():
    mf.SINK_FORMATS = mf.SINK_FORMATS + ("AVRO",)
    cases, skipped = [], []
    for path in sorted(glob.glob(os.path.join(mf.QTT_DIR, "*.json"))):
        try:
            doc = json.load(open(path))
        except ValueError:
            continue
        for test in doc.get("tests", []):
            props = dict(test.get("properties") or {})
            props.pop(mf.EMIT_INTERVAL, None)
            if "expectedException" in test or props:
                continue
            for fmt_tag, t in mf.expand_formats(test):
                st = t.get("statements", [])
                if len(st) != 2 or not re.search(r"(?i)GROUP\s+BY", st[1]):
                    continue
                name = "%s: %s%s" % (os.path.basename(path), t["name"], " [%s]" % fmt_tag if fmt_tag else "")
                try:
                    c = mf.extract_agg(path, t, fmt_tag)
                except mf.Skip as e:
                    if re.search(r"(?i)value_format\s*=\s*'AVRO'", st[0]):
                        skipped.append((name, str(e)))
                    continue
                sk = c["sink"]
                if c["desc"]["table_source"] or not sk or sk["value_format"] != "AVRO":
                    continue
                if sk["key_format"] not in KEY_FORMATS:
                    skipped.append((name, "key format " + sk["key_format"]))
                elif c["desc"]["emit"] != "CHANGES":
                    skipped.append((name, "EMIT " + c["desc"]["emit"]))
                else:
                    cases.append(c)
    with open(os.path.join(mf.OUT_DIR, "qtt_sink_avro.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_sink_avro_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("AVRO sink cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], c["source"], "key", c["sink"]["key_format"], "window", c["desc"]["window_kind"],
              "raw" if c["raw"] else "no raw", [a["kind"] for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
