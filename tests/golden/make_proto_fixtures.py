#!/usr/bin/env python3
"""Extract the QTT aggregate cases written for PROTOBUF / PROTOBUF_NOSR into
tests/golden/qtt_proto.json, in the layout tests/qtt.py's load_cases("proto") reads.

Runs in the build container only, like make_fixtures.py, whose extraction it reuses unchanged but
for two settings: the two protobuf formats join the formats that get a "raw" block (the source's
records) and a "sink" block.  On top of make_fixtures.py's case layout every raw record carries
"value_hex", its value serialized by tests/proto_ref.py against the schema ksqlDB derives from the
columns (field numbers 1..n, default representation: a NULL column is absent, which is
make_fixtures.py's null_as_default read the other way), and every expected output "value_hex", the
bytes the sink writes for the expected row (null_as_default again: an expected NULL and an expected
default are both an absent field).  Kept: stream sources with a KAFKA or JSON key, EMIT CHANGES.
Every kept and skipped case is printed.  The output holds data only.

usage: make_proto_fixtures.py [output path]
"""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_fixtures as mf  # noqa: E402
import proto_ref as pr  # noqa: E402

KEY_FORMATS = ("KAFKA", "JSON")
SOURCE_ID, SINK_ID = 11, 12  # the schema ids of the PROTOBUF framing in the fixture's bytes
PTYPE = {"INT32": "int32", "INT64": "int64", "DOUBLE": "double", "STRING": "string"}


def result_type(case, vc):
    if vc["src"] != "AGG":
        return "INT64"
    ag = case["desc"]["aggs"][vc["agg"]]
    if ag["kind"] in ("COUNT", "COUNT_STAR"):
        return "INT64"
    return "DOUBLE" if ag["kind"] == "AVG" else case["desc"]["col_types"][ag["arg_col"]]


def source_value(fmt, fields, value):
    """A QTT input value (JSON object) as the source topic's record value."""
    if value is None:
        return None
    up = {k.upper(): x for k, x in value.items()}
    msg = b""
    for i, f in enumerate(fields):
        x = up.get(f["name"])
        if x is None:
            continue
        x = mf.conv(f["type"], x)
        if x == mf.TYPE_DEFAULT[f["type"]] and not (f["type"] == "DOUBLE" and str(x).startswith("-")):
            continue  # proto3 without presence: the default is not written
        msg += pr.field(i + 1, PTYPE[f["type"]], x)
    return (pr.framing(SOURCE_ID) if fmt == "PROTOBUF" else b"") + msg


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(mf.OUT_DIR, "qtt_proto.json")
    mf.SINK_FORMATS = mf.SINK_FORMATS + mf.PROTO_FORMATS
    mf.RAW_FORMATS = mf.RAW_FORMATS + mf.PROTO_FORMATS
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
                if not re.search(r"(?i)value_format\s*=\s*'PROTOBUF(_NOSR)?'", st[0]) and \
                        not re.search(r"(?i)[^_]format\s*=\s*'PROTOBUF(_NOSR)?'", st[0]):
                    continue
                name = "%s: %s%s" % (os.path.basename(path), t["name"], " [%s]" % fmt_tag if fmt_tag else "")
                try:
                    c = mf.extract_agg(path, t, fmt_tag)
                except mf.Skip as e:
                    skipped.append((name, str(e)))
                    continue
                sk = c["sink"]
                if c["desc"]["table_source"] or not sk or sk["value_format"] not in mf.PROTO_FORMATS:
                    skipped.append((name, "table source or no sink block"))
                elif sk["key_format"] not in KEY_FORMATS:
                    skipped.append((name, "key format " + sk["key_format"]))
                elif c["desc"]["emit"] != "CHANGES":
                    skipped.append((name, "EMIT " + c["desc"]["emit"]))
                else:
                    fmt = sk["value_format"]
                    raw = c["raw"]  # None: the key is not the group column (replayed as columns)
                    if raw:
                        raw["schema_id"] = SOURCE_ID if fmt == "PROTOBUF" else None
                        for rec in raw["records"]:
                            b = source_value(fmt, raw["fields"], rec["value"])
                            rec["value_hex"] = None if b is None else b.hex()
                    sk["schema_id"] = SINK_ID if fmt == "PROTOBUF" else None
                    cols = [(vc["name"], result_type(c, vc)) for vc in sk["value_cols"]]
                    sk["value_types"] = [t for _, t in cols]
                    for o in c["outputs"]:
                        if o["tombstone"]:
                            o["value_hex"] = None
                            continue
                        up = {k.upper(): x for k, x in o["raw_value"].items()}
                        row = [None if up.get(n) is None else mf.conv(t, up[n]) for n, t in cols]
                        o["value_hex"] = pr.encode_value(cols, row, fmt, SINK_ID).hex()
                    cases.append(c)
    with open(out_path, "w") as f:
        json.dump({"generator": "tests/golden/make_proto_fixtures.py", "cases": cases}, f, indent=0, sort_keys=True)
    print("PROTOBUF cases:", len(cases))
    for c in cases:
        print("  kept:", c["name"], c["source"], c["sink"]["value_format"], "key", c["sink"]["key_format"], "window",
              c["desc"]["window_kind"], "raw" if c["raw"] else "no raw", [a["kind"] for a in c["desc"]["aggs"]])
    for name, why in skipped:
        print("  skipped:", name, "--", why)


if __name__ == "__main__":
    sys.exit(main())
