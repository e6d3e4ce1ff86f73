"""CPU restatement of a JSON sink value that has ARRAY columns (TEST INFRASTRUCTURE, like
sink_ref.py, on which it is built: the checker of khip_sink_encode's KHIP_SINK_ARRAY columns).

The reference serializes an ARRAY column of a JSON value through the same JsonConverter / Jackson
path as a scalar one: a compact list [e0,e1,...] of elements printed as scalars of the element
type (Long.toString, Double.toString, non-finite doubles as the strings "NaN" / "Infinity" /
"-Infinity"), null for a NULL element, [] for the empty list.  DELIMITED and KAFKA reject an ARRAY
column at plan time (topk-group-by.json "topk DELIMITED"), so there is nothing to restate for them.

A column is (name, type) for a scalar and (name, type, L) for an ARRAY of L slots; an ARRAY's value
is a Python list (None = a NULL element), a scalar's a number or None.
"""
import json
import math

import numpy as np

import qtt
from sink_ref import json_string, json_value


def json_array(typ, vals):
    return "[" + ",".join(json_value(typ, v) for v in vals) + "]"


def encode_value(cols, vals, tombstone=False):
    """The JSON record value of a row; None for a tombstone."""
    if tombstone:
        return None
    fields = []
    for c, v in zip(cols, vals):
        text = json_array(c[1], v) if len(c) > 2 else json_value(c[1], v)
        fields.append(json_string(c[0]) + ":" + text)
    return ("{" + ",".join(fields) + "}").encode()


def row_list(values, null_bytes, r, typ):
    """Row r's list from (n, L) values and the library's null bytes, by the rule of khip_sink_rows:
    the leading slots up to the first byte that is neither 0 (an element) nor 2 (a NULL element)."""
    out = []
    for v, nb in zip(values[r], null_bytes[r]):
        if nb == 2:
            out.append(None)
        elif nb == 0:
            out.append(float(v) if typ == "DOUBLE" else int(v))
        else:
            break
    return out


def pack_lists(lists, L, typ):
    """Lists (None = NULL element) -> ((n, L) values, (n, L) uint8 null bytes); the slots past a
    list's end hold value 0 and byte 1."""
    dt = {"INT32": np.int32, "INT64": np.int64, "DOUBLE": np.float64}[typ]
    vals = np.zeros((len(lists), L), dt)
    nb = np.ones((len(lists), L), np.uint8)
    for r, lst in enumerate(lists):
        for e, x in enumerate(lst):
            nb[r, e] = 2 if x is None else 0
            if x is not None:
                vals[r, e] = x
    return vals, nb


# ------------------------------------------------------------------------------ the QTT fixtures

# The two "(projected)" cases of qtt_offset_n.json carry no "raw" block (their source has BOOLEAN /
# STRING columns, which the fixture projects away), but their statements declare value_format =
# 'JSON' like the rest of latest- / earliest-offset-udaf.json.  Their raw_value keeps the dropped
# fields L3 and L4, which no restatement of the projected query can produce: the comparison is over
# the projected query's columns.
PROJECTED_JSON = ("latest n by offset (projected)", "earliest n by offset (projected)")


def json_cases():
    """Every JSON-format case of qtt_topk.json and qtt_offset_n.json."""
    out = []
    for kind in ("topk", "offset_n"):
        for c in qtt.load_cases(kind):
            raw = c.get("raw")
            if (raw and raw["format"] == "JSON") or (raw is None and c["name"] in PROJECTED_JSON):
                out.append((kind, c))
    return out


def case_columns(case):
    """The sink's value columns of a case, [(name, element type, L)]: aggregate i is output field i
    (the fixture's raw_value has its fields in SELECT order), an ARRAY of the argument's type with
    L = the aggregate's k / N slots."""
    d = case["desc"]
    names = list(case["outputs"][0]["raw_value"])[:len(d["aggs"])]
    return [(nm.upper(), d["col_types"][a["arg_col"]], a["k"]) for nm, a in zip(names, d["aggs"])]


def same_value(got, want, typ):
    """json.loads of our bytes against the fixture's raw_value for one element: integers exact,
    doubles within the QTT comparator's 1e-6, non-finite doubles (stored as text) by their string."""
    if got is None or want is None:
        return got is None and want is None
    if typ == "DOUBLE":
        if isinstance(got, str) or isinstance(want, str):
            return str(got) == str(want)
        return math.isfinite(got) and abs(float(got) - float(want)) < 1e-6
    return type(got) is int and got == want


def assert_parses_to(value_bytes, cols, raw_value):
    got = json.loads(value_bytes)
    assert list(got) == [c[0] for c in cols], (list(got), cols)
    want = {k.upper(): v for k, v in raw_value.items()}
    for name, typ, _ in cols:
        g, w = got[name], want[name]
        assert isinstance(g, list) and len(g) == len(w), (name, g, w)
        assert all(same_value(a, b, typ) for a, b in zip(g, w)), (name, g, w)
