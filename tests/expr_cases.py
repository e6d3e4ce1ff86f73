"""Shared by tests/test_expr_ref.py and tests/test_gpu_expr.py: the fixture cases of
tests/golden/qtt_expr.json as batches, and the comparison of an applied batch with expr_ref's.

The statements are lowered by hand in tests/test_expr_ref.py (LOWERED); this module only turns a
case's records into columns and its expected records into (key, OUT values) rows."""
import json
import os

import numpy as np

import expr_ref as xr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qtt_expr.json")


def load_cases():
    return json.load(open(GOLDEN))["cases"]


def _fields(low, rec):
    """The record's value as {column name: python value or None} (numeric columns only)."""
    v = rec["value"]
    names = [n for n, _ in low["value_cols"]]
    if v is None:
        return None
    if low["format"] == "DELIMITED":
        parts = v.split(",")
        return {n: (parts[i] if i < len(parts) and parts[i] != "" else None) for i, n in enumerate(names)}
    return {n: v.get(n, v.get(n.lower())) for n in names}


def _num(t, s):
    if s is None or t == "STRING":
        return 0
    return float(s) if t == "DOUBLE" else int(s)


def batch_of(case, low):
    """The case's input records as an expr_ref batch.  Columns: the key column first when the
    statement reads it as a value (low["key_col"] = (name, type)), then low["value_cols"]."""
    recs = case["inputs"]
    n = len(recs)
    cols, valid, types = [], [], []
    if low.get("key_col"):
        name, t = low["key_col"]
        types.append(t)
        cols.append(np.asarray([_num(t, r["key"]) for r in recs], xr.NP[xr.TYPE[t]]))
        valid.append(np.asarray([r["key"] is not None for r in recs], bool))
    rows = [_fields(low, r) for r in recs]
    for name, t in low["value_cols"]:
        types.append(t)
        dt = np.int64 if t == "STRING" else xr.NP[xr.TYPE[t]]
        cols.append(np.asarray([_num(t, None if f is None else f[name]) for f in rows], dt))
        valid.append(np.asarray([f is not None and f[name] is not None for f in rows], bool))
    b = {"ts": np.arange(n, dtype=np.int64), "cols": cols, "valid": valid,
         "row_valid": np.asarray([f is not None for f in rows], bool),
         "key_valid": np.asarray([r["key"] is not None for r in recs], bool)}
    if low["key_type"] == "STRING":
        b["utf8_keys"] = [None if r["key"] is None else str(r["key"]).encode() for r in recs]
    else:
        b["key"] = np.asarray([0 if r["key"] is None else int(r["key"]) for r in recs], np.int64)
    return types, b


def expected_rows(case, low):
    """[(key, [OUT values, None for NULL])] the reference emits.  low["outs"]: per OUT column the
    output field (a DELIMITED position or a JSON name) and its type; low["where_field"]: the statement's
    predicate sits in the projection (a BOOLEAN output column), and the rows kept are those where the
    reference computed true."""
    out = []
    for r in case["outputs"]:
        v = r["value"]
        if low.get("where_field") is not None and not v[low["where_field"]]:
            continue
        vals = []
        for field, t in low["outs"]:
            if isinstance(field, int):
                parts = v.split(",")
                s = parts[field] if parts[field] != "" else None
            else:
                s = v.get(field)
            vals.append(None if s is None else (float(s) if t == "DOUBLE" else int(s)))
        out.append((r["key"], vals))
    return out


def result_rows(res, batch, low):
    """An applied batch (expr_ref.apply's or Expr.columns') as expected_rows shapes it."""
    out = []
    for i in range(res["n"]):
        if not res["key_valid"][i]:
            key = None
        elif low["key_type"] == "STRING":
            o = res["key_offsets"]
            key = bytes(res["key_bytes"][o[i]:o[i + 1]]).decode()
        else:
            key = int(res["key"][i])
        out.append((key, [res["cols"][c][i].item() if res["valid"][c][i] else None for c in range(len(low["outs"]))]))
    return out


# ------------------------------------------------------------------ batches for the library

def host_batch(abi, b):
    return abi.HostBatch(b["ts"], keys=b.get("key"), key_valid=b.get("key_valid"), row_valid=b.get("row_valid"),
                         cols=b.get("cols", []), col_valid=b.get("valid", []), utf8_keys=b.get("utf8_keys"),
                         partition=b.get("partition"), stream_time=b.get("stream_time"))


def device_batch(abi, b, torch):
    """The same arrays on the device (bitmaps packed as HostBatch packs them, None when all valid)."""
    h = host_batch(abi, b)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = abi.DeviceBatch(t(h.ts), keys=t(h.keys), key_valid=t(h.key_valid), row_valid=t(h.row_valid),
                        cols=[t(c) for c in h.cols], col_valid=[t(v) for v in h.col_valid],
                        key_offsets=t(h.key_offsets), key_bytes=t(h.key_bytes), partition=t(h.partition),
                        stream_time=t(h.stream_time))
    return d


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, ref, produced_nan=()):
    """Every array of an applied batch (Expr.columns) against expr_ref.apply's, bit for bit.  A NULL
    bitmap of the library means all valid.  produced_nan: OUT columns whose NaNs arithmetic produced —
    there NaN == NaN whatever its sign and payload (the platform's)."""
    n = ref["n"]
    assert got["n"] == n, (got["n"], n)
    for f in ("ts", "partition", "stream_time", "key", "key_offsets", "key_bytes"):
        if ref[f] is None or (n == 0 and got[f] is None):  # (an empty device input has NULL pointers)
            continue
        assert got[f] is not None, f
        assert np.array_equal(got[f], ref[f]), (f, got[f][:8], ref[f][:8])
    for f in ("key_valid", "row_valid"):
        g = np.ones(n, bool) if got[f] is None else got[f]
        assert np.array_equal(g, ref[f]), (f, np.flatnonzero(g != ref[f])[:8])
    assert len(got["cols"]) == len(ref["cols"])
    for c, (gc, rc) in enumerate(zip(got["cols"], ref["cols"])):
        gv = np.ones(n, bool) if got["valid"][c] is None else got["valid"][c]
        assert np.array_equal(gv, ref["valid"][c]), ("valid", c, np.flatnonzero(gv != ref["valid"][c])[:8])
        assert gc.dtype == rc.dtype, (c, gc.dtype, rc.dtype)
        gb, rb = _bits(gc), _bits(rc)
        if c in produced_nan:
            both = np.isnan(gc) & np.isnan(rc)
            gb, rb = np.where(both, 0, gb), np.where(both, 0, rb)
        bad = np.flatnonzero(gb != rb)
        assert bad.size == 0, ("col", c, bad[:8], gc[bad[:8]], rc[bad[:8]])


# ------------------------------------------------------------------ random well-typed programs and edge rows

NUMERIC = ("INT32", "INT64", "DOUBLE")
_NAN_PAYLOAD = xr.bits_f64(0x7FF8000000000123)
EDGE = {
    "INT32": [0, 1, -1, 2, 7, -7, 100, -2**31, 2**31 - 1, 65536, -65536],
    "INT64": [0, 1, -1, 2, 7, -7, 100, -2**63, 2**63 - 1, 2**31, -2**31, 2**32, 2**53 + 1, -(2**53) - 3],
    "DOUBLE": [0.0, -0.0, 1.0, -1.0, 1.5, -2.5, 7.0, float("inf"), float("-inf"), float("nan"), _NAN_PAYLOAD,
               5e-324, -5e-324, 1.1125369292536007e-308, 2.0**31, -2.0**31, 2.0**31 - 0.5, 2.0**63, -2.0**63,
               1.7976931348623157e308, 0.1, 1e16 + 2.0],
}


def random_tree(rng, types, depth, want):
    """A well-typed tree of at most `depth` levels over columns of `types`: want "NUM" or "BOOL".
    Returns (tree, type name)."""
    num_cols = [c for c, t in enumerate(types) if t in NUMERIC]
    if want == "BOOL":
        r = rng.random()
        if depth <= 1 or r < 0.15:
            c = rng.randrange(len(types))  # IS [NOT] NULL of a bare column, STRING columns included
            return (rng.choice(["IS_NULL", "IS_NOT_NULL"]), ("COL", c)), "BOOL"
        if r < 0.60:
            a, _ = random_tree(rng, types, depth - 1, "NUM")
            b, _ = random_tree(rng, types, depth - 1, "NUM")
            return (rng.choice(xr.CMP), a, b), "BOOL"
        if r < 0.70:
            a, _ = random_tree(rng, types, depth - 1, "NUM")
            return (rng.choice(["IS_NULL", "IS_NOT_NULL"]), a), "BOOL"
        if r < 0.80:
            return ("NOT", random_tree(rng, types, depth - 1, "BOOL")[0]), "BOOL"
        return (rng.choice(["AND", "OR"]), random_tree(rng, types, depth - 1, "BOOL")[0],
                random_tree(rng, types, depth - 1, "BOOL")[0]), "BOOL"
    r = rng.random()
    if depth <= 1 or r < 0.2:
        if rng.random() < 0.7:
            c = rng.choice(num_cols)
            return ("COL", c), types[c]
        t = rng.choice(NUMERIC)
        return ({"INT32": "I32", "INT64": "I64", "DOUBLE": "F64"}[t], rng.choice(EDGE[t])), t
    if r < 0.75:
        a, ta = random_tree(rng, types, depth - 1, "NUM")
        b, tb = random_tree(rng, types, depth - 1, "NUM")
        return (rng.choice(xr.ARITH), a, b), NUMERIC[xr.promote(xr.TYPE[ta], xr.TYPE[tb])]
    a, ta = random_tree(rng, types, depth - 1, "NUM")
    if r < 0.85:
        return ("NEG", a), ta
    t = rng.choice(NUMERIC)
    return ({"INT32": "CAST_I32", "INT64": "CAST_I64", "DOUBLE": "CAST_F64"}[t], a), t


def random_program(rng, types, depth=4):
    """Sink trees of a random program within the limits (checked by expr_ref.check)."""
    from ksql_amd import abi
    while True:
        trees = []
        if rng.random() < 0.6:
            trees.append(("WHERE", random_tree(rng, types, depth, "BOOL")[0]))
        sinks = [("OUT", random_tree(rng, types, depth, "NUM")[0]) for _ in range(rng.randint(1, 3))]
        if rng.random() < 0.3:
            sinks.append(("OUT", ("COL", rng.choice([c for c, t in enumerate(types) if t in NUMERIC]))))
        if rng.random() < 0.4:
            k, t = random_tree(rng, types, depth - 1, "NUM")
            sinks.append(("KEY", k if t != "DOUBLE" else ("CAST_I64", k)))
        rng.shuffle(sinks)
        trees += sinks
        try:
            xr.check(types, abi.expr_words(*trees))
        except xr.Unsupported:
            continue
        return trees


def edge_rows(rng, types, n, null_rate=0.15):
    """n rows of edge values: (cols, valid) as expr_ref / HostBatch take them."""
    cols, valid = [], []
    for t in types:
        if t == "STRING":
            cols.append(np.zeros(n, np.int64))
        else:
            cols.append(np.asarray([rng.choice(EDGE[t]) for _ in range(n)], xr.NP[xr.TYPE[t]]))
        valid.append(np.asarray([rng.random() >= null_rate for _ in range(n)], bool))
    return cols, valid
