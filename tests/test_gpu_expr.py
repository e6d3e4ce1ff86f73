"""khip_expr_apply on the GPU: the device WHERE filter and computed columns / GROUP BY key between
decode and push, against tests/expr_ref.py (bit for bit) and the reference's QTT cases.

Shapes are the smallest at which the kernels can go wrong: around a wave (63 / 64 / 65 rows: the
bitmaps are written one 64-row word per wave), around the block (abi.EXPR_BLOCK = 256) and several
blocks plus one row; every keep pattern moves the compaction's positions differently."""
import ctypes as C
import json
import random
import struct
from fractions import Fraction

import numpy as np
import pytest

import expr_cases as xc
import expr_ref as xr
from ksql_amd import abi
from test_expr_ref import LOWERED

pytestmark = pytest.mark.gpu

KHIP_E_INVALID, KHIP_E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def apply_both(prod, torch, types, words, batch, where, produced_nan=()):
    """The program over the batch as host and as device input, each against expr_ref."""
    ref = xr.apply(types, words, batch)
    e = abi.Expr(prod, types, words)
    try:
        assert [int(t) for t in e.out_types] == ref["out_types"]
        for kind in where:
            b = xc.host_batch(abi, batch) if kind == "host" else xc.device_batch(abi, batch, torch)
            out, nerr = e.apply(b)
            xc.assert_same(e.columns(out), ref, produced_nan)
            assert nerr == ref["n_errors"], (kind, nerr, ref["n_errors"])
    finally:
        e.close()
    return ref


# ------------------------------------------------------------------ the reference's own cases

@pytest.mark.parametrize("case", xc.load_cases(), ids=lambda c: c["name"])
def test_fixture_cases(prod, torch, case):
    low = LOWERED[case["name"]]
    types, batch = xc.batch_of(case, low)
    words = abi.expr_words(*low["program"])
    e = abi.Expr(prod, types, words)
    for kind in ("host", "device"):
        b = xc.host_batch(abi, batch) if kind == "host" else xc.device_batch(abi, batch, torch)
        out, nerr = e.apply(b)
        got = e.columns(out)
        if got["key_valid"] is None:
            got["key_valid"] = np.ones(got["n"], bool)
        for c in range(len(got["valid"])):
            if got["valid"][c] is None:
                got["valid"][c] = np.ones(got["n"], bool)
        assert xc.result_rows(got, batch, low) == xc.expected_rows(case, low), kind
        assert nerr == 0
    e.close()


# ------------------------------------------------------------------ shapes

TYPES3 = ["INT32", "INT64", "DOUBLE"]
A, B, Cc = ("COL", 0), ("COL", 1), ("COL", 2)
WHERE3 = ("WHERE", ("GT", ("MUL", A, B), Cc))
OUTS3 = [("OUT", ("ADD", A, ("I32", 1))), ("OUT", ("MUL", B, ("I32", 2))), ("OUT", ("DIV", Cc, ("F64", 2.0)))]
KEY3 = ("KEY", ("MOD", A, ("I32", 7)))
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 3 * abi.EXPR_BLOCK + 1]
PATTERNS = ["all", "none", "alternating", "ends"]


def shape_batch(rng, n, pattern, bitmaps, keys, extras):
    a = np.asarray([rng.randrange(-50, 50) for _ in range(n)], np.int32)
    b = np.asarray([rng.randrange(-1000, 1000) for _ in range(n)], np.int64)
    keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0,
            "ends": (np.arange(n) == 0) | (np.arange(n) == n - 1)}[pattern]
    c = (a.astype(np.int64) * b).astype(np.float64) + np.where(keep, -0.5, 0.5)  # a*b > c exactly where keep
    batch = {"ts": np.asarray([rng.randrange(-5, 10**6) for _ in range(n)], np.int64), "cols": [a, b, c]}
    if bitmaps:  # every bitmap present, with cleared bits (n % 8 != 0 for most sizes)
        batch["valid"] = [np.asarray([rng.random() > 0.1 for _ in range(n)], bool) for _ in range(3)]
        batch["row_valid"] = np.asarray([rng.random() > 0.1 for _ in range(n)], bool)
        batch["key_valid"] = np.asarray([rng.random() > 0.1 for _ in range(n)], bool)
    if keys == "utf8":
        batch["utf8_keys"] = [b"" if rng.random() < 0.2 else ("k%d" % rng.randrange(10**rng.randrange(1, 9))).encode()
                              for _ in range(n)]
    else:
        batch["key"] = np.asarray([rng.randrange(-2**63, 2**63) for _ in range(n)], np.int64)
    if extras:
        batch["partition"] = np.sort(np.asarray([rng.randrange(4) for _ in range(n)], np.int32))
        batch["stream_time"] = np.maximum.accumulate(np.maximum(batch["ts"], 0)) if n else np.zeros(0, np.int64)
    return batch


@pytest.mark.parametrize("bitmaps,keys,key_sink,extras", [
    (False, "i64", True, False),   # the issue's program: WHERE + three OUTs + KEY, NULL bitmap pointers
    (True, "i64", True, True),
    (False, "i64", False, True),   # the key passes through
    (True, "i64", False, False),
    (False, "utf8", False, False),
    (True, "utf8", False, True),
    (True, "utf8", True, False),   # the KEY sink replaces a UTF-8 key
], ids=lambda v: str(v))
def test_shapes(prod, torch, bitmaps, keys, key_sink, extras):
    trees = [WHERE3] + OUTS3 + ([KEY3] if key_sink else [])
    words = abi.expr_words(*trees)
    rng = random.Random(int(bitmaps) + 2 * (keys == "utf8") + 4 * int(key_sink) + 8 * int(extras))
    e = abi.Expr(prod, TYPES3, words)
    assert e.out_types == [abi.TYPE["INT32"], abi.TYPE["INT64"], abi.TYPE["DOUBLE"]]
    i = 0
    for n in SIZES:
        for pattern in PATTERNS:
            batch = shape_batch(rng, n, pattern, bitmaps, keys, extras)
            ref = xr.apply(TYPES3, words, batch)
            if not bitmaps:
                want = {"all": n, "none": 0, "alternating": (n + 1) // 2, "ends": min(n, 2)}[pattern]
                assert ref["n"] == want
            i += 1
            b = xc.host_batch(abi, batch) if i % 2 else xc.device_batch(abi, batch, torch)
            out, nerr = e.apply(b)
            xc.assert_same(e.columns(out), ref)
            assert nerr == ref["n_errors"]
    e.close()


@pytest.mark.parametrize("keys", ["i64", "utf8"])
@pytest.mark.parametrize("key_sink", [False, True])
def test_without_where_every_row_passes(prod, torch, keys, key_sink):
    """No WHERE: null-value rows keep row_valid 0 and get NULL outputs; untouched arrays pass through."""
    trees = OUTS3 + ([KEY3] if key_sink else [])
    words = abi.expr_words(*trees)
    rng = random.Random(5)
    for n in (0, 1, 65, 257):
        for bitmaps in (False, True):
            batch = shape_batch(rng, n, "alternating", bitmaps, keys, True)
            ref = apply_both(prod, torch, TYPES3, words, batch, ("host", "device"))
            assert ref["n"] == n


def test_device_input_arrays_pass_through_unfiltered(prod, torch):
    """Without a WHERE a device input's ts / key / bitmaps are handed on as they are (the documented alias)."""
    rng = random.Random(6)
    batch = shape_batch(rng, 100, "all", True, "i64", True)
    d = xc.device_batch(abi, batch, torch)
    e = abi.Expr(prod, TYPES3, abi.expr_words(*OUTS3))
    out, _ = e.apply(d, count_errors=False)
    for f in ("ts", "key_i64", "key_valid", "row_valid", "partition", "stream_time"):
        assert getattr(out.struct, f) == getattr(d.struct, f), f
    e.close()


def test_output_goes_straight_to_the_aggregate(prod, torch):
    """No WHERE, n_errors NULL, no khip_expr_sync: apply returns with the work done, so the aggregate
    (another handle, another stream) may read the projected columns at once.  Host and device input."""
    rng = random.Random(8)
    n = 20000
    words = abi.expr_words(("OUT", ("MUL", B, ("CAST_I64", A))))
    batch = shape_batch(rng, n, "all", True, "i64", False)
    batch["key"] = batch["key"] % 50
    batch["ts"] = np.sort(batch["ts"])
    ref = xr.apply(TYPES3, words, batch)
    desc_args = dict(window_kind="TUMBLING", size_ms=100_000, col_types=["INT64"], aggs=[("SUM", 0), ("COUNT", 0)])
    o = abi.AggHandle(abi.load_oracle(), abi.make_agg_desc(**desc_args))
    exp_stats = o.push(abi.HostBatch(ref["ts"], keys=ref["key"], key_valid=ref["key_valid"], row_valid=ref["row_valid"],
                                     cols=ref["cols"], col_valid=ref["valid"]))
    exp = o.snapshot()
    o.close()
    e = abi.Expr(prod, TYPES3, words)
    for kind in ("device", "host"):
        g = abi.AggHandle(prod, abi.make_agg_desc(**desc_args))
        b = xc.host_batch(abi, batch) if kind == "host" else xc.device_batch(abi, batch, torch)
        out, _ = e.apply(b, count_errors=False)
        assert g.push(out) == exp_stats, kind
        got = g.snapshot()
        g.close()
        assert got["n"] == exp["n"] > 0
        for f in ("key", "ws"):
            assert np.array_equal(got[f], exp[f]), (kind, f)
        for a in (0, 1):
            assert np.array_equal(got["values"][a], exp["values"][a]), (kind, a)
    e.close()


# ------------------------------------------------------------------ differential

DIFF_TYPES = ["INT32", "INT64", "DOUBLE", "STRING", "INT64", "DOUBLE", "INT32"]


@pytest.mark.parametrize("chunk", range(4))
def test_random_programs(prod, torch, chunk):
    """200 random well-typed programs (4 x 50; depth <= 4, within the limits), 2,000 edge rows each."""
    rng = random.Random(100 + chunk)
    n = 2000
    cols, valid = xc.edge_rows(rng, DIFF_TYPES, n)
    batch = {"ts": np.arange(n, dtype=np.int64), "key": np.arange(n, dtype=np.int64) % 97, "cols": cols, "valid": valid,
             "row_valid": np.asarray([rng.random() > 0.02 for _ in range(n)], bool)}
    dev = xc.device_batch(abi, batch, torch)
    host = xc.host_batch(abi, batch)
    for i in range(50):
        trees = xc.random_program(rng, DIFF_TYPES)
        words = abi.expr_words(*trees)
        ref = xr.apply(DIFF_TYPES, words, batch)
        # a NaN that only passed COL -> OUT keeps its bits; one that arithmetic produced is "a NaN"
        produced = [c for c, t in enumerate(t for t in trees if t[0] == "OUT") if t[1][0] != "COL"]
        e = abi.Expr(prod, DIFF_TYPES, words)
        try:
            out, nerr = e.apply(dev if i % 2 else host)
            xc.assert_same(e.columns(out), ref, produced)
            assert nerr == ref["n_errors"], (trees, nerr, ref["n_errors"])
        except AssertionError as ex:
            raise AssertionError("program %r: %s" % (trees, ex))
        finally:
            e.close()


def test_double_multiply_add_is_not_contracted(prod, torch):
    """a * b + c with a triple whose fused and two-rounding results differ: the device gives Java's."""
    a = b = 1.0 + 2.0**-30
    c = -(1.0 + 2.0**-29)
    two = a * b + c                                         # a * b rounds to 1 + 2^-29: the sum is 0
    fused = float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding of the exact value: 2^-60
    assert two == 0.0 and fused == 2.0**-60 and two != fused
    n = 70
    batch = {"ts": np.arange(n), "key": np.arange(n), "cols": [np.full(n, a), np.full(n, b), np.full(n, c)]}
    words = abi.expr_words(("OUT", ("ADD", ("MUL", A, B), Cc)), ("OUT", ("SUB", Cc, ("NEG", ("MUL", A, B)))))
    ref = apply_both(prod, torch, ["DOUBLE"] * 3, words, batch, ("host", "device"))
    assert xr.f64_bits(ref["cols"][0][0].item()) == xr.f64_bits(two)


# ------------------------------------------------------------------ decode -> filter / project -> aggregate

def test_decode_filter_project_aggregate(prod, torch):
    """SELECT k, SUM(price * qty), COUNT(*) FROM s WINDOW TUMBLING WHERE amount > 100 GROUP BY k, from the
    JSON record bytes to the snapshot without a host copy of the columns.  Filtered rows carry what the
    aggregate would otherwise count: far-future timestamps (they would advance stream time and make the
    rows after them late), null keys and negative timestamps (they would count as drops)."""
    rng = random.Random(21)
    n = 3000
    fields = [("PRICE", "INT64", 0), ("QTY", "INT32", 1), ("AMOUNT", "DOUBLE", 2)]
    keys, vals, ts = [], [], []
    for i in range(n):
        amount = rng.choice([50.0, 100.0, 100.5, 250.0])
        kept = amount > 100
        t = i * 20
        k = rng.randrange(40)
        if not kept and rng.random() < 0.2:
            t = 10**9 + i   # far in the future
        if rng.random() < 0.05:
            k = None        # kept or not: the aggregate counts only the kept ones
        if rng.random() < 0.03:
            t = -1
        rec = {"PRICE": rng.randrange(-10**6, 10**6), "QTY": rng.randrange(-5, 50), "AMOUNT": amount}
        if rng.random() < 0.05:
            rec["QTY"] = None   # price * qty throws: a NULL argument, and a processing-log record
        if rng.random() < 0.05:
            del rec["AMOUNT"]   # NULL > 100 is false
        keys.append(None if k is None else struct.pack(">q", k))
        vals.append(None if rng.random() < 0.02 else json.dumps(rec).encode())
        ts.append(t)
    ts = np.asarray(ts, np.int64)
    types = ["INT64", "INT32", "DOUBLE"]
    words = abi.expr_words(("WHERE", ("GT", ("COL", 2), ("I32", 100))), ("OUT", ("MUL", ("COL", 0), ("COL", 1))))
    desc_args = dict(window_kind="TUMBLING", size_ms=5_000, grace_ms=1_000, col_types=["INT64"],
                     aggs=[("SUM", 0), ("COUNT_STAR", -1)])

    sd = abi.SerdeHandle(prod, "JSON", fields, key_type="INT64")
    e = abi.Expr(prod, types, words)
    g = abi.AggHandle(prod, abi.make_agg_desc(**desc_args))
    o = abi.AggHandle(abi.load_oracle(), abi.make_agg_desc(**desc_args))
    third = n // 3
    for lo in (0, third, 2 * third):  # three pushes: stream time carries over
        hi = n if lo == 2 * third else lo + third
        d, nerr = sd.decode(ts[lo:hi], keys[lo:hi], vals[lo:hi])
        assert nerr == 0
        dec = sd.columns(d, types)
        out, xerr = e.apply(d)
        got_stats = g.push(out)
        batch = {"ts": ts[lo:hi], "key": dec["key"], "key_valid": dec["key_valid"], "row_valid": dec["row_valid"],
                 "cols": dec["cols"], "valid": dec["valid"]}
        ref = xr.apply(types, words, batch)
        assert 0 < ref["n"] < hi - lo and xerr == ref["n_errors"] > 0
        xc.assert_same(e.columns(out), ref)
        exp_stats = o.push(abi.HostBatch(ref["ts"], keys=ref["key"], key_valid=ref["key_valid"],
                                         row_valid=ref["row_valid"], cols=ref["cols"], col_valid=ref["valid"]))
        assert got_stats == exp_stats, (got_stats, exp_stats)
        assert got_stats["rows_in"] == ref["n"] and got_stats["dropped_null_key"] > 0
    got, exp = g.snapshot(), o.snapshot()
    assert got["n"] == exp["n"] > 0
    for f in ("key", "ws", "we", "rowtime"):
        assert np.array_equal(got[f], exp[f]), f
    for a in (0, 1):
        assert np.array_equal(got["values"][a], exp["values"][a]) and np.array_equal(got["nulls"][a], exp["nulls"][a])
    for h in (sd, e, g, o):
        h.close()


# ------------------------------------------------------------------ errors

def _create(prod, types, words):
    tmap = dict(abi.TYPE, STRING=abi.TYPE_STRING)
    ct = (C.c_int32 * max(len(types), 1))(*[tmap[t] for t in types])
    code = (C.c_int64 * max(len(words), 1))(*words)
    h = C.c_void_p()
    st = prod.expr_create(0, len(types), ct, code, len(words), C.byref(h))
    msg = prod.dll.khip_last_error().decode()
    if st == 0:
        prod.expr_destroy(h)
    return st, msg


_C0 = ("COL", 0)
_DEEP = _C0
for _ in range(8):
    _DEEP = ("ADD", _C0, _DEEP)
_W = abi.expr_words
_ERR_TYPES = ["INT64", "STRING", "DOUBLE"]
INVALID = {
    "unknown opcode": [99],
    "column index out of range": [abi.X["COL"] | (3 << 32), abi.X["OUT"]],
    "stack underflow": [abi.X["ADD"]],
    "values left on the stack": _W(("OUT", _C0)) + _W(_C0),
    "numeric where BOOLEAN is needed": _W(("WHERE", _C0)),
    "BOOLEAN where numeric is needed": _W(("OUT", ("GT", _C0, _C0))),
    "STRING outside IS [NOT] NULL": _W(("OUT", ("NEG", ("COL", 1)))),
    "second WHERE": _W(("WHERE", ("IS_NULL", _C0)), ("WHERE", ("IS_NULL", _C0))),
    "WHERE after another sink": _W(("OUT", _C0), ("WHERE", ("IS_NULL", _C0))),
    "second KEY": _W(("KEY", _C0), ("KEY", _C0)),
    "truncated constant": _W(("OUT", _C0)) + [abi.X["CONST_F64"]],
    "empty program": [],
}
UNSUPPORTED = {
    "more than 64 instruction words": (_ERR_TYPES, _W(*[("OUT", ("ADD", _C0, _C0))] * 22)),
    "stack deeper than 8": (_ERR_TYPES, _W(("OUT", _DEEP))),
    # 33 OUTs need at least 66 words: the word limit refuses the program first
    "more than 32 OUT columns": (_ERR_TYPES, _W(*[("OUT", _C0)] * 33)),
    "more than 64 input columns": (["INT64"] * 65, _W(("OUT", _C0))),
}


@pytest.mark.parametrize("what", sorted(INVALID))
def test_create_invalid(prod, what):
    with pytest.raises(xr.Invalid):
        xr.check(_ERR_TYPES, INVALID[what])
    st, msg = _create(prod, _ERR_TYPES, INVALID[what])
    assert st == KHIP_E_INVALID and msg, (what, st, msg)


@pytest.mark.parametrize("what", sorted(UNSUPPORTED))
def test_create_unsupported(prod, what):
    types, words = UNSUPPORTED[what]
    with pytest.raises(xr.Unsupported):
        xr.check(types, words)
    st, msg = _create(prod, types, words)
    assert st == KHIP_E_UNSUPPORTED and msg, (what, st, msg)


def test_limits_themselves_are_accepted(prod, torch):
    """64 words, a stack of 8, 32 OUT columns, 64 input columns: at the limit, not over it."""
    deep = _C0
    for _ in range(7):
        deep = ("ADD", _C0, deep)  # eight operands on the stack
    assert _create(prod, ["INT64"], _W(("OUT", deep)))[0] == 0
    words = _W(*[("OUT", ("COL", c + 32)) for c in range(32)])
    assert len(words) == 64
    n = 130
    rng = random.Random(3)
    cols, valid = xc.edge_rows(rng, ["INT64"] * 64, n)
    batch = {"ts": np.arange(n), "key": np.arange(n), "cols": cols, "valid": valid}
    ref = apply_both(prod, torch, ["INT64"] * 64, words, batch, ("host", "device"))
    assert len(ref["cols"]) == 32


def test_apply_argument_errors(prod):
    e = abi.Expr(prod, TYPES3, abi.expr_words(WHERE3, *OUTS3))
    few = abi.HostBatch(np.arange(4), keys=np.arange(4), cols=[np.zeros(4, np.int32), np.zeros(4, np.int64)])
    out = abi.Batch()
    st = prod.expr_apply(e.h, C.byref(few.struct), C.byref(out), None)
    assert st == KHIP_E_INVALID and "column" in prod.dll.khip_last_error().decode()
    assert prod.expr_apply(None, C.byref(few.struct), C.byref(out), None) == KHIP_E_INVALID
    assert prod.expr_apply(e.h, None, C.byref(out), None) == KHIP_E_INVALID
    assert prod.expr_sync(None) == KHIP_E_INVALID
    n = C.c_int32()
    assert prod.expr_n_out(None, C.byref(n)) == KHIP_E_INVALID
    assert prod.expr_out_type(e.h, 3, C.byref(n)) == KHIP_E_INVALID
    assert prod.expr_destroy(None) == 0
    e.close()
