"""The expression step's semantics, on the CPU: tests/expr_ref.py (the pure-Python restatement the GPU
tests compare against) reproduces the reference's own QTT cases (tests/golden/qtt_expr.json) through
the hand-lowered programs below, and holds the edge tables of include/ksqldb_hip.h's "WHERE filters
and computed columns".  Also: the abi.py builder round-trips, the header declares the six entry
points and INTEGRATION.md lists their handles."""
import math
import os
import re

import numpy as np
import pytest

import expr_cases as xc
import expr_ref as xr
from ksql_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1

C1, C2 = ("COL", 0), ("COL", 1)
_PF = dict(format="DELIMITED", key_type="STRING",
           value_cols=[("C1", "INT64"), ("C2", "INT32"), ("C3", "STRING")],
           outs=[(0, "INT64"), (1, "INT32")])  # SELECT *: C3 (STRING) is left out of the projection
_STAR = [("OUT", C1), ("OUT", C2)]
_PF2 = dict(_PF, value_cols=[("C1", "INT64"), ("C2", "INT32")])

# The program each fixture statement lowers to (what the Java side would pass to khip_expr_create).
# Integer literals are INTEGER unless they need a BIGINT; BETWEEN is (x >= lo) AND (x <= hi), NOT
# BETWEEN its NOT, IS NOT DISTINCT FROM the NOT of DISTINCT.
LOWERED = {
    # SELECT col0, col0+col1, col2+10, col1*25, 12*4+2 — col0 is the INT key, read as a value too
    "in projection": dict(
        format="JSON", key_type="INT64", key_col=("col0", "INT32"),
        value_cols=[("col1", "INT64"), ("col2", "DOUBLE")],
        program=[("OUT", ("ADD", ("COL", 0), ("COL", 1))), ("OUT", ("ADD", ("COL", 2), ("I32", 10))),
                 ("OUT", ("MUL", ("COL", 1), ("I32", 25))),
                 ("OUT", ("ADD", ("MUL", ("I32", 12), ("I32", 4)), ("I32", 2)))],
        outs=[("KSQL_COL_0", "INT64"), ("KSQL_COL_1", "DOUBLE"), ("KSQL_COL_2", "INT64"), ("KSQL_COL_3", "INT32")]),
    # SELECT K, name WHERE id > 100 — NAME (STRING) is not projected here
    "project and filter": dict(
        format="DELIMITED", key_type="STRING",
        value_cols=[("ID", "INT64"), ("NAME", "STRING"), ("VALUE", "DOUBLE")],
        program=[("WHERE", ("GT", ("COL", 0), ("I32", 100)))], outs=[]),
    # SELECT K, name, id WHERE id < -100
    "project and negative filter": dict(
        format="DELIMITED", key_type="STRING",
        value_cols=[("ID", "INT64"), ("NAME", "STRING"), ("VALUE", "DOUBLE")],
        program=[("WHERE", ("LT", ("COL", 0), ("I32", -100))), ("OUT", ("COL", 0))], outs=[(1, "INT64")]),
    "Filter on long literal": dict(_PF, program=[("WHERE", ("EQ", C1, ("I64", 4294967296)))] + _STAR),
    "Filter on BETWEEN": dict(
        _PF, program=[("WHERE", ("AND", ("GE", C1, ("I32", 1)), ("LE", C1, ("I32", 3))))] + _STAR),
    "Filter on NOT BETWEEN": dict(
        _PF, program=[("WHERE", ("NOT", ("AND", ("GE", C1, ("I32", 1)), ("LE", C1, ("I32", 3)))))] + _STAR),
    "Filter on NULL": dict(_PF, program=[("WHERE", ("IS_NULL", C1))] + _STAR),
    "Filter on NOT NULL": dict(_PF, program=[("WHERE", ("IS_NOT_NULL", C1))] + _STAR),
    "Filter on IS DISTINCT FROM": dict(_PF2, program=[("WHERE", ("DISTINCT", C1, C2))] + _STAR),
    "Filter on IS NOT DISTINCT FROM": dict(_PF2, program=[("WHERE", ("NOT", ("DISTINCT", C1, C2)))] + _STAR),
    # SELECT ID, ID = COL0, NULL IS NULL: a BOOLEAN does not leave a program, so ID = COL0 runs as the
    # WHERE and the rows kept must be those where the reference computed true (none: a NULL side gives
    # false).  NULL IS NULL has no lowering (there is no NULL literal; the Java side folds it).
    "null equals": dict(
        format="JSON", key_type="INT64", key_col=("ID", "INT32"), value_cols=[("COL0", "INT64")],
        program=[("WHERE", ("EQ", ("COL", 0), ("COL", 1)))], outs=[], where_field="KSQL_COL_0"),
}

CASES = xc.load_cases()


def test_every_fixture_case_has_a_lowering():
    assert len(CASES) == 11
    assert sorted(c["name"] for c in CASES) == sorted(LOWERED)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_reference_restatement_reproduces_the_fixture(case):
    low = LOWERED[case["name"]]
    types, batch = xc.batch_of(case, low)
    res = xr.apply(types, abi.expr_words(*low["program"]), batch)
    assert xc.result_rows(res, batch, low) == xc.expected_rows(case, low)
    assert res["n_errors"] == 0


# ------------------------------------------------------------------ edge tables

def run1(types, tree, values):
    """One row through OUT(tree) (or WHERE(tree) for a BOOLEAN): (state, value)."""
    steps, outs, _, _ = xr.check(types, abi.expr_words(("OUT", tree)))
    _, o, _, errs = xr.eval_row(steps, [(v, v is None) for v in values])
    assert errs == (o[0][0] == xr.ERROR)
    return o[0]


def runb(types, tree, values):
    """A BOOLEAN tree through WHERE: 'T', 'F' or 'E'."""
    steps, _, _, _ = xr.check(types, abi.expr_words(("WHERE", tree)))
    keep, _, _, errs = xr.eval_row(steps, [(v, v is None) for v in values])
    assert not (keep and errs)
    return "E" if errs else "T" if keep else "F"


@pytest.mark.parametrize("t,lo", [("INT32", I32_MIN), ("INT64", I64_MIN)])
def test_integer_division_edges(t, lo):
    a, b = ("COL", 0), ("COL", 1)
    for x in (0, 1, -1, 7, -7, lo, -lo - 1):
        assert run1([t, t], ("DIV", a, b), [x, 0]) == (xr.ERROR, None)
        assert run1([t, t], ("MOD", a, b), [x, 0]) == (xr.ERROR, None)
    assert run1([t, t], ("DIV", a, b), [lo, -1]) == (xr.VALUE, lo)
    assert run1([t, t], ("MOD", a, b), [lo, -1]) == (xr.VALUE, 0)
    assert run1([t, t], ("DIV", a, b), [-7, 2]) == (xr.VALUE, -3)  # toward zero
    assert run1([t, t], ("MOD", a, b), [-7, 2]) == (xr.VALUE, -1)  # the dividend's sign
    assert run1([t, t], ("MOD", a, b), [7, -2]) == (xr.VALUE, 1)
    assert run1([t, t], ("NEG", a), [lo, 0]) == (xr.VALUE, lo)
    assert run1([t, t], ("ADD", a, b), [-lo - 1, 1]) == (xr.VALUE, lo)
    assert run1([t, t], ("MUL", a, b), [lo, -1]) == (xr.VALUE, lo)
    assert run1([t, t], ("ADD", a, b), [None, 1]) == (xr.ERROR, None)  # unboxing a NULL throws


def test_double_division_by_zero_is_not_an_error():
    a, b = ("COL", 0), ("COL", 1)
    t = ["DOUBLE", "DOUBLE"]
    assert run1(t, ("DIV", a, b), [1.0, 0.0]) == (xr.VALUE, math.inf)
    assert run1(t, ("DIV", a, b), [1.0, -0.0]) == (xr.VALUE, -math.inf)
    assert math.isnan(run1(t, ("DIV", a, b), [0.0, 0.0])[1])
    assert math.isnan(run1(t, ("MOD", a, b), [1.0, 0.0])[1])
    assert run1(t, ("MOD", a, b), [-7.5, 2.0]) == (xr.VALUE, -1.5)
    assert run1(["INT32", "DOUBLE"], ("DIV", a, b), [1, 0.0]) == (xr.VALUE, math.inf)  # promoted: no exception


def test_saturating_casts():
    a = ("COL", 0)
    table32 = [(math.nan, 0), (math.inf, I32_MAX), (-math.inf, I32_MIN), (2.0**31, I32_MAX), (-2.0**31, I32_MIN),
               (2.0**31 - 0.5, I32_MAX), (-2.0**31 - 1.5, I32_MIN), (2.0**63, I32_MAX), (-2.0**63, I32_MIN),
               (-1.9, -1), (1.9, 1), (-0.0, 0)]
    for d, want in table32:
        assert run1(["DOUBLE"], ("CAST_I32", a), [d]) == (xr.VALUE, want), d
    table64 = [(math.nan, 0), (math.inf, I64_MAX), (-math.inf, I64_MIN), (2.0**63, I64_MAX), (-2.0**63, I64_MIN),
               (2.0**31, 2**31), (-2.0**31, -2**31), (2.0**63 - 1024, 2**63 - 1024), (-1.9, -1)]
    for d, want in table64:
        assert run1(["DOUBLE"], ("CAST_I64", a), [d]) == (xr.VALUE, want), d
    assert run1(["INT64"], ("CAST_I32", a), [2**32 + 5]) == (xr.VALUE, 5)       # the low 32 bits
    assert run1(["INT64"], ("CAST_I32", a), [2**31]) == (xr.VALUE, I32_MIN)
    assert run1(["INT64"], ("CAST_F64", a), [2**53 + 1]) == (xr.VALUE, 2.0**53)  # ties to even
    assert run1(["INT64"], ("CAST_F64", a), [2**53 + 3]) == (xr.VALUE, 2.0**53 + 4)
    assert run1(["INT64"], ("CAST_F64", a), [None]) == (xr.NULL, None)           # null-safe
    assert run1(["INT64", "INT64"], ("CAST_F64", ("DIV", a, ("COL", 1))), [1, 0]) == (xr.ERROR, None)


def test_nan_under_every_comparison():
    a, b = ("COL", 0), ("COL", 1)
    t = ["DOUBLE", "DOUBLE"]
    for op in xr.CMP:
        for row in ([math.nan, 1.0], [1.0, math.nan], [math.nan, math.nan]):
            assert runb(t, (op, a, b), row) == "F", (op, row)
    assert runb(t, ("EQ", a, b), [-0.0, 0.0]) == "T"
    assert runb(t, ("NE", a, b), [-0.0, 0.0]) == "F"
    assert runb(t, ("DISTINCT", a, b), [-0.0, 0.0]) == "F"


def test_null_and_error_operands_of_a_comparison():
    a, b = ("COL", 0), ("COL", 1)
    t = ["INT64", "INT64"]
    err = ("DIV", ("I64", 1), ("COL", 2))  # ERROR when column 2 is 0
    t3 = t + ["INT64"]
    for op in ("EQ", "NE", "LT", "LE", "GT", "GE"):
        assert runb(t3, (op, a, err), [None, 0, 0]) == "F", op  # a NULL left hides the right side's ERROR
        assert runb(t3, (op, err, a), [None, 0, 0]) == "E", op  # the mirror: the left is evaluated first
        assert runb(t3, (op, a, err), [5, 0, 0]) == "E", op
        assert runb(t3, (op, a, b), [5, None, 0]) == "F", op
        assert runb(t3, (op, a, b), [None, None, 0]) == "F", op
    # IS DISTINCT FROM evaluates both sides on every path
    assert runb(t3, ("DISTINCT", a, err), [None, 0, 0]) == "E"
    assert runb(t3, ("DISTINCT", err, a), [None, 0, 0]) == "E"
    assert runb(t, ("DISTINCT", a, b), [None, None]) == "F"
    assert runb(t, ("DISTINCT", a, b), [None, 3]) == "T"
    assert runb(t, ("DISTINCT", a, b), [3, None]) == "T"
    assert runb(t, ("DISTINCT", a, b), [3, 3]) == "F"
    assert runb(t, ("DISTINCT", a, b), [3, 4]) == "T"
    assert runb(t3, ("IS_NULL", err), [0, 0, 0]) == "E"
    assert runb(t3, ("IS_NOT_NULL", err), [0, 0, 0]) == "E"
    assert runb(t3, ("IS_NULL", err), [0, 0, 2]) == "F"


def test_short_circuit_error_table():
    """Every cell: A, B in {true, false, ERROR}."""
    t = ["INT64", "INT64"]
    # a BOOLEAN from a column: 1 -> true, 0 -> false, 2 -> ERROR
    def boolean(c):
        return ("EQ", ("DIV", ("I64", 2), ("SUB", ("I64", 2), ("COL", c))), ("I64", 2))  # 2 / (2 - x) == 2
    A, B = boolean(0), boolean(1)
    val = {"T": 1, "F": 0, "E": 2}
    and_table = {"TT": "T", "TF": "F", "TE": "E", "FT": "F", "FF": "F", "FE": "F", "ET": "E", "EF": "E", "EE": "E"}
    or_table = {"TT": "T", "TF": "T", "TE": "T", "FT": "T", "FF": "F", "FE": "E", "ET": "E", "EF": "E", "EE": "E"}
    for cell, want in and_table.items():
        assert runb(t, ("AND", A, B), [val[cell[0]], val[cell[1]]]) == want, ("AND", cell)
    for cell, want in or_table.items():
        assert runb(t, ("OR", A, B), [val[cell[0]], val[cell[1]]]) == want, ("OR", cell)
    assert runb(t, ("NOT", A), [2, 0]) == "E"
    assert runb(t, ("NOT", A), [1, 0]) == "F"


def test_promotion_follows_java():
    a, b = ("COL", 0), ("COL", 1)
    assert xr.check(["INT32", "INT32"], abi.expr_words(("OUT", ("ADD", a, b))))[1] == [xr.INT32]
    assert xr.check(["INT32", "INT64"], abi.expr_words(("OUT", ("ADD", a, b))))[1] == [xr.INT64]
    assert xr.check(["INT64", "DOUBLE"], abi.expr_words(("OUT", ("MOD", a, b))))[1] == [xr.DOUBLE]
    assert run1(["INT32", "INT32"], ("MUL", a, b), [65536, 65536]) == (xr.VALUE, 0)  # INT op INT wraps at 32
    assert run1(["INT32", "INT64"], ("MUL", a, b), [65536, 65536]) == (xr.VALUE, 2**32)
    assert run1(["INT64", "DOUBLE"], ("ADD", a, b), [2**53 + 1, 0.0]) == (xr.VALUE, 2.0**53)


def test_sinks_and_errors_are_counted_per_row_and_sink():
    words = abi.expr_words(("WHERE", ("GT", ("COL", 0), ("I32", 0))), ("OUT", ("DIV", ("I32", 10), ("COL", 1))),
                           ("OUT", ("COL", 1)), ("KEY", ("MOD", ("COL", 0), ("COL", 1))))
    b = {"ts": np.arange(6), "key": np.arange(6), "row_valid": [1, 1, 1, 0, 1, 1],
         "cols": [np.asarray([1, 2, -1, 5, 0, 3], np.int32), np.asarray([5, 0, 0, 0, 0, 0], np.int32)],
         "valid": [None, np.asarray([1, 1, 1, 1, 1, 0], bool)]}
    r = xr.apply(["INT32", "INT32"], words, b)
    assert r["rows"].tolist() == [0, 1, 5]     # row 2 and 4 fail the WHERE, row 3 is a null value
    assert r["n_errors"] == 2 + 2              # row 1: OUT 0 and KEY; row 5 (NULL divisor): OUT 0 and KEY
    assert r["valid"][0].tolist() == [True, False, False] and r["valid"][1].tolist() == [True, True, False]
    assert r["cols"][0].tolist() == [2, 0, 0] and r["key"].tolist() == [1, 0, 0]
    assert r["key_valid"].tolist() == [True, False, False]


# ------------------------------------------------------------------ create-time checks of the restatement

def test_restatement_rejects_what_create_rejects():
    C = ("COL", 0)
    w = abi.expr_words
    X = abi.X
    for bad in ([], [99], [X["COL"] | (3 << 32), X["OUT"]], [X["ADD"]], w(C), w(("OUT", ("GT", C, C))),
                w(("WHERE", C)), w(("OUT", ("COL", 1))), w(("OUT", ("IS_NULL", ("IS_NULL", C)))),
                w(("WHERE", ("IS_NULL", C)), ("WHERE", ("IS_NULL", C))), w(("OUT", C), ("WHERE", ("IS_NULL", C))),
                w(("KEY", C), ("KEY", C)), [X["CONST_I64"]], w(("KEY", ("COL", 2)))):
        with pytest.raises(xr.Invalid):
            xr.check(["INT64", "STRING", "DOUBLE"], bad)
    deep = C
    for _ in range(8):
        deep = ("ADD", C, deep)  # right-nested: nine operands on the stack
    for bad in (w(*[("OUT", C)] * 33), w(("OUT", deep)), w(*[("OUT", ("ADD", C, C))] * 22)):
        with pytest.raises(xr.Unsupported):
            xr.check(["INT64"], bad)
    with pytest.raises(xr.Unsupported):
        xr.check(["INT64"] * 65, w(("OUT", C)))
    assert xr.check(["INT64", "STRING"], w(("WHERE", ("IS_NOT_NULL", ("COL", 1)))))[2]


# ------------------------------------------------------------------ builder, header, documents

def test_builder_round_trips():
    trees = [("WHERE", ("GT", ("MUL", ("COL", 0), ("COL", 1)), ("I64", 100))),
             ("OUT", ("ADD", ("CAST_F64", ("COL", 2)), ("F64", -0.0))), ("OUT", ("NEG", ("I32", -7))),
             ("KEY", ("MOD", ("COL", 63), ("I64", I64_MIN)))]
    words = abi.expr_words(*trees)
    assert words[:6] == [abi.X["COL"], abi.X["COL"] | (1 << 32), abi.X["MUL"], abi.X["CONST_I64"], 100, abi.X["GT"]]
    assert all(-2**63 <= w < 2**63 for w in words)
    back = abi.expr_trees(words)
    assert repr(back) == repr(trees)  # (repr: -0.0 and 0.0 compare equal)
    assert abi.expr_words(*back) == words
    assert abi.expr_words(("OUT", ("I32", 2**31))) == [abi.X["CONST_I32"], -2**31, abi.X["OUT"]]  # sign-extended
    assert abi.expr_words(("OUT", ("F64", 1.0)))[1] == 0x3FF0000000000000
    assert {v: k for k, v in abi.X.items()} == xr.OPS


def test_header_opcodes_match_the_binding():
    src = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define KHIP_X_(\w+) (\d+)", src)}
    assert got == abi.X


def test_header_declares_the_entry_points_and_integration_lists_their_handles():
    src = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "typedef struct khip_expr khip_expr;" in src
    for name in ("create", "n_out", "out_type", "apply", "sync", "destroy"):
        assert re.search(r"khip_status khip_expr_%s\(" % name, src), name
        assert re.search(r'MethodHandle EXPR_%s\s*=\s*fn\("khip_expr_%s"' % (name.upper(), name), doc), name
    assert "expr_" + "apply" in abi.PRODUCT_ONLY and hasattr(abi, "Expr")
