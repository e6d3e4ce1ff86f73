"""exact_ref.model (a closed form in numpy) equals the oracle bit for bit, under assert_exact, on the
exact-class streams with the special groups planted: what tests/test_gpu_exact.py expects of the
HIP path is pinned here, without a GPU, before any kernel runs."""
import numpy as np
import pytest

import exact_ref
from exact_ref import assert_exact
from ksql_amd import abi

COLS = ["i32", "i64", "x", "x"]
TYPES = [exact_ref.COL_TYPE[c] for c in COLS]
ALL_AGGS = [("COUNT_STAR", -1), ("COUNT", 0), ("SUM", 0), ("SUM", 1), ("SUM", 2), ("MIN", 0), ("MAX", 0),
            ("MIN", 1), ("MAX", 1), ("MIN", 2), ("MAX", 2), ("AVG", 0), ("AVG", 1), ("AVG", 2), ("COUNT", 2),
            ("SUM", 3)]
SUM_X = 4
WINDOWS = {"none": dict(window_kind="NONE"), "tumbling": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=2000)}


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


def _stream(e, pushes, seed=0):
    return exact_ref.make_stream(np.random.default_rng(5000 + e + pushes + seed), pushes, 20_000, 24, e, 2000, 500,
                                 jump=100_000 if pushes == 4 else 0)


def _model(stream, win, having=None):
    w = WINDOWS[win]
    return exact_ref.model(stream, w.get("size_ms", 0), COLS, ALL_AGGS, w.get("grace_ms", -1), having)


@pytest.mark.parametrize("pushes", [1, 3, 4])
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("e", exact_ref.SCALES)
def test_model_equals_oracle(orc, e, win, pushes):
    stream = _stream(e, pushes)
    exp = _model(stream, win)
    o = abi.AggHandle(orc, abi.make_agg_desc(key_type="INT64", col_types=TYPES, aggs=ALL_AGGS, **WINDOWS[win]))
    for p in range(pushes):
        st = o.push(stream.batch(p, COLS))
        assert st["windows_late"] == 0 and st["rows_accepted"] == st["rows_in"]
        assert_exact(o.snapshot(), exp[p]["snapshot"], "snapshot after push %d" % p)
        assert_exact(o.changes(), exp[p]["changes"], "changes of push %d" % p)
    o.close()
    if win == "tumbling" and pushes == 4:  # the jump expired the early windows
        assert exp[-1]["snapshot"]["n"] < exp[-1]["changes"]["n"] + exp[-2]["snapshot"]["n"]
        assert exp[-1]["snapshot"]["ws"].min() > 0


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("op", ["GT", "NE", "LE"])
def test_having_row_sets(orc, op, win):
    """HAVING SUM(x) > 0.0 / != 0.0 / <= 0.0 after every push: a NaN sum matches only !=."""
    stream = _stream(-10, 4, seed=5)
    having = {"agg": SUM_X, "op": op, "value": 0.0}
    exp = _model(stream, win, having)
    full = _model(stream, win)
    o = abi.AggHandle(orc, abi.make_agg_desc(key_type="INT64", col_types=TYPES, aggs=ALL_AGGS, **WINDOWS[win]))
    for p in range(4):
        o.push(stream.batch(p, COLS))
        assert_exact(o.snapshot(having), exp[p]["snapshot"], "push %d" % p)
        s = full[p]["snapshot"]
        nan_keys = s["key"][np.isnan(s["values"][SUM_X])]
        kept = np.isin(nan_keys, exp[p]["snapshot"]["key"])
        assert kept.all() if op == "NE" else not kept.any()
        if win == "none":
            assert (len(nan_keys) >= 5) == (p >= 1)  # the four NaN groups and +Inf - Inf, from push 2 on
    o.close()


def test_special_groups_table():
    """The special groups give what their definition says (the model against literal values, so a
    mistake shared by model and oracle does not pass): unwindowed, after P1, P2, P3."""
    stream = exact_ref.make_stream(np.random.default_rng(3), 3, 1000, 24, 0, 2000, 500)
    aggs = [("SUM", 0), ("AVG", 0), ("MIN", 0), ("MAX", 0), ("COUNT", 0), ("SUM", 1), ("MIN", 1), ("MAX", 1),
            ("SUM", 2), ("AVG", 2)]
    res = exact_ref.model(stream, 0, ["x", "i64", "i32"], aggs)

    def row(p, name):
        s = res[p]["snapshot"]
        r = int(np.flatnonzero(s["key"] == stream.special[name])[0])
        return [None if s["nulls"][a][r] else s["values"][a][r] for a in range(len(aggs))]

    bits = lambda v: np.float64(v).view(np.int64)
    for kind in exact_ref.NANS:
        assert row(0, "nan_" + kind)[:4] == [2.0, 1.0, -3.0, 5.0]
        for p in (1, 2):
            s, a, mn, mx = row(p, "nan_" + kind)[:4]
            assert np.isnan(s) and np.isnan(a) and mn == -3.0 and np.isnan(mx)
    assert row(0, "inf_cancel")[:4] == [np.inf] * 4
    s, a, mn, mx = row(2, "inf_cancel")[:4]
    assert np.isnan(s) and np.isnan(a) and mn == -np.inf and mx == np.inf
    assert row(2, "inf_pos")[:2] == [np.inf, np.inf] and row(2, "inf_neg")[:2] == [-np.inf, -np.inf]
    z = row(2, "neg_zero")
    assert [bits(v) for v in z[:4]] == [bits(0.0), bits(0.0), bits(-0.0), bits(-0.0)]
    z = row(2, "zeros")
    assert [bits(v) for v in z[:4]] == [bits(0.0), bits(0.0), bits(-0.0), bits(0.0)]
    assert row(2, "overflow")[:4] == [np.inf, np.inf, 2.0**1020, 7 * 2.0**1020]
    assert row(0, "overflow")[0] == np.inf  # 32 rows: past 16 * 2^1020 already
    s, a, mn, mx, cnt = row(2, "subnormal")[:5]
    assert s != 0 and abs(s) < 2.3e-308 and cnt == 15 and a == s / 15 and mn < 0 < mx
    assert row(2, "all_null") == [0.0, 0.0, None, None, 0, 0, None, None, 0, 0.0]
    I = exact_ref
    assert row(2, "int_max")[5:] == [-2, I.I64_MAX, I.I64_MAX, -2, -1.0]
    assert row(2, "int_min")[5:] == [I.I64_MIN, I.I64_MIN, I.I64_MIN, I.I32_MIN, float(I.I32_MIN) / 3]
    assert row(2, "int_both")[5:8] == [I.I64_MAX - 1, I.I64_MIN, I.I64_MAX]
    assert exact_ref.plant_signalling(stream)[0] == exact_ref.NANS["signalling"]


def test_assert_exact_tells_zero_signs_and_not_nans():
    a = {"n": 2, "key": np.array([1, 2]), "ws": np.zeros(2, np.int64), "we": np.zeros(2, np.int64),
         "rowtime": np.zeros(2, np.int64), "values": [np.array([0.0, np.nan])], "nulls": [np.zeros(2, bool)]}
    b = dict(a, values=[np.array([0.0, -np.nan])])
    b["values"][0][1:].view(np.uint64)[0] = exact_ref.NANS["payload"]
    assert_exact(a, b)
    c = dict(a, values=[np.array([-0.0, np.nan])])
    with pytest.raises(AssertionError):
        assert_exact(c, a)
    d = dict(a, values=[np.array([5e-324, np.nan])])
    with pytest.raises(AssertionError):
        assert_exact(d, a)
