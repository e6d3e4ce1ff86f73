"""The N forms of LATEST_BY_OFFSET / EARLIEST_BY_OFFSET without a GPU: the extracted QTT cases, the
reference models the GPU tests compare against (tests/offset_n_ref.py), that their synthetic
expectations cover what the lists can get wrong, and the interface constants.

The cases of tests/golden/qtt_offset_n.json (make_offset_n_fixtures.py): the twelve non-SESSION
N-form cases of latest-offset-udaf.json / earliest-offset-udaf.json, the two "n by offset" cases
projected onto their INT / BIGINT / DOUBLE arguments.
"""
import os
import re

import numpy as np
import pytest

import offset_n_ref as nr
import qtt
from ksql_amd import abi

CASES = qtt.load_cases("offset_n")
IDS = [c["name"] for c in CASES]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extracted_cases():
    assert sorted(IDS) == sorted([
        "nulls ignored - multiple", "nulls not ignored - multiple", "latest n by offset (projected)",
        "latest n by offset with nulls", "latest n by offset with all nulls",
        "null first - multiple - ignoring nulls", "null first - multiple - not ignoring nulls",
        "nulls later - multiple - nulls ignored", "null later - multiple - nulls not ignored",
        "earliest n by offset (projected)", "earliest n by offset with nulls", "earliest n by offset with all nulls"])
    kinds = set()
    for c in CASES:
        d = c["desc"]
        assert d["window_kind"] == "NONE" and c["outputs"] and c["input"]
        assert all(a["kind"] in nr.NFORM and a["k"] == 2 for a in d["aggs"])
        assert all(isinstance(v, list) for o in c["outputs"] for v in o["values"])
        kinds |= {a["kind"] for a in d["aggs"]}
    assert kinds == set(nr.NFORM)
    out = [o for c in CASES for o in nr.golden_outputs(c)]
    assert any(None in lst for _, lists in out for lst in lists)   # a NULL element inside a list
    assert any(lst == [] for _, lists in out for lst in lists)     # the empty array
    assert any(len(lst) == 1 for _, lists in out for lst in lists) and any(len(lst) == 2 for _, lists in out for lst in lists)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_qtt(case):
    """aggregate() record by record gives every expected output record (the final table with it)."""
    assert nr.model_outputs(case) == nr.golden_outputs(case)


@pytest.mark.parametrize("split", [1, 2, None])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_expect_reproduces_qtt(case, split):
    """The oracle-derived expectation, fed the case in pushes of 1, 2 and all rows: every push's
    changes are the reference's output records of its rows, in order (one-row pushes), and the final
    table is the last output per key."""
    d = case["desc"]
    e = nr.Expect(abi.load_oracle(), d["col_types"], nr.case_aggs(case), flags=abi.FLAG_CHANGELOG)
    n = len(case["input"])
    step = split or n
    rows = []
    for lo in range(0, n, step):
        part = case["input"][lo:lo + step]
        cols = [np.array([0 if r["cols"][c] is None else r["cols"][c] for r in part], abi.NP_TYPE[abi.TYPE[t]])
                for c, t in enumerate(d["col_types"])]
        valid = [np.array([r["cols"][c] is not None for r in part], bool) for c in range(len(cols))]
        e.push([r["ts"] for r in part], cols, valid, keys=[0 if r["key"] is None else r["key"] for r in part],
               key_valid=[r["key"] is not None for r in part], row_valid=[r["row_valid"] for r in part])
        chg = e.changes()
        per_agg = [nr.lists_of(chg, i) for i in range(len(d["aggs"]))]
        rows += [(int(chg["key"][r]), [per_agg[i][r] for i in range(len(d["aggs"]))]) for r in range(chg["n"])]
    snap = e.snapshot()
    e.close()
    golden = nr.golden_outputs(case)
    if split == 1:
        assert rows == golden
    final = dict(golden)
    per_agg = [nr.lists_of(snap, i) for i in range(len(d["aggs"]))]
    assert [(int(snap["key"][r]), [per_agg[i][r] for i in range(len(d["aggs"]))]) for r in range(snap["n"])] == sorted(final.items())


def test_aggregate_rules():
    lst = []
    for v in (1, None, 2, 3, None, 4):
        lst = nr.aggregate("LATEST_BY_OFFSET", 3, v, lst)
    assert lst == [2, 3, 4]
    lst = []
    for v in (1, None, 2, 3, None):
        lst = nr.aggregate("LATEST_BY_OFFSET_NULLS", 3, v, lst)
    assert lst == [2, 3, None]
    lst = []
    for v in (None, 1, None, 2, 3, 4):
        lst = nr.aggregate("EARLIEST_BY_OFFSET", 3, v, lst)
    assert lst == [1, 2, 3]
    lst = []
    for v in (None, 1, None, 2, 3, 4):
        lst = nr.aggregate("EARLIEST_BY_OFFSET_NULLS", 3, v, lst)
    assert lst == [None, 1, None]
    assert nr.aggregate("LATEST_BY_OFFSET", 1, 9, [8]) == [9] and nr.aggregate("EARLIEST_BY_OFFSET", 1, 9, [8]) == [8]
    nan = int(np.array([0xFFF4000000000123], np.uint64).view(np.int64)[0])  # a signalling NaN's bits stay what they are
    assert nr.col_bits(np.array([nan], np.int64).view(np.float64)) == [nan]


COMBOS = [(w, t, s, n) for w in nr.WINDOWS for t in ("INT64", "DOUBLE") for s, n in (("ignore", 3), ("keep", 2))]


@pytest.mark.parametrize("win,typ,shape,n", COMBOS)
def test_synthetic_expectation_covers(win, typ, shape, n):
    """The expectation of the GPU tests' synthetic streams (same seeds, same cutting): consistent with
    the oracle's COUNT(x) / COUNT(*) (asserted inside Expect for every snapshot) and covering the
    cases the resolve can get wrong."""
    s, per_push, pull, everything, classes = nr.expectation(win, typ, shape, n)
    assert len(per_push) == 7
    # per group and push: m = 0 on a resident non-empty list, 0 < m < N, m >= N
    assert classes["zero"] > 0 and classes["some"] > 0 and classes["full"] > 0, classes
    if win != "none":
        assert sum(st["windows_late"] for st, _, _ in per_push) > 0
        assert classes["same_push_closed"] > 0                      # a window updated and closed by one push
    assert sum(st["dropped_null_key"] + st["dropped_null_row"] + st["dropped_bad_ts"] for st, _, _ in per_push) > 0
    lat, ear = nr.lists_of(everything, 0), nr.lists_of(everything, 2 if shape == "ignore" else 1)
    assert any(len(x) == n for x in lat) and any(0 < len(x) < n for x in lat) or n == 1
    assert any(len(x) == n for x in ear)
    if shape == "keep":
        assert any(None in x for x in lat) and any(None in x for x in ear)
        assert any(x and x[0] is None for x in lat + ear) and any(x and x[-1] is None for x in lat + ear)
        assert any(x and all(v is None for v in x) for x in lat + ear)   # an all-NULL list
    elif win != "none":
        assert any(x == [] for x in lat)                                # a group whose arguments were all NULL
    for x, y in zip(lat, ear):
        assert (len(x) == 0) == (len(y) == 0)
    if typ == "DOUBLE":
        flat = [v for x in lat + ear for v in x if v is not None]
        assert any(v == -2**63 for v in flat)                           # -0.0
        assert any((v & 0x7FF0000000000000) == 0x7FF0000000000000 and (v & 0x000FFFFFFFFFFFFF) not in (0, 1 << 51)
                   for v in flat)                                       # a NaN that is not the canonical one
    assert pull[2]["n"] > 0
    # the changes of a push are not empty and carry arrays
    assert all(chg["n"] > 0 for _, _, chg in per_push[1:])


def test_cutting_does_not_matter():
    """One push and seven pushes of the same records: the same final table."""
    col_types, aggs, having = nr.query("INT64", "keep", 3)
    s, per_push, _, everything, _ = nr.expectation("tumb", "INT64", "keep", 3)
    e = nr.Expect(abi.load_oracle(), col_types, aggs, **nr.WINDOWS["tumb"])
    e.push(apps=nr.stream_applications("tumb"), **nr.tr.push_args(s, 0, nr.N_REC, 1))
    one = e.snapshot()
    e.close()
    nr.assert_same(one, per_push[-1][1], "one push")


def test_shared_query_expectation():
    s, per_push, pull, everything, _ = nr.expectation("hop", "INT32", "shared", 0)
    l2, l5, e3 = nr.lists_of(everything, 0), nr.lists_of(everything, 1), nr.lists_of(everything, 3)
    scalar, snull = everything["values"][2], everything["null_bytes"][2]
    assert any(len(x) == 5 for x in l5)
    for r in range(everything["n"]):
        assert l2[r] == l5[r][-2:]                                      # the last two of the last five
        assert (l5[r] == []) == bool(snull[r]) and (snull[r] or l5[r][-1] == int(scalar[r]))
        assert (not e3[r]) == (not l5[r])
    assert per_push[-1][1]["n"] < everything["n"]                       # the HAVING on COUNT(*) hides rows


def test_abi_array_helpers():
    K = abi.AGG_K
    assert abi.agg_is_array(abi.AGG["LATEST_BY_OFFSET"] | K(3)) and abi.agg_is_array(abi.AGG["EARLIEST_BY_OFFSET"] | K(1))
    assert abi.agg_is_array(abi.AGG["LATEST_BY_OFFSET_NULLS"] | K(2)) and abi.agg_is_array(abi.AGG["EARLIEST_BY_OFFSET_NULLS"] | K(5))
    for name in nr.NFORM:  # without k bits: the scalar forms
        assert not abi.agg_is_array(abi.AGG[name])
    assert abi.agg_is_array(abi.AGG["TOPK"] | K(3)) and not abi.agg_is_array(abi.AGG["MAX"])
    d = abi.make_agg_desc(col_types=["INT32", "DOUBLE"], aggs=[
        ("LATEST_BY_OFFSET", 0, 3), ("COUNT_STAR", -1), ("EARLIEST_BY_OFFSET_NULLS", 1, 5), ("LATEST_BY_OFFSET", 1),
        ("EARLIEST_BY_OFFSET", 0, 1), ("TOPK", 0, 2)])
    assert [d.aggs[i].kind for i in range(6)] == [6 | 3 << 16, 0, 7 | 0x100 | 5 << 16, 6, 7 | 1 << 16, 8 | 2 << 16]
    assert abi.agg_result_len(d) == [3, 1, 5, 1, 1, 2]
    assert [abi.agg_is_array(d.aggs[i].kind) for i in range(6)] == [True, False, True, False, True, True]
    assert abi.result_types(d) == [abi.TYPE["INT32"], abi.TYPE["INT64"], abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"],
                                   abi.TYPE["INT32"], abi.TYPE["INT32"]]
    assert (abi.NULL_PRESENT, abi.NULL_PAST_END, abi.NULL_ELEMENT) == (0, 1, 2)
    vals = np.array([[7, 0, 9, 0], [0, 0, 0, 0]], np.int64)
    nb = np.array([[0, 2, 0, 1], [1, 1, 1, 1]], np.uint8)
    assert abi.array_row(vals, nb, 0) == [7, None, 9] and abi.array_row(vals, nb, 1) == []


def test_header_matches_abi():
    text = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"(?m)^#define (KHIP_AGG_\w+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert defs["KHIP_AGG_LATEST_BY_OFFSET"] == abi.AGG["LATEST_BY_OFFSET"] == 6
    assert defs["KHIP_AGG_EARLIEST_BY_OFFSET"] == abi.AGG["EARLIEST_BY_OFFSET"] == 7
    assert defs["KHIP_AGG_KEEP_NULLS"] == abi.AGG_KEEP_NULLS
    assert re.search(r"(?m)^#define KHIP_AGG_K\(k\) \(\(int32_t\)\(k\) << 16\)$", text)
    assert re.search(r"(?m)^#define KHIP_ABI_VERSION 8$", text)
    flat = re.sub(r"[\s*]+", " ", text)
    for ref in ("LatestByOffset.java:149-218", "EarliestByOffset.java:162-228"):
        assert ref in flat
    # the N forms are routed, and the null byte 2 is documented at khip_snapshot
    assert "N forms (arrays) are never routed here" not in flat
    assert re.search(r"2 = a NULL element inside the list", flat)
    assert re.search(r"LATEST_BY_OFFSET\(col, N\[, ignoreNulls\]\)", flat)
