"""TOPK / TOPKDISTINCT without a GPU: the extracted QTT cases, the reference models the GPU tests
compare against (tests/topk_ref.py), that their random expectations are not vacuous, and the
interface constants.

The cases of tests/golden/qtt_topk.json (make_topk_fixtures.py): "topk integer", "topk long",
"topk double" of topk-group-by.json in the AVRO, JSON, PROTOBUF and PROTOBUF_NOSR formats, and
"topk distinct integer", "topk distinct long" of topk-distinct.json.
"""
import os
import re

import numpy as np
import pytest

import qtt
import topk_ref as tr
from ksql_amd import abi

CASES = qtt.load_cases("topk")
IDS = [c["name"] for c in CASES]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extracted_cases():
    base = sorted({re.sub(r" \[\w+\]$", "", n) for n in IDS})
    assert base == ["topk distinct integer", "topk distinct long", "topk double", "topk integer", "topk long"]
    assert len(CASES) == 3 * 4 + 2
    for c in CASES:
        d = c["desc"]
        assert d["window_kind"] == "NONE" and c["outputs"] and c["input"] and len(c["outputs"]) == len(c["input"])
        assert [(a["kind"] in tr.TOPK, a["k"]) for a in d["aggs"]] == [(True, 3)]
        assert all(isinstance(o["values"][0], list) for o in c["outputs"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_qtt(case):
    """aggregate() record by record gives every expected output record (the final table with it)."""
    assert tr.model_outputs(case) == tr.golden_outputs(case)


def test_distinct_integer_repeats_an_unchanged_row():
    """"topk distinct integer" emits a row equal to the one before it (a duplicate value changes
    nothing, the record is forwarded all the same): the GPU output-sequence test must see it."""
    c = next(c for c in CASES if c["name"] == "topk distinct integer")
    out = tr.golden_outputs(c)
    assert any(out[i] == out[i - 1] for i in range(1, len(out)))


def test_java_order():
    nan, nan2 = tr.uncanon(0x7FF8000000000000, "DOUBLE"), tr.uncanon(-0x000BFFFFFFFFFEDD, "DOUBLE")
    assert nan2 != nan2 and tr.canon(nan, "DOUBLE") == tr.canon(nan2, "DOUBLE")  # every NaN is one value
    order = [float("-inf"), -1.0, -0.0, 0.0, 5e-324, 1.0, float("inf"), nan]
    assert all(tr.compare_to(a, b, "DOUBLE") < 0 for a, b in zip(order, order[1:]))
    assert tr.canon(-0.0, "DOUBLE") != tr.canon(0.0, "DOUBLE")
    lst = tr.aggregate("TOPKDISTINCT", 3, "DOUBLE", nan2, tr.aggregate("TOPKDISTINCT", 3, "DOUBLE", nan, [1.0]))
    assert tr.canon_list(lst, "DOUBLE") == [0x7FF8000000000000, tr.canon(1.0, "DOUBLE")]
    lst = []
    for v in (0.0, -0.0, 0.0, -0.0):
        tr.aggregate("TOPKDISTINCT", 3, "DOUBLE", v, lst)
    assert tr.canon_list(lst, "DOUBLE") == [0, -2**63]
    lst = []
    for v in (5, 5, None, 7, 5, 1):
        tr.aggregate("TOPK", 3, "INT32", v, lst)
    assert lst == [7, 5, 5]  # an equal value does not displace the last element of a full list


@pytest.mark.parametrize("typ", tr.TYPES)
@pytest.mark.parametrize("win", list(tr.WINDOWS))
def test_random_expectation_not_vacuous(win, typ):
    """The expectation of the GPU tests' random streams (same seeds, same cutting): consistent with
    the oracle's MAX(x) / COUNT(x) (asserted inside Expect for every snapshot) and covering the
    cases the lists can get wrong."""
    s, per_push, pull, everything, stats = tr.expectation(win, typ, "beside")
    col_types, aggs, having = tr.query(typ, "beside")
    assert sum(st["windows_late"] for st, _, _ in per_push) > 0 or win == "none"
    assert win == "none" or sum(st["windows_late"] for st, _, _ in per_push) > 0  # late-dropped records
    assert sum(st["dropped_null_key"] + st["dropped_null_row"] + st["dropped_bad_ts"] for st, _, _ in per_push) > 0
    n = everything["n"]
    assert n > 250
    t3 = tr.lists_of(everything, 1, typ)   # TOPK(x, 3)
    d3 = tr.lists_of(everything, 3, typ)   # TOPKDISTINCT(x, 3)
    t8 = tr.lists_of(everything, 5, typ)   # TOPK(x, 8)
    # TOPK against the oracle's MAX(x) / COUNT(x) (Expect checked it per row; once more in the open)
    orc_h = tr.Expect(abi.load_oracle(), col_types, aggs, **tr.WINDOWS[win])
    orc_h.push(apps=tr.stream_applications(win), **tr.push_args(s, 0, tr.N, len(col_types)))
    raw = orc_h.h.snapshot()
    orc_h.close()
    if win == "none":  # (a windowed one-push table has lost its expired windows: compare where nothing expires)
        assert raw["n"] == n
        for r in range(n):
            cnt = int(raw["values"][orc_h.cnt_at[1]][r])
            assert len(t3[r]) == min(cnt, 3) and len(t8[r]) == min(cnt, 8)
            assert (not t3[r] and raw["nulls"][1][r]) or t3[r][0] == tr.canon(raw["values"][1][r].item(), typ)
    assert sum(len(x) == 3 for x in t3) * 2 >= n                      # at least half of the groups: a full list
    if win != "none":
        assert any(0 < len(x) < 3 for x in t3)                        # a partly filled list
    assert any(0 < len(x) < 8 for x in t8) or win == "none"
    assert any(len(x) == 0 for x in t3) or win == "none"              # a group whose arguments were all NULL
    assert any(a == b for x in t3 for a, b in zip(x, x[1:]))          # TOPK keeps duplicates
    assert all(len(set(x)) == len(x) for x in d3)
    assert stats["dup_seen"] > 0                                      # TOPKDISTINCT saw a value it holds
    for x, y in zip(t3, d3):                                          # descending, and the same head
        assert x == sorted(x, key=lambda c: tr.jkey(tr.uncanon(c, typ), typ), reverse=True)
        assert x[:1] == y[:1]
    if typ == "INT64":
        assert any(tr.I64_MAX in x for x in d3)
        if win != "none":  # (an unwindowed group holds ~45 values: Long.MIN_VALUE is never among its top 8)
            assert any(tr.I64_MIN in x for x in t3) and any(tr.I64_MIN in x for x in d3)
    if typ == "DOUBLE":
        assert any(tr.NAN_BITS in x for x in t3)
        if win != "none":  # -0.0 and 0.0 are two values
            assert any(-2**63 in x for x in d3) and any(0 in x for x in d3)
    # the HAVING on COUNT(*) hides rows from the final snapshot and emits tombstones on the way
    assert per_push[-1][1]["n"] < n or win == "none"
    assert pull[2]["n"] > 0


def test_all_null_group_exists():
    """Windowed streams have groups with no non-NULL argument: [] (not SQL NULL) in the layout."""
    _, _, _, everything, _ = tr.expectation("tumb", "INT32", "TOPK")
    empty = [r for r in range(everything["n"]) if everything["nulls"][0][r].all()]
    assert empty and everything["values"][0].shape == (everything["n"], 3)


def test_abi_names_and_spec_form():
    assert abi.AGG["TOPK"] == 8 and abi.AGG["TOPKDISTINCT"] == 9 and abi.AGG_K(3) == 3 << 16
    d = abi.make_agg_desc(col_types=["INT32", "DOUBLE"], aggs=[("TOPK", 0, 3), ("COUNT_STAR", -1), ("TOPKDISTINCT", 1, 8),
                                                              ("MAX", 1)])
    assert [d.aggs[i].kind for i in range(4)] == [8 | 3 << 16, 0, 9 | 8 << 16, 4]
    assert abi.result_types(d) == [abi.TYPE["INT32"], abi.TYPE["INT64"], abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"]]
    assert abi.agg_result_len(d) == [3, 1, 8, 1]
    assert "agg_result_len" in abi.PRODUCT_ONLY


def test_header_defines_match_abi():
    text = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"(?m)^#define (KHIP_AGG_\w+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert defs["KHIP_AGG_TOPK"] == abi.AGG["TOPK"] and defs["KHIP_AGG_TOPKDISTINCT"] == abi.AGG["TOPKDISTINCT"]
    assert re.search(r"(?m)^#define KHIP_AGG_K\(k\) \(\(int32_t\)\(k\) << 16\)$", text)
    assert re.search(r"(?m)^#define KHIP_ABI_VERSION 8$", text)
    assert re.search(r"khip_status khip_agg_result_len\(const khip_agg_desc\* desc, int32_t agg_index,\s+int32_t\* out_len\);", text)
    for ref in ("TopkKudaf.java:119-142", "TopkDistinctKudaf.java:130-153", "TopkKudaf.java:104-110"):
        assert ref in text
