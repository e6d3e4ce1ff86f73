"""LATEST_BY_OFFSET / EARLIEST_BY_OFFSET without a GPU: the extracted QTT cases, the two reference
models the GPU tests compare against (tests/offset_ref.py), and the interface constants.

The cases of tests/golden/qtt_offset.json (make_offset_fixtures.py; the non-SESSION scalar forms
of the reference's latest-offset-udaf.json and earliest-offset-udaf.json):
  latest by offset (projected), nulls ignored - single, nulls not ignored - single,
  latest by offset with all nulls, earliest by offset (projected),
  null first - single - ignoring nulls, null first - single - not ignoring nulls,
  nulls later - single - nulls ignored, null later - single - nulls not ignored,
  earliest by offset with all nulls.
"""
import os
import re

import pytest

import offset_ref
import qtt
from ksql_amd import abi

CASES = qtt.load_cases("offset")
IDS = [c["name"] for c in CASES]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extracted_cases():
    assert len(CASES) == 10
    assert sorted(IDS) == sorted([
        "latest by offset (projected)", "nulls ignored - single", "nulls not ignored - single",
        "latest by offset with all nulls", "earliest by offset (projected)",
        "null first - single - ignoring nulls", "null first - single - not ignoring nulls",
        "nulls later - single - nulls ignored", "null later - single - nulls not ignored",
        "earliest by offset with all nulls"])
    for c in CASES:
        assert c["desc"]["window_kind"] == "NONE" and c["outputs"] and c["input"]
        assert all(a["kind"] in offset_ref.OFFSET for a in c["desc"]["aggs"])
    proj = [c for c in CASES if c["name"].endswith("(projected)")]
    assert [c["desc"]["col_types"] for c in proj] == [["INT32", "INT64", "DOUBLE"]] * 2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_record_rules_reproduce_qtt(case):
    """The per-record aggregate() rules give every expected output record, and the final table."""
    rows = offset_ref.run_case(case)
    assert qtt.compare_outputs(case, rows) == []
    assert qtt.compare_agg(case, qtt.fold(rows)) == []


@pytest.mark.parametrize("split", [None, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_expectation_reproduces_qtt(case, split):
    """MAX / MIN of the sequence column through the oracle, translated back to values: the expected
    final table as one batch and as 1-row pushes, and with 1-row pushes every output record."""
    orc = abi.load_oracle()
    snap, rows = offset_ref.case_expect(orc, case, split, changelog=True)
    assert qtt.compare_agg(case, snap) == []
    assert qtt.compare_agg(case, qtt.fold(rows)) == []
    if split == 1:
        assert qtt.compare_outputs(case, rows) == []


def test_abi_names_and_result_types():
    assert abi.AGG["LATEST_BY_OFFSET"] == 6 and abi.AGG["EARLIEST_BY_OFFSET"] == 7
    assert abi.AGG_KEEP_NULLS == 0x100
    assert abi.AGG["LATEST_BY_OFFSET_NULLS"] == 6 | 0x100
    assert abi.AGG["EARLIEST_BY_OFFSET_NULLS"] == 7 | 0x100
    assert {k: v for k, v in abi.AGG.items() if v < 6} == {"COUNT_STAR": 0, "COUNT": 1, "SUM": 2, "MIN": 3, "MAX": 4,
                                                            "AVG": 5}
    d = abi.make_agg_desc(col_types=["INT32", "INT64", "DOUBLE"],
                          aggs=[("LATEST_BY_OFFSET", 0), ("EARLIEST_BY_OFFSET_NULLS", 1), ("LATEST_BY_OFFSET_NULLS", 2),
                                ("COUNT_STAR", -1), ("EARLIEST_BY_OFFSET", 2)])
    assert [d.aggs[i].kind for i in range(5)] == [6, 7 | 0x100, 6 | 0x100, 0, 7]
    assert abi.result_types(d) == [abi.TYPE["INT32"], abi.TYPE["INT64"], abi.TYPE["DOUBLE"], abi.TYPE["INT64"],
                                   abi.TYPE["DOUBLE"]]


def test_header_defines_match_abi():
    text = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"(?m)^#define (KHIP_AGG_\w+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert defs["KHIP_AGG_LATEST_BY_OFFSET"] == abi.AGG["LATEST_BY_OFFSET"]
    assert defs["KHIP_AGG_EARLIEST_BY_OFFSET"] == abi.AGG["EARLIEST_BY_OFFSET"]
    assert defs["KHIP_AGG_KEEP_NULLS"] == abi.AGG_KEEP_NULLS
    assert re.search(r"(?m)^#define KHIP_ABI_VERSION 8$", text)
    for ref in ("LatestByOffset.java:87-146", "EarliestByOffset.java:85-158", "KudafByOffsetUtils.java:77-104"):
        assert ref in text
