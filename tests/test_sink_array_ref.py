"""tests/sink_array_ref.py (the CPU restatement of a JSON value with ARRAY columns) pinned to the
reference's own output: the raw_value of every JSON-format case of qtt_topk.json and
qtt_offset_n.json, and hand-written edge cases.  No GPU: this pins the yardstick that
test_gpu_sink_array.py holds the device to.
"""
import json
import struct

import pytest

import sink_array_ref as ar

CASES = ar.json_cases()


def test_case_selection():
    names = [c["name"] for _, c in CASES]
    assert len(names) == 5 + 12, names  # topk: integer / long / double [JSON], two distinct; every N-form case
    assert all("AVRO" not in nm and "PROTOBUF" not in nm for nm in names)
    assert set(ar.PROJECTED_JSON) <= set(names)


@pytest.mark.parametrize("kind,case", CASES, ids=[c["name"] for _, c in CASES])
def test_restatement_parses_to_raw_value(kind, case):
    cols = ar.case_columns(case)
    checked = 0
    for o in case["outputs"]:
        if o["tombstone"]:
            continue
        b = ar.encode_value(cols, o["values"])
        assert b == b.strip() and b" " not in b  # compact
        ar.assert_parses_to(b, cols, o["raw_value"])
        checked += 1
    assert checked == len(case["outputs"]) > 0


def test_projected_cases_have_three_typed_columns():
    for _, c in CASES:
        if c["name"] in ar.PROJECTED_JSON:
            assert [(n, t) for n, t, _ in ar.case_columns(c)] == [("L0", "INT32"), ("L1", "INT64"), ("L2", "DOUBLE")]


def test_hand_written():
    nan_payload = struct.unpack("<d", struct.pack("<Q", 0x7FF8_0000_DEAD_BEEF))[0]
    cols = [("A", "INT64", 3), ("D", "DOUBLE", 4), ("S", "INT32")]
    assert ar.encode_value(cols, [[], [], 7]) == b'{"A":[],"D":[],"S":7}'
    assert ar.encode_value(cols, [[None], [None, 1.5], None]) == b'{"A":[null],"D":[null,1.5],"S":null}'
    assert ar.encode_value(cols, [[-2**63, 2**63 - 1, 0], [-0.0, 0.0], -1]) == \
        b'{"A":[-9223372036854775808,9223372036854775807,0],"D":[-0.0,0.0],"S":-1}'
    assert ar.encode_value(cols, [[1], [float("nan"), nan_payload, float("inf"), float("-inf")], 0]) == \
        b'{"A":[1],"D":["NaN","NaN","Infinity","-Infinity"],"S":0}'
    assert ar.encode_value(cols, [[1], [5e-324, 1e7, 1e-3, 123456.789], 0]) == \
        b'{"A":[1],"D":[4.9E-324,1.0E7,0.001,123456.789],"S":0}'
    assert ar.encode_value([('q"\n', "INT32", 1)], [[5]]) == b'{"q\\"\\n":[5]}'
    assert ar.encode_value(cols, [[1], [2.0], 3], tombstone=True) is None
    assert json.loads(ar.encode_value(cols, [[1, None, 3], [], 9])) == {"A": [1, None, 3], "D": [], "S": 9}


def test_row_list_and_pack_round_trip():
    lists = [[], [4], [None, 5, None], [1, 2, 3]]
    vals, nb = ar.pack_lists(lists, 3, "INT64")
    assert nb.tolist() == [[1, 1, 1], [0, 1, 1], [2, 0, 2], [0, 0, 0]]
    assert [ar.row_list(vals, nb, r, "INT64") for r in range(4)] == lists
    # a list ends at the first byte that is neither 0 nor 2, whatever follows it
    nb[1] = [0, 1, 0]
    assert ar.row_list(vals, nb, 1, "INT64") == [4]
