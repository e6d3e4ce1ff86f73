"""The sink serializers' CPU restatement (tests/sink_ref.py) pinned independently:
Double.toString digits against Python's shortest round-trip repr (which agrees with the JDK 19+
specification except where Java prefers a closer two-digit decimal for the smallest subnormals,
e.g. Double.MIN_VALUE = "4.9E-324"), the layout switches at 1e-3 and 1e7, and the key / value
formats on hand-written examples taken from the QTT expected records."""
import json
import math
import os
import random
import struct

import pytest

import sink_ref


def test_schubfach_matches_shortest_repr():
    rng = random.Random(3)
    n = bad = 0
    for _ in range(60000):
        v = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if math.isnan(v) or abs(v) < 1e-320:
            continue
        n += 1
        bad += sink_ref.java_double_str(v) != sink_ref.python_java_str(v)
    for _ in range(60000):
        v = float("%de%d" % (rng.randint(1, 10 ** rng.randint(1, 17)), rng.randint(-300, 300)))
        n += 1
        bad += sink_ref.java_double_str(v) != sink_ref.python_java_str(v)
    assert n > 100000 and bad == 0


def test_java_layout_examples():
    cases = [(1.0, "1.0"), (-0.0, "-0.0"), (0.0, "0.0"), (100.0, "100.0")]
    cases += list({0.1: "0.1", 0.001: "0.001",
             9.999e-4: "9.999E-4", 1e7: "1.0E7", 9999999.0: "9999999.0", 1.5e-7: "1.5E-7",
             123456.789: "123456.789", 1.0 / 3: "0.3333333333333333", 2.0 ** 63: "9.223372036854776E18",
             5e-324: "4.9E-324", 1.7976931348623157e308: "1.7976931348623157E308",
             float("nan"): "NaN", float("inf"): "Infinity", float("-inf"): "-Infinity"}.items())
    for v, s in cases:
        assert sink_ref.java_double_str(v) == s, (v, sink_ref.java_double_str(v), s)


def test_formats():
    assert sink_ref.encode_key("KAFKA", [("K", "INT64")], [1]) == b"\0" * 7 + b"\1"
    assert sink_ref.encode_key("KAFKA", [("K", "INT32")], [-1]) == b"\xff" * 4
    assert sink_ref.encode_key("JSON", [("K", "INT32"), ("K2", "INT32")], [1, 2]) == b'{"K":1,"K2":2}'
    assert sink_ref.encode_key("JSON", [("K", "STRING")], ['a"b']) == b'"a\\"b"'
    assert sink_ref.encode_key("DELIMITED", [("A", "STRING"), ("B", "INT32")], ["x,y", 3]) == b'"x,y",3'
    assert sink_ref.window_suffix("TUMBLING", 5, 10) == struct.pack(">q", 5)
    assert sink_ref.window_suffix("SESSION", 5, 10) == struct.pack(">qq", 10, 5)
    assert sink_ref.encode_value("JSON", [("COUNT", "INT64"), ("A", "DOUBLE")], [3, None]) == b'{"COUNT":3,"A":null}'
    assert sink_ref.encode_value("JSON", [("A", "DOUBLE")], [float("nan")]) == b'{"A":"NaN"}'
    assert sink_ref.encode_value("DELIMITED", [("A", "INT64"), ("B", "DOUBLE")], [None, 2.5]) == b",2.5"
    assert sink_ref.encode_value("DELIMITED", [("A", "INT64")], [1], tombstone=True) is None
    # commons-csv 1.4 MINIMAL: first-field RFC 4180 TEXTDATA rule, leading <= '#', trailing <= ' '
    assert sink_ref.csv_field("STRING", "") == '""'
    assert sink_ref.csv_field("STRING", "#x") == '"#x"'
    assert sink_ref.csv_field("STRING", "x ") == '"x "'
    assert sink_ref.csv_field("STRING", 'a"b') == '"a""b"'


# ---- delimiters other than ','

DELIM_CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                          "delimited_delimiters.json")))["cases"]


def test_fixture_all_numeric_output_with_its_delimiter():
    """The reference's "0-1" (two INT columns, value_delimiter '-'), and the other cases' outputs from
    their input fields: joined with the output delimiter, nothing quoted."""
    case = DELIM_CASES[0]
    assert case["delimiter_out"] == "-" and case["outputs"] == ["0-1"]
    cols = [tuple(c) for c in case["columns"]]
    assert sink_ref.encode_value("DELIMITED", cols, [0, 1], delim="-") == b"0-1"
    assert sink_ref.encode_key("DELIMITED", cols, [0, 1], delim="-") == b"0-1"
    for case in DELIM_CASES[1:]:
        cols = [tuple(c) for c in case["columns"]]
        for text, want in zip(case["inputs"], case["outputs"]):
            vals = [p if t == "STRING" else int(p) for (n, t), p in zip(cols, text.split(case["delimiter_in"]))]
            assert sink_ref.encode_value("DELIMITED", cols, vals, delim=case["delimiter_out"]) == want.encode()


# (type, value, printed text) and per delimiter the texts commons-csv's MINIMAL rule quotes: the ones
# holding the delimiter.  A digit, '-', '.', 'E', 'I' and 'N' are all above '#', no text ends <= ' ',
# so nothing else about a printed number asks for quotes.
QUOTING_NUMBERS = [("INT32", -5, "-5"), ("INT64", 100, "100"), ("INT64", 7, "7"), ("DOUBLE", 1.5, "1.5"),
                   ("DOUBLE", -2.25, "-2.25"), ("DOUBLE", 1.0e10, "1.0E10"), ("DOUBLE", float("nan"), "NaN"),
                   ("DOUBLE", float("inf"), "Infinity"), ("DOUBLE", float("-inf"), "-Infinity")]
QUOTED_UNDER = {"-": {"-5", "-2.25", "-Infinity"}, ".": {"1.5", "-2.25", "1.0E10"}, "E": {"1.0E10"},
                "0": {"100", "1.0E10"}, "\t": set(), " ": set(), ",": set(), "|": set()}


@pytest.mark.parametrize("delim", list(QUOTED_UNDER), ids=[repr(d) for d in QUOTED_UNDER])
def test_number_quoting_by_delimiter(delim):
    for first in (True, False):
        for typ, v, text in QUOTING_NUMBERS:
            want = '"%s"' % text if text in QUOTED_UNDER[delim] else text
            assert sink_ref.csv_field(typ, v, first, delim) == want, (typ, v, first)
    cols = [(str(i), t) for i, (t, _, _) in enumerate(QUOTING_NUMBERS)]
    want = delim.join('"%s"' % x if x in QUOTED_UNDER[delim] else x for _, _, x in QUOTING_NUMBERS).encode()
    assert sink_ref.encode_value("DELIMITED", cols, [v for _, v, _ in QUOTING_NUMBERS], delim=delim) == want
