"""The CPU deserializer restatement (tests/serde_ref.py) on known answers: Jackson's BigDecimal
intValue() / longValue() for JSON float tokens into INT / BIGINT columns
(KsqlJsonDeserializer.java:68-70, JsonSerdeUtils.java:95-121)."""
import json
import os

import pytest

import format_cases as fc
import serde_ref


def test_bigdecimal_low_bits():
    b = serde_ref.bigdec_low_bits
    assert b("3000000000.5", 32) == 3000000000 - (1 << 32)
    assert b("1e20", 64) == 10 ** 20 - 5 * (1 << 64)
    assert b("-1e20", 64) == -(10 ** 20 - 5 * (1 << 64))
    assert b("9007199254740993.7", 64) == 9007199254740993  # a double would give ...992
    assert b("1e400", 32) == 0 and b("1e400", 64) == 0  # 10^400 is a multiple of 2^64
    assert b("-2.9", 32) == -2 and b("12.5e-1", 64) == 1 and b("0.5e1", 64) == 5 and b("1e-5", 64) == 0


def test_json_decimal_tokens_decode():
    fields = [("A", "INT32", 0), ("B", "INT64", 1), ("C", "DOUBLE", 2)]
    out, err = serde_ref.decode("JSON", fields, "INT64", [b"\0" * 8],
                                [b'{"A": 3000000000.5, "B": 1e20, "C": 3000000000.5}'])
    assert err == 0
    row = out[0][3]
    assert row == {"A": -1294967296, "B": 7766279631452241920, "C": 3000000000.5}


# ---- delimiters other than ',' (the reference's own QTT cases, tests/golden/delimited_delimiters.json)

DELIM_CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                          "delimited_delimiters.json")))["cases"]


def delimiter_case_expected(case):
    """The numbers the reference expects out of a fixture case (a SELECT of every column): its expected
    output text split at the output delimiter (no field of the fixture is quoted); NAME only as non-NULL."""
    rows = []
    for text in case["outputs"]:
        parts = text.split(case["delimiter_out"])
        assert len(parts) == len(case["columns"])
        rows.append({n: (True if t == "STRING" else int(p)) for (n, t), p in zip(case["columns"], parts)})
    return rows


def test_fixture_covers_the_delimiters():
    assert [(c["delimiter_in"], c["delimiter_out"]) for c in DELIM_CASES] == [
        ("-", "-"), ("|", "|"), ("|", "$"), (" ", " "), ("\t", "\t")]


@pytest.mark.parametrize("case", DELIM_CASES, ids=[c["name"][:60] for c in DELIM_CASES])
def test_fixture_inputs_decode_with_their_delimiter(case):
    fields = [(n, t, i) for i, (n, t) in enumerate(case["columns"])]
    vals = [v.encode() for v in case["inputs"]]
    exp, nerr = serde_ref.decode("DELIMITED", fields, "INT64", [b"\0" * 8] * len(vals), vals, case["delimiter_in"])
    assert nerr == 0
    for (kv, key, rv, row), want in zip(exp, delimiter_case_expected(case)):
        assert kv and rv
        for (n, t) in case["columns"]:
            assert (row[n] is not None) if t == "STRING" else row[n] == want[n], (n, row, want)
    # with ',' the same bytes are one field: an arity error (two columns or more)
    assert serde_ref.decode("DELIMITED", fields, "INT64", [b"\0" * 8] * len(vals), vals)[1] == len(vals)


@pytest.mark.parametrize("case", fc.DECODE_CASES, ids=[c["id"] for c in fc.DECODE_CASES])
def test_random_cases_are_balanced(case):
    """Every seeded case of the GPU decode tests: 5 % to 25 % failed records and both NULL and
    non-NULL rows in every output column, by the reference alone."""
    fc.check_shares(fc.case_reference(case), case["fields"])


def test_halfway_texts_round_as_python_does():
    """The generator's own claims: the midpoint text is exact (ties to even: to x or its neighbour by
    the parity of x's last bit), one digit up rounds away from zero and one down toward zero; at most
    768 significant digits and 1077 characters (the decoder's big integers are sized for 800 digits)."""
    for x in fc.HALFWAY_FIXED + [-v for v in fc.HALFWAY_FIXED] + [1.5, 3e-310, -7.25e200]:
        mid, up, down = fc.halfway_texts(x)
        ax = abs(x)
        nxt = fc.from_bits(fc.bits_of(ax) + 1)
        sign = -1.0 if str(mid).startswith("-") else 1.0
        assert fc.same_double(float(down), sign * ax) and fc.same_double(float(up), sign * nxt)
        assert fc.same_double(float(mid), sign * (nxt if fc.bits_of(ax) & 1 else ax))
    pool = fc.halfway_pool()
    assert max(len(t) for t, _ in pool) <= 1077 + 1 and max(fc.significant_digits(t) for t, _ in pool) <= 768
    assert min(fc.significant_digits(t) for t, _ in pool) > 19
    assert sorted(t for t, _ in pool if not fc.tail_nonzero(t)) == ["-1" + "0" * 23, "1" + "0" * 23]
    assert any(v == float("inf") for _, v in pool) and any(v == 0.0 for _, v in pool)


@pytest.mark.parametrize("fmt", ["DELIMITED", "JSON"])
def test_deferred_batches_reference(fmt):
    """serde_ref on the deferred-double batches: only the "fail" records fail, and the halfway texts
    come back as Python rounds them."""
    keys, vals = fc.mixed_batch(fmt, 65)
    exp, nerr = serde_ref.decode(fmt, fc.DEFER_FIELDS, "INT64", keys, vals)
    assert nerr == 13 and [i for i, r in enumerate(exp) if not r[2]] == list(range(1, 65, 5))
    keys, vals = fc.grow_batch(fmt)
    assert serde_ref.decode(fmt, fc.DEFER_FIELDS, "INT64", keys, vals)[1] == 0
