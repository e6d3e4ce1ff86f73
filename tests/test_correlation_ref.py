"""tests/correlation_ref.py on the CPU: the restated fold and the exact model against the
reference's QTT goldens (bit for bit), model == fold inside the exact domain, the model within
5 * 2^-53 of the true coefficient everywhere, the undo path, the edges, and a guard that the
expectations the GPU tests use are not vacuous.  CPU only."""
import math
import os
import random
import re

import numpy as np
import pytest

import correlation_ref as cr
import qtt
import topk_ref as tr
from ksql_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("correlation")
IDS = [c["name"] for c in CASES]
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def test_fixture_cases():
    assert IDS == ["correlation int", "correlation long"]
    assert [c["desc"]["col_types"] for c in CASES] == [["INT32", "INT32"], ["INT64", "INT64"]]
    for c in CASES:
        assert c["desc"]["aggs"] == [{"kind": "CORRELATION", "arg_col": 0, "arg_col2": 1}]
        assert c["desc"]["key_type"] == "UTF8" and len(c["input"]) == len(c["outputs"]) == 7
        assert sum(r["cols"][0] is None for r in c["input"]) == 1 and sum(r["cols"][1] is None for r in c["input"]) == 1
        assert sum(o["values"][0] != o["values"][0] for o in c["outputs"]) == 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_reproduces_goldens_bit_for_bit(case):
    for (key, recs), o in zip(cr.case_sequences(case), case["outputs"]):
        assert key == o["key"] and not o["tombstone"]
        assert cr.same(cr.fold(recs), o["values"][0]), (key, recs, cr.fold(recs), o["values"][0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_equals_goldens_bit_for_bit(case):
    for (key, recs), o in zip(cr.case_sequences(case), case["outputs"]):
        pairs = cr.pairs_of(recs)
        assert cr.exact_domain(pairs)
        got = cr.model(pairs)
        assert cr.same(got, o["values"][0]), (key, recs, got, o["values"][0])
        assert got == got or cr.bits(got) == cr.NAN_BITS


def _exact_group(rng, g):
    n = rng.choice([2, 3, 4, 5, 8, 17, 64]) if g % 4 else rng.randint(100, 1 << 10)
    b = rng.randint(1, 15)
    slope = rng.choice([0, 1, -1, 2])
    pairs = []
    for _ in range(n):
        x = rng.randint(-(1 << b), 1 << b)
        y = max(-(1 << 15), min(1 << 15, slope * x + rng.randint(-(1 << (b // 2)), 1 << (b // 2)))) if slope else rng.randint(-(1 << b), 1 << b)
        pairs.append((x, y))
    return pairs


def test_model_equals_fold_in_the_exact_domain():
    """|x|, |y| <= 2^15 and n <= 2^10: every drawn group is inside the exact domain (asserted: none is
    discarded), so the reference's doubles are the integers and the two agree bit for bit, in any
    record order."""
    rng = random.Random(31)
    groups = nans = 0
    for g in range(600):
        pairs = _exact_group(rng, g) if g % 25 else [(rng.randint(-9, 9), 7) for _ in range(6)]  # (a constant y: NaN)
        assert cr.exact_domain(pairs), pairs[:4]
        m = cr.model(pairs)
        assert cr.same(m, cr.fold(pairs)), (pairs[:6], len(pairs), m, cr.fold(pairs))
        shuffled = pairs[:]
        rng.shuffle(shuffled)
        assert cr.same(m, cr.fold(shuffled))
        groups += 1
        nans += m != m
    assert groups == 600 and 0 < nans < 100


def test_exact_domain_predicate():
    assert cr.exact_domain([(1 << 15, -(1 << 15))] * (1 << 10))
    assert not cr.exact_domain([(1 << 26, 1 << 26), (1, 1)])  # x² sums to 2^52 + 1, n * that passes 2^53
    assert not cr.exact_domain([(I64_MAX, 1), (0, 0)])


def _rel_err(pairs):
    """|model - true| / |true| as an exact-enough rational: the true coefficient to 120 digits."""
    t = cr.true_coefficient(pairs)
    m = cr.model(pairs)
    if t is None:
        assert m != m
        return None
    assert m == m
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 120
        return abs((decimal.Decimal(m) - t) / t) if t != 0 else (decimal.Decimal(0) if m == 0.0 else decimal.Decimal(1))


@pytest.mark.parametrize("typ", cr.TYPES)
def test_model_within_5u_of_the_true_coefficient(typ):
    """Random INT / BIGINT groups, full-range values and the extremes among them: the model is within
    5 * 2^-53 relative of the Pearson coefficient (computed from exact integers with a 120-digit
    decimal square root, about 400 bits)."""
    rng = random.Random(41 if typ == "INT32" else 42)
    lo, hi = (-2**31, 2**31 - 1) if typ == "INT32" else (I64_MIN, I64_MAX)
    worst, checked = 0.0, 0
    for g in range(400):
        n = rng.choice([2, 3, 4, 5, 8, 17, 64, 300])
        b = rng.randint(1, 31 if typ == "INT32" else 63)
        slope = rng.choice([0, 1, -1, 3])

        def val():
            return rng.choice([lo, hi, 0, -1]) if rng.random() < 0.2 else (
                rng.randint(lo, hi) if g % 3 == 0 else rng.randint(-(1 << b), (1 << b) - 1))
        pairs = []
        for _ in range(n):
            x = val()
            pairs.append((x, max(lo, min(hi, slope * x + rng.randint(-(1 << (b // 2)), 1 << (b // 2)))) if slope else val()))
        e = _rel_err(pairs)
        if e is None:
            continue
        assert e <= 5 * cr.U, (typ, pairs[:4], n, float(e) / cr.U)
        worst = max(worst, float(e) / cr.U)
        checked += 1
    assert checked > 380
    print("worst |model - true| / (u |true|) = %.3f" % worst)


def test_undo_equals_the_model_of_the_remainder():
    """A table source: rows enter and leave a group.  The state is additive, so the words after
    undos are the remainder's: the model over the running integer state equals the model of the
    remaining rows, bit for bit; a group emptied again is NaN."""
    rng = random.Random(51)
    emptied = 0
    for g in range(200):
        w, live = [0] * 6, []
        big = g % 2
        for _ in range(rng.randint(5, 200)):
            if live and rng.random() < 0.4:
                x, y = live.pop(rng.randrange(len(live)))
                sign = -1
            else:
                x = rng.choice([I64_MIN, I64_MAX, 0]) if big and rng.random() < 0.3 else rng.randint(-1000, 1000)
                y = rng.choice([None, rng.randint(-50, 50), 3 * x + rng.randint(-5, 5)])
                live.append((x, y))
                sign = 1
            if x is not None and y is not None:
                for i, v in enumerate((1, x, y, x * x, y * y, x * y)):
                    w[i] += sign * v
        if g % 10 == 0:
            while live:
                x, y = live.pop()
                if y is not None:
                    for i, v in enumerate((1, x, y, x * x, y * y, x * y)):
                        w[i] -= v
            emptied += 1
            assert w == [0] * 6 and cr.bits(cr.model_state(*w)) == cr.NAN_BITS
        assert cr.bits(cr.model_state(*w)) == cr.bits(cr.model(cr.pairs_of(live)))
    assert emptied == 20


def test_fold_undo_restated():
    f = cr.Fold()
    for x, y in [(1, 8), (-1, -2), (5, None), (None, 3), (-4, -1)]:
        f.aggregate(x, y)
    assert f.count == 3 and f.map() == 0.7455284088780169
    f.undo(-4, -1)
    f.undo(5, None)
    assert f.count == 2 and f.map() == 1.0
    f.undo(1, 8)
    f.undo(-1, -2)
    assert f.count == 0 and f.map() != f.map()


def test_model_edges():
    for pairs in ([], [(5, 7)], [(I64_MIN, I64_MAX)], [(3, 1), (3, 2), (3, 9)], [(1, 4), (2, 4), (-7, 4)], [(2, 2)] * 1000):
        assert cr.bits(cr.model(pairs)) == cr.NAN_BITS, pairs[:3]
    assert cr.model([(x, x) for x in (1, 5, -9, 12)]) == 1.0
    assert cr.model([(x, x) for x in (I64_MIN, I64_MAX, 0, 2**40)]) == 1.0
    assert cr.model([(x, -x) for x in (1, 5, -9, 12)]) == -1.0
    assert cr.model([(1, 8), (-1, -2), (-4, -1)]) == 0.7455284088780169
    assert math.isnan(cr.NAN) and cr.bits(cr.NAN) == 0x7FF8000000000000
    # the reference squares Long::doubleValue, rounded beyond 2^53; the model does not
    big = [(2**62 + 1, 1), (2**62 + 3, 2), (2**62 + 5, 4)]
    assert abs(cr.model(big) - cr.model([(1, 1), (3, 2), (5, 4)])) < 1e-15  # (r does not change under a shift)
    assert not cr.same(cr.model(big), cr.fold(big))


@pytest.mark.parametrize("typ", cr.TYPES)
@pytest.mark.parametrize("win", list(tr.WINDOWS))
def test_gpu_expectations_are_not_vacuous(win, typ):
    """What tests/test_gpu_correlation.py compares against: groups with n = 0, 1, 2 and >= 1000 pairs
    (the thousand in the unwindowed stream, whose hot group nothing expires), NaN and finite results,
    positive and negative r, a group where COUNT(x), COUNT(y) and the pair count all differ, the
    HAVING hides rows, the pull query returns rows, the extremes are in."""
    s, per_push, pull, everything, stats = cr.expectation(win, typ, "beside")
    assert all(stats[k] > 0 for k in ("n0", "n1", "n2", "nan", "finite", "pos", "neg", "counts_differ")), stats
    assert stats["n1000"] > 0 or win != "none", stats
    assert per_push[0][1]["n"] == 0 and per_push[0][0]["windows_applied"] <= 3  # the first record alone: hidden
    assert pull[2]["n"] > 0
    assert not everything["nulls"][1].any()
    for c in (0, 1):
        v = s["cols"][c][s["col_valid"][c]]
        assert v.min() == tr.pool(typ).min() and v.max() == tr.pool(typ).max()
        assert 0.25 < 1 - s["col_valid"][c].mean() < 0.35
    # NaNs of the expectation are the canonical quiet NaN
    v = everything["values"][1]
    assert (cr.raw_bits(v)[np.isnan(v)] == cr.NAN_BITS).all()


def test_abi_names():
    assert abi.AGG["CORRELATION"] == 12 and abi.AGG_ARG2(3) == 3 << 16 == abi.AGG_K(3)
    d = abi.make_agg_desc(col_types=["INT32", "INT32", "INT64"], aggs=[("CORRELATION", 0, 1), ("CORRELATION", 1, 0),
                                                                       ("COUNT_STAR", -1)])
    assert [d.aggs[i].kind for i in range(3)] == [12 | (1 << 16), 12, 0]
    assert [d.aggs[i].arg_col for i in range(3)] == [0, 1, -1]
    assert abi.result_types(d) == [abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"], abi.TYPE["INT64"]]
    assert abi.agg_result_len(d) == [1, 1, 1]


def test_header_defines_match_abi():
    text = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"(?m)^#define (KHIP_AGG_\w+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert defs["KHIP_AGG_CORRELATION"] == 12 == abi.AGG["CORRELATION"]
    assert re.search(r"(?m)^#define KHIP_AGG_ARG2\(col\) \(\(int32_t\)\(col\) << 16\)$", text)
    assert re.search(r"(?m)^#define KHIP_ABI_VERSION 8$", text)
    for ref in ("CorrelationUdaf.java:48-67", ":86-102", ":104-113", ":115-134", ":136-152", "2^32 - 1", "0x7FF8000000000000"):
        assert ref in text
