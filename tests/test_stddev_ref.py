"""tests/stddev_ref.py on the CPU: the restated fold against the reference's QTT goldens (bit for
bit), the exact model against the goldens and against the fold (within the derived bound), the
undo path, and a guard that the expectations the GPU tests use are not vacuous.  CPU only."""
import os
import random
import re

import pytest

import qtt
import stddev_ref as sr
import topk_ref as tr
from ksql_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("stddev")
IDS = [c["name"] for c in CASES]


def _kind_typ(case):
    d = case["desc"]
    return d["aggs"][0]["kind"], d["col_types"][d["aggs"][0]["arg_col"]]


def test_fixture_cases():
    assert IDS == ["stddev_sample int", "stddev_sample long", "stddev_samp int", "stddev_samp long"]
    assert [_kind_typ(c) for c in CASES] == [("STDDEV_SAMPLE", "INT32"), ("STDDEV_SAMPLE", "INT64"),
                                             ("STDDEV_SAMP", "INT32"), ("STDDEV_SAMP", "INT64")]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_reproduces_goldens_bit_for_bit(case):
    kind, typ = _kind_typ(case)
    seqs = sr.case_sequences(case)
    assert len(seqs) == len(case["outputs"]) == 8
    for (key, xs), o in zip(seqs, case["outputs"]):
        assert key == o["key"] and not o["tombstone"]
        assert sr.bits(sr.fold(kind, typ, xs)) == sr.bits(o["values"][0]), (key, xs, sr.fold(kind, typ, xs), o["values"][0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_against_goldens(case):
    """Exact on both int cases and on key 100 of the long cases; everywhere within the bound.  Key 0
    of `stddev_samp long` is 1 ulp off: the model gives 1.5372286026580001e18, the fold (and the
    golden) 1.5372286026580004e18."""
    kind, typ = _kind_typ(case)
    off = []
    for (key, xs), o in zip(sr.case_sequences(case), case["outputs"]):
        got, want = sr.model(kind, xs), o["values"][0]
        assert abs(got - want) <= sr.rel_bound(len(xs)) * abs(want), (key, xs, got, want)
        if sr.bits(got) != sr.bits(want):
            off.append((key, got, want))
    if typ == "INT32":
        assert not off
    assert all(key == 0 for key, _, _ in off), off
    if case["name"] == "stddev_samp long":
        assert (0, 1.5372286026580001e18, 1.5372286026580004e18) in off


def _families(typ):
    fams = [lambda r: r.randint(-1000, 1000), lambda r: (1 << 20) + r.randrange(50)]
    if typ == "INT64":
        fams.append(lambda r: r.randint(-(1 << 40), 1 << 40))
    return fams


@pytest.mark.parametrize("typ", sr.TYPES)
def test_model_against_fold_random(typ):
    """Random groups, n from 2 to 2000, values in ±1e3, 2^20 + [0, 50) and (BIGINT) ±2^40: inputs on
    which no Java integer operation wraps, so no group is left out."""
    rng = random.Random(11 if typ == "INT32" else 12)
    groups, worst = 0, 0.0
    for g in range(400):
        n = rng.choice([2, 3, 4, 5, 8, 17, 64]) if g % 4 else rng.randint(100, 2000)
        fam = _families(typ)[g % len(_families(typ))]
        xs = [fam(rng) for _ in range(n)]
        for kind in sr.KINDS:
            f, m = sr.fold(kind, typ, xs), sr.model(kind, xs)  # (a Wrap fails the test: none may be skipped)
            assert abs(m - f) <= sr.rel_bound(n) * abs(f), (kind, n, m, f)
            if f:
                worst = max(worst, abs(m - f) / abs(f) / (n * sr.U))
        groups += 1
    assert groups == 400
    print("worst |model - fold| / (n u |fold|) = %.3f" % worst)


def test_fold_raises_where_java_wraps():
    with pytest.raises(sr.Wrap):
        sr.fold("STDDEV_SAMP", "INT32", [2**31 - 1, 2**31 - 1])       # the INT sum passes 2^31
    with pytest.raises(sr.Wrap):
        sr.fold("STDDEV_SAMP", "INT64", [1, 2**62, 2**62])            # x * (n + 1) passes 2^63
    assert sr.model("STDDEV_SAMP", [2**31 - 1, 2**31 - 1]) == 0.0     # the device path: the true variance
    assert sr.model("STDDEV_SAMP", [0, 2**62]) == float(2**123)


@pytest.mark.parametrize("typ", sr.TYPES)
def test_undo_within_the_absolute_bound(typ):
    """A table source: values enter and leave a group.  The reference's M2 after undos carries the
    rounding of every term added and removed, so the bound is absolute: (ops + 8) u A / (n - 1), A
    the sum of the magnitudes of all those terms.  STDDEV_SAMP only (the reference's M2 can go
    slightly negative after undos, and its sqrt is then NaN)."""
    rng = random.Random(21)
    checked = emptied = 0
    for g in range(200):
        fam = _families(typ)[g % len(_families(typ))]
        f, live = sr.Fold(typ), []
        for _ in range(rng.randint(5, 300)):
            if live and rng.random() < 0.4:
                f.undo(live.pop(rng.randrange(len(live))))
            else:
                live.append(fam(rng))
                f.aggregate(live[-1])
        if g % 10 == 0:  # a group emptied back to COUNT 0
            while live:
                f.undo(live.pop())
            emptied += 1
        n = len(live)
        assert f.count == n and f.sum == sum(live)
        m = sr.model("STDDEV_SAMP", live)
        if n < 2:
            assert m == 0.0 == f.map("STDDEV_SAMP")
            continue
        assert abs(m - f.map("STDDEV_SAMP")) <= (f.ops + 8) * sr.U * f.A / (n - 1), (n, m, f.map("STDDEV_SAMP"), f.A)
        checked += 1
    assert checked > 150 and emptied == 20


def test_model_edges():
    assert sr.model("STDDEV_SAMPLE", []) == sr.model("STDDEV_SAMPLE", [5]) == 0.0
    assert sr.model("STDDEV_SAMP", [7] * 1000) == 0.0
    assert sr.model("STDDEV_SAMP", [0, 10]) == 50.0 and sr.model("STDDEV_SAMPLE", [0, 10]) == 7.0710678118654755
    lo, hi = -2**63, 2**63 - 1
    assert sr.model("STDDEV_SAMP", [lo, hi]) == (2 * (lo * lo + hi * hi) - 1) / 2 / 1.0


@pytest.mark.parametrize("typ", sr.TYPES)
@pytest.mark.parametrize("win", list(tr.WINDOWS))
def test_gpu_expectations_are_not_vacuous(win, typ):
    """What tests/test_gpu_stddev.py compares against: groups with n = 0, 1, 2 and >= 1000 non-null
    records all occur (the thousand in the unwindowed stream, whose hot group nothing expires; a
    window of the others holds a few hundred), the HAVING hides rows, the pull query returns rows,
    the extremes are in."""
    s, per_push, pull, everything, stats = sr.expectation(win, typ, "beside")
    assert all(stats[k] > 0 for k in ("n0", "n1", "n2")), stats
    assert stats["n1000"] > 0 or win != "none", stats
    assert everything["values"][2].max() >= (1000 if win == "none" else 500)
    assert per_push[-1][1]["n"] < everything["n"] or win == "none"  # (every unwindowed group ends with two records)
    assert per_push[0][1]["n"] == 0 and per_push[0][0]["windows_applied"] <= 3  # the first record alone: hidden
    assert pull[2]["n"] > 0
    v = everything["values"][1]
    assert (v > 0).any() and ((v == 0).any() or win == "none") and not everything["nulls"][1].any()
    x = s["cols"][0][s["col_valid"][0]]
    assert x.min() == tr.pool(typ).min() and x.max() == tr.pool(typ).max()


def test_abi_names():
    assert abi.AGG["STDDEV_SAMP"] == 10 and abi.AGG["STDDEV_SAMPLE"] == 11
    d = abi.make_agg_desc(col_types=["INT32", "INT64"], aggs=[("STDDEV_SAMP", 0), ("STDDEV_SAMPLE", 1), ("COUNT_STAR", -1)])
    assert [d.aggs[i].kind for i in range(3)] == [10, 11, 0]
    assert abi.result_types(d) == [abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"], abi.TYPE["INT64"]]
    assert abi.agg_result_len(d) == [1, 1, 1]


def test_header_defines_match_abi():
    text = open(os.path.join(REPO, "include", "ksqldb_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"(?m)^#define (KHIP_AGG_\w+)\s+(0x[0-9A-Fa-f]+|\d+)\b", text)}
    assert defs["KHIP_AGG_STDDEV_SAMP"] == 10 and defs["KHIP_AGG_STDDEV_SAMPLE"] == 11
    assert re.search(r"(?m)^#define KHIP_ABI_VERSION 8$", text)
    for ref in ("StandardDeviationSampUdaf.java:124-144", ":170-176", ":179-196", "2^32 - 1"):
        assert ref in text
