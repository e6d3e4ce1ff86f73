"""The partitioned engine's retry protocol on the host (ksql_amd/csrc/khip_retry.hpp, compiled
here for the host with g++ and the address / undefined-behaviour sanitizers through
tools/retry_plan_check.cpp): the work-item encoding, the pass-0 list from the learned bits, what
one pass's fail[] bytes make of the next pass, and the end-of-push rule.  CPU only."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAIL_TABLE, FAIL_REGION, FAIL_FATAL = 1, 2, 4


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rp") / "rpcheck")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe,
                           os.path.join(REPO, "tools", "retry_plan_check.cpp")])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return [json.loads(x) for x in p.stdout.splitlines()]
    return run


def plan(checker, learned, fails):
    """[pass-0 state, one state per fail vector (up to the first error)], learned bits afterwards."""
    words = ["plan", len(learned), len(fails)] + list(learned) + [f for v in fails for f in v]
    out = checker([" ".join(str(w) for w in words)])
    return out[:-1], out[-1]["learned"]


def item(p, sbits, sub):
    return p | sbits << 16 | sub << 20


def items_of(p, sbits):
    return [item(p, sbits, k) for k in range(1 << sbits)]


def test_item_round_trip(checker):
    cases = [(0, 0, 0), (65535, 12, 4095), (65535, 0, 0), (0, 12, 4095), (1234, 5, 31), (2047, 1, 1)]
    got = checker(["item %d %d %d" % c for c in cases])
    for (p, sbits, sub), g in zip(cases, got):
        assert g == {"w": item(p, sbits, sub), "p": p, "sbits": sbits, "sub": sub}
    assert got[1]["w"] == 0xFFFCFFFF  # every field at its limit, no overlap


def test_pass0_list(checker):
    (s0,), _ = plan(checker, [0, 0, 0, 0], [])
    assert s0["work"] == [] and s0["image"] == [] and s0["plist"] == [] and s0["sbits"] == [0, 0, 0, 0]
    learned = [0, 2, 0, 1, 3]
    (s0,), kept = plan(checker, learned, [])
    exp = [w for p, b in enumerate(learned) for w in items_of(p, b)]  # 2^sbits items each, in partition order
    assert len(exp) == 1 + 4 + 1 + 2 + 8
    assert s0["work"] == exp and s0["image"] == exp and s0["plist"] == []
    assert s0["decoded"] == [x for p, b in enumerate(learned) for k in range(1 << b) for x in (p, b, k)]
    assert kept == learned


def test_planner_fail_bits(checker):
    #          fits  table       region       both                      fatal
    fail = [0, FAIL_TABLE, FAIL_REGION, FAIL_TABLE | FAIL_REGION, FAIL_FATAL, 0]
    learned = [1, 0, 2, 1, 0, 0]
    (s0, s1), kept = plan(checker, learned, [fail])
    assert s1["ok"] and s1["grow"]
    assert s1["sbits"] == [1, 1, 2, 2, 0, 0]  # bit 1: one more sub-pass bit
    assert s1["plist"] == [1, 2, 3, 4]  # a partition that did not fail is absent
    exp = items_of(1, 1) + items_of(2, 2) + items_of(3, 2) + items_of(4, 0)  # ALL items of each are re-queued
    assert s1["work"] == exp
    assert s1["image"] == exp + [1, 2, 3, 4]  # the upload: work, then plist
    assert kept == [1, 1, 2, 2, 0, 0]
    # bit 1 alone: no growth; bit 2 alone: growth, the same sub-passes
    (_, t), _ = plan(checker, [0, 0], [[FAIL_TABLE, 0]])
    assert t["ok"] and not t["grow"] and t["sbits"] == [1, 0] and t["work"] == items_of(0, 1) and t["plist"] == [0]
    (_, t), _ = plan(checker, [0, 3], [[0, FAIL_REGION]])
    assert t["ok"] and t["grow"] and t["sbits"] == [0, 3] and t["work"] == items_of(1, 3) and t["plist"] == [1]
    # bit 4 alone (the push fails on the counter block's fatal flag): the partition is listed, nothing grows
    (_, t), _ = plan(checker, [0, 0], [[0, FAIL_FATAL]])
    assert t["ok"] and not t["grow"] and t["sbits"] == [0, 0] and t["work"] == items_of(1, 0) and t["plist"] == [1]


def test_planner_successive_passes(checker):
    steps, kept = plan(checker, [0, 0, 1], [[1, 0, 1], [1, 0, 0], [0, 0, 0]])
    assert [s["sbits"] for s in steps] == [[0, 0, 1], [1, 0, 2], [2, 0, 2], [2, 0, 2]]
    assert steps[1]["plist"] == [0, 2] and steps[2]["plist"] == [0] and steps[3]["plist"] == []
    assert steps[2]["work"] == items_of(0, 2) and steps[3]["work"] == [] and steps[3]["image"] == []
    assert not steps[2]["grow"]  # (reported per pass, not latched)
    assert kept == [2, 0, 2]


def test_too_many_sub_passes(checker):
    steps, _ = plan(checker, [12, 0], [[FAIL_TABLE, 0], [0, 0]])
    assert len(steps) == 2 and steps[0]["ok"] and len(steps[0]["work"]) == 4096 + 1
    assert not steps[1]["ok"] and steps[1]["sbits"][0] == 13
    assert len(steps[1]["work"]) < 8192  # the error status, not an 8192-item list
    steps, _ = plan(checker, [11], [[FAIL_TABLE]])
    assert steps[1]["ok"] and steps[1]["work"] == items_of(0, 12) and steps[1]["work"][-1] == item(0, 12, 4095)


def test_learn_keeps_the_maximum(checker):
    # learned[p] = max(learned[p], used[p]): bits only rise within a push, and stay
    _, kept = plan(checker, [3, 0, 1], [[0, 1, 0], [0, 1, 0]])
    assert kept == [3, 2, 1]
    _, kept = plan(checker, [3, 0, 1], [])
    assert kept == [3, 0, 1]


@pytest.mark.parametrize("P", [1, 2048])
def test_partition_counts(checker, P):
    learned = [(p * 7) % 3 for p in range(P)] if P > 1 else [0]
    fail = [(FAIL_TABLE if p % 5 == 0 else 0) | (FAIL_REGION if p % 11 == 3 else 0) for p in range(P)]
    if P == 1:
        fail = [FAIL_TABLE]
    (s0, s1), kept = plan(checker, learned, [fail])
    exp0 = [w for p, b in enumerate(learned) for w in items_of(p, b)] if any(learned) else []
    assert s0["work"] == exp0
    used = [b + (1 if f & FAIL_TABLE else 0) for b, f in zip(learned, fail)]
    failed = [p for p in range(P) if fail[p]]
    assert s1["ok"] and s1["sbits"] == used and s1["plist"] == failed
    assert s1["grow"] == any(f & FAIL_REGION for f in fail)
    exp1 = [w for p in failed for w in items_of(p, used[p])]
    assert s1["work"] == exp1 and s1["image"] == exp1 + failed
    assert kept == used
