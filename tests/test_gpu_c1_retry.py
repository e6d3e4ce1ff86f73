"""Eviction and retry in the same push: the C1 / C1V merges (ksql_amd/csrc/khip_agg_c1.hip).

A push's merge evicts the resident rows of closed windows to the closed store, and a partition
whose groups overflow the LDS table (fail bit 1) or its region (fail bit 2) is retried: ALL its
2^sbits sub-items run again over the same source rows.  A sibling item that fit on the failed pass
has already moved its closed rows, so every closed row must leave exactly once per push (the merge
moves them on the first pass only, failed items included; retries skip them).  A duplicate shows
as an extra row in snapshots, pulls and count_rows, an inflated `new` statistic, and a HAVING
count that counts the row twice: every case compares all of those with the oracle after each push.

Each case runs in a child process on the tuning build (KSQL_AMD_LIB_VARIANT=tune) with
KHIP_PART_LOG2=11 (2048 partitions, the fewest the pipelines take) and KHIP_C1_TRACE=1: c1_push
prints one line per merge pass, and the parent asserts from them that the second push really
EVICTED AND RETRIED before anything it compared counts: a pass with sub-items, failed partitions
and closed rows moved, followed by at least one more pass, all at P = 2048.

The three pushes (TUMBLING 5 s, grace 1 s, disorder < 100 ms; per-partition counts are means of a
binomial over 2048 partitions, the partition being the top bits of a hash of the key):
  1. W0 = [0, 5000): `w0` keys per partition, one in eight with 4 records (HAVING COUNT > 3 holds
     for closed rows); W1 = [5000, 10000): `w1` keys.
  2. `g2` new keys per partition in [10000, 14600): W0 closes as of the stream time before the
     push (evicted in this push), W1's rows stay live, untouched residents.
  3. records in [14500, 17100) over all earlier keys: W2's rows are merged again, W1 closes.
RETENTION 10 min: the default (size + grace) would expire W0 from snapshots as it closes.
HOPPING 6 s / 2 s uses the same times: windows starting at 0 and 2000 close in push 2, those at
4000, 6000 and 8000 stay open.

Shapes (hmax = 3/4 of the LDS table; cmax = the region's rows, from the hint):
- region: KHIP_C1_LOG2H=11 (hmax 1536), hint 2^20 (cmax 2048, no sub-passes to start with),
  w0 300, w1 100, g2 2500.  Pass 0: every partition overflows the table.  Pass 1 (2 sub-items of
  1250 +- 35 entries): the first item fits the region, the second does not.  Pass 2 after the
  regrow.  6.6 M records.
- table_subs0: hint 2^22 (cmax 8192, every partition starts with 2 sub-items), g2 3072: each
  sub-item holds 1536 +- 39 entries, about half overflow the table on pass 0 while their siblings
  fit (fail_table > 0, fail_region == 0 on that pass).  7.7 M records.
- region_id64 / region_wide: the region shape with keys from a pool over 2^30 above 2^40 (64-bit
  identities) and with keys spread over 2^53 (wide records: the first push is redone wide).
- the value pipeline at KHIP_C1V_LOG2H=9 (hmax 384): sum_i64 TUMBLING + HAVING + changelog at
  hint 600000 (cmax 1024, 2 sub-items to start with), w0 150, w1 300, g2 1100; c3_f64 TUMBLING at
  hint 2^19 (cmax 1024), w0 100, w1 150 (push 1 fits the table, so push 2 starts without
  sub-passes), g2 1100; all_i32 HOPPING at hint 2^18 (cmax 512), 50 / 60 / 330 keys per partition
  (a key's pane and its 3 windows share the table; push 1 already needs sub-passes for about half
  the partitions, which keep them).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE_LIB = os.path.join(REPO, "ksql_amd", "libksqldb_hip_tune.so")
LOG2P = 11
P = 1 << LOG2P

RETENTION = 600_000  # closed windows stay in the window store (the default, size + grace, expires them as they close)
COUNT_HAVING = {"agg": 0, "op": "GT", "value": 3}
SUM_HAVING = {"agg": 0, "op": "GT", "value": 0}

CASES = {
    "region": dict(knobs={"KHIP_C1_LOG2H": "11"}, hint=1 << 20, w=(300, 100, 2500), changes=True),
    "table_subs0": dict(knobs={"KHIP_C1_LOG2H": "11"}, hint=1 << 22, w=(300, 100, 3072), changes=False,
                        fail="table"),
    "region_id64": dict(knobs={"KHIP_C1_LOG2H": "11"}, hint=1 << 20, w=(300, 100, 2500), changes=False, keymap="pool30"),
    "region_wide": dict(knobs={"KHIP_C1_LOG2H": "11"}, hint=1 << 20, w=(300, 100, 2500), changes=False, keymap="bij53"),
    "v_sum_i64": dict(knobs={"KHIP_C1V_LOG2H": "9"}, hint=600_000, w=(150, 300, 1100), changes=True, shape="sum_i64",
                      having=SUM_HAVING, subs0=True),
    "v_all_i32_hop": dict(knobs={"KHIP_C1V_LOG2H": "9"}, hint=1 << 18, w=(50, 60, 330), changes=False, shape="all_i32",
                          hop=True),
    "v_c3_f64": dict(knobs={"KHIP_C1V_LOG2H": "9"}, hint=1 << 19, w=(100, 150, 1100), changes=False, shape="c3_f64",
                     subs0=False),
}


def _ramp(rng, n, t0, t1):
    """n timestamps rising from t0 to t1 with a disorder below 100 ms."""
    return t0 + (np.arange(n) * (t1 - t0)) // max(n, 1) + rng.integers(0, 100, n)


def three_pushes(rng, w, parts=P, keymap="dense", n3=400_000):
    """[(keys, ts)] * 3 for w = (W0 keys, W1 keys, push-2 keys) per partition (module docstring)."""
    n0, n1, n2 = (x * parts for x in w)
    ids = rng.permutation(n0 + n1 + n2)
    if keymap == "pool30":  # distinct keys over 2^30 above 2^40
        pool = rng.permutation(np.unique(rng.integers(0, 1 << 30, int(len(ids) * 1.05)))[: len(ids)])
        assert len(pool) == len(ids)
        ids = (1 << 40) + pool
    elif keymap == "bij53":  # a bijection on [0, 2^53) (odd multiplier)
        ids = (ids * 0x5DEECE66D) & ((1 << 53) - 1)
    k0, k1, k2 = ids[:n0], ids[n0:n0 + n1], ids[n0 + n1:]
    heavy = k0[: n0 // 8]
    ka = rng.permutation(np.concatenate([k0, heavy, heavy, heavy]))
    p1 = (np.concatenate([ka, k1]), np.concatenate([_ramp(rng, len(ka), 0, 4900), _ramp(rng, n1, 5000, 9500)]))
    p2 = (k2, _ramp(rng, n2, 10_000, 14_500))
    p3 = (ids[rng.integers(0, len(ids), n3)], _ramp(rng, n3, 14_500, 17_000))
    return [p1, p2, p3], k0


def run_three_pushes(prod, orc, name, case, parts=P, c1_pushes=3):
    """The case's three pushes through the product and the oracle, everything compared after each
    push and at the end (module docstring).  Returns the product's kernel_times counters.
    c1_pushes: the pushes the pipeline must have taken (0: the general path took them all)."""
    from ksql_amd import abi
    from test_gpu_parity import assert_snap_equal
    rng = np.random.default_rng(sum(name.encode()))
    pushes, k0 = three_pushes(rng, case["w"], parts, case.get("keymap", "dense"))
    shape = case.get("shape")
    flags = abi.FLAG_CHANGELOG if case["changes"] else 0
    if shape is None:
        having = COUNT_HAVING
        kw = dict(window_kind="TUMBLING", size_ms=5000, advance_ms=5000, grace_ms=1000, aggs=[("COUNT_STAR", -1)],
                  capacity_hint=case["hint"], having=having, retention_ms=RETENTION)
        batches = [abi.HostBatch(ts, keys=k) for k, ts in pushes]
    else:
        from test_gpu_c1v import SHAPES, _values
        having = case.get("having")
        win = dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000) if case.get("hop") else \
            dict(window_kind="TUMBLING", size_ms=5000)
        kw = dict(col_types=SHAPES[shape][0], aggs=SHAPES[shape][1], capacity_hint=case["hint"], having=having,
                  grace_ms=1000, retention_ms=RETENTION, **win)
        batches = [abi.HostBatch(ts, keys=k, cols=[_values(rng, len(k), shape)], col_valid=[rng.random(len(k)) > 0.03])
                   for k, ts in pushes]
    gd, od = abi.make_agg_desc(flags=flags | abi.FLAG_PROFILE, **kw), abi.make_agg_desc(flags=flags, **kw)
    g, o = abi.AggHandle(prod, gd), abi.AggHandle(orc, od)
    for i, b in enumerate(batches):
        os.write(2, b"[push %d]\n" % (i + 1))
        gs, os_ = g.push(b), o.push(b)
        print("push", i + 1, gs, flush=True)
        assert gs == os_, (i, gs, os_)
        if case["changes"]:
            gc, oc = g.changes(), o.changes()
            assert_snap_equal(gc, oc, gd)
            assert np.array_equal(gc["tombstone"], oc["tombstone"]), i
        osnap = o.snapshot()
        assert g.snapshot()["n"] == osnap["n"], i
        assert g.count_rows(None) == osnap["n"], i
        if having is not None:
            assert g.count_rows(having) == o.snapshot(having)["n"], i
    os.write(2, b"[push end]\n")
    assert_snap_equal(g.snapshot(), osnap, gd)
    # pulls of keys whose W0 rows were closed in the retried push: one row per (key, window)
    keys = np.unique(k0[rng.integers(0, len(k0), 300)])
    got = g.get(keys=keys)
    m = np.isin(osnap["key"], keys)
    exp = {"n": int(m.sum()), "key": osnap["key"][m], "ws": osnap["ws"][m], "we": osnap["we"][m],
           "rowtime": osnap["rowtime"][m], "values": [v[m] for v in osnap["values"]],
           "nulls": [v[m] for v in osnap["nulls"]]}
    assert exp["n"] >= len(keys)
    assert len(set(zip(got["key"].tolist(), got["ws"].tolist()))) == got["n"]
    assert_snap_equal(got, exp, gd)
    kt = g.kernel_times()
    g.close()
    o.close()
    assert kt["c1_pushes"] == c1_pushes and kt["c1_declined"] == 0, kt
    return kt


def _child(name):
    """Child process (tuning build): the case against the oracle; prints OK."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from ksql_amd import abi
    prod, orc = abi.load_product(), abi.load_oracle()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    kt = run_three_pushes(prod, orc, name, CASES[name])
    print(json.dumps({"c1_pushes": kt["c1_pushes"], "c1_declined": kt["c1_declined"]}))
    print("OK")


TRACE = re.compile(r"^\[c1 trace\] (.*)$")


def parse_trace(stderr):
    """{push number: [one dict of ints per pass]} from the child's stderr."""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.match(r"^\[push (\d+)\]$", line)
        if m:
            cur = out.setdefault(int(m.group(1)), [])
            continue
        if line == "[push end]":
            cur = None
        m = TRACE.match(line)
        if m and cur is not None:
            cur.append({k: int(v) for k, v in (f.split("=") for f in m.group(1).split())})
    return out


def evicted_and_retried(passes):
    """The pass (its index) on which a sibling had evicted while another item failed, when a later
    pass follows; else None."""
    for i, t in enumerate(passes[:-1]):
        if t["sub_items"] > 0 and t["failed"] > 0 and t["closed_after"] > t["closed_before"]:
            return i
    return None


def run_child(name, knobs, timeout=300):
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_C1_TRACE="1", KHIP_PART_LOG2=str(LOG2P), **knobs)
    return subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_c1_retry as t; "
                           "t._child(%r)" % (os.path.join(REPO, "tests"), name)], cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("name", list(CASES))
def test_c1_evict_and_retry(name):
    if not os.path.exists(TUNE_LIB):
        pytest.skip("tuning build not present (make -C ksql_amd TUNING=1)")
    case = CASES[name]
    p = run_child(name, case["knobs"])
    print(p.stderr[-6000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2, 3], sorted(trace)
    passes = trace[2]
    val = 0 if case.get("shape") is None else 1
    assert passes and all(t["P"] == P and t["val"] == val for t in passes), passes
    assert [t["pass"] for t in passes] == list(range(len(passes))), passes
    w = evicted_and_retried(passes)
    assert w is not None, passes
    if case.get("fail") == "table":  # a pass 0 that already runs sub-items: table overflow alone
        assert w == 0 and passes[0]["pass"] == 0, passes
        assert passes[0]["fail_table"] > 0 and passes[0]["fail_region"] == 0, passes
    else:  # the region overflow with a fitting sibling
        assert any(t["sub_items"] > 0 and t["fail_region"] > 0 for t in passes[:-1]), passes
    if "subs0" in case:
        assert (passes[0]["sub_items"] > 0) == case["subs0"], passes
    # the closed store grew once: its rows after the last pass are those after the first
    assert passes[-1]["closed_after"] == passes[0]["closed_after"] > passes[0]["closed_before"], passes
