"""Eviction and retry in the same push on the general path (part_push, khip_agg_part.hip): the
workloads of test_gpu_c1_retry.py with the pipelines switched off, so the same records go through
k_part_merge_c1 (COUNT(*)) and the generic k_part_merge (SUM).  The retry protocol is the one
both drivers share: a failed partition re-runs ALL its sub-items, closed rows
leave on the first pass only.  A duplicate closed row would show in snapshots, pulls, count_rows,
the `new` statistic and the HAVING count, all compared with the oracle after every push
(test_gpu_c1_retry.run_three_pushes).

Each case runs in a child process on the tuning build with KHIP_PART_LOG2=11 (2048 partitions) and
KHIP_PART_TRACE=1: part_push prints one `[part trace]` line per pass, and the parent asserts from
them that push 2 really evicted and retried: a pass with failed partitions after which the closed
store had grown, followed by at least one more pass.  (The closed count of a push is read back
once, after pass 0, where every eviction happens: closed_after is that word on every pass.)

The `region` workload (three_pushes, w = (300, 100, 2500), hint 2^20 → cmax 2048 rows per region,
no sub-passes to start with, HAVING, changelog, RETENTION 10 min, 6.6 M records).  Unlike the
pipelines' merges (3/4 of the table), k_part_merge_c1 and k_part_merge fail a partition only when
a probe sequence wraps the WHOLE delta table (probes >= H), so what overflows is H itself:
- merge_c1: KHIP_C1P=0 KHIP_C1_LOG2H=11, H = 2048.  Push 2 brings 2500 +- 50 new groups per
  partition (binomial over 2048 partitions): pass 0 evicts W0's 300 closed rows per partition and
  every partition overflows the table (2500 - 2048 is 9 sigma).  Pass 1 runs 2 sub-items of 1250
  +- 35 entries, which fit; the region then holds W1's 100 live rows + 2500 new ones > cmax 2048:
  fail_region, the regions grow to 4096 rows, pass 2 places everything.
- merge: the sum_i64 shape with KHIP_C1V=0 and KHIP_MERGE_LDS_KB=40: the generic merge's table is
  mH = (40 KB / entry bytes - 64) rounded down to 64 entries = 1792 (22-byte entries: id, sum,
  rowtime, list slot) — below 2500 - 5 sigma and above 1250 + 5 sigma, so the passes are the same
  three.  Live groups before push 2 (400 per partition) stay below the split threshold
  (3/8 of mH per partition), so P is still 2048 in push 2.
"""
import json
import os
import re
import subprocess
import sys

import pytest
from test_gpu_c1_retry import LOG2P, P, SUM_HAVING, TUNE_LIB, run_three_pushes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "merge_c1": dict(knobs={"KHIP_C1P": "0", "KHIP_C1_LOG2H": "11"}, hint=1 << 20, w=(300, 100, 2500), changes=True,
                     kernel="merge_c1", H=2048),
    "merge": dict(knobs={"KHIP_C1V": "0", "KHIP_MERGE_LDS_KB": "40"}, hint=1 << 20, w=(300, 100, 2500), changes=True,
                  shape="sum_i64", having=SUM_HAVING, kernel="merge", H=1792),
}

TRACE = re.compile(r"^\[part trace\] (.*)$")


def _child(name):
    """Child process (tuning build): the case against the oracle; prints OK."""
    from ksql_amd import abi
    prod, orc = abi.load_product(), abi.load_oracle()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    kt = run_three_pushes(prod, orc, name, CASES[name], c1_pushes=0)
    print(json.dumps({"c1_pushes": kt["c1_pushes"], "c1_declined": kt["c1_declined"]}))
    print("OK")


def parse_trace(stderr):
    """{push number: [one dict per pass]} from the child's stderr (ints, but the kernel's name)."""
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
            f = dict(x.split("=") for x in m.group(1).split())
            cur.append({k: (v if k == "kernel" else int(v)) for k, v in f.items()})
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_part_evict_and_retry(name):
    if not os.path.exists(TUNE_LIB):
        pytest.skip("tuning build not present (make -C ksql_amd TUNING=1)")
    case = CASES[name]
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", KHIP_PART_LOG2=str(LOG2P), **case["knobs"])
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_part_retry as t; "
                        "t._child(%r)" % (os.path.join(REPO, "tests"), name)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    print(p.stderr[-6000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2, 3], sorted(trace)
    passes = trace[2]
    assert passes and all(t["P"] == P and t["kernel"] == case["kernel"] for t in passes), passes
    assert all(t["H"] == case["H"] for t in passes), passes
    assert [t["pass"] for t in passes] == list(range(len(passes))), passes
    # evicted and retried: failed partitions, closed rows moved, and at least one more pass
    assert any(t["failed"] > 0 and t["closed_after"] > t["closed_before"] for t in passes[:-1]), passes
    # the shape's own course: the table overflows on pass 0, the region on a pass with sub-items
    assert passes[0]["fail_table"] > 0 and passes[0]["sub_items"] == 0, passes
    assert any(t["sub_items"] > 0 and t["fail_region"] > 0 for t in passes[:-1]), passes
    assert passes[-1]["failed"] == 0, passes
    # the closed store grew once in the push
    assert len({t["closed_after"] for t in passes}) == 1, passes
