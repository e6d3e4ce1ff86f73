"""The partitioned engine's alternative kernel paths, forced through the tuning build's knobs.

The release library always takes the measured defaults, so some paths run only when a push
declines the default one.  Here each knob set runs in a child process on the tuning build
(`KSQL_AMD_LIB_VARIANT=tune`: the same kernels, KHIP_* knobs read from the environment), with a
COUNT(*) TUMBLING + HAVING workload against the oracle (table, batch statistics, HAVING count):
- KHIP_C1P=0: the general path instead of the COUNT(*) pipeline (khip_agg_c1.hip);
- KHIP_R8K=0: R8 records through the general scatter / refine kernels, not their own ones;
- KHIP_R8_U=4: R8 staged steps of 4 records per thread;
- KHIP_SCATTER2=0: one-level scatter (no refine pass);
- KHIP_R8=0: 12-byte (R12) records where R8 would fit;
- KHIP_C1P=0 + KHIP_C1_AU=4: the general path's COUNT(*) merge with fewer records per thread;
- KHIP_C1_LOG2H=13 / 11: the pipeline's merge with a twice larger LDS table, and with a twice
  smaller one (partitions overflow it: the sub-pass retries);
- KHIP_C1V=0: value aggregates through the general path instead of the value-record pipeline;
  KHIP_C1V_SPEC=0: its merge without the plane-shape specialisation (SUM(BIGINT) here);
  KHIP_C1V_LOG2H=9: a small LDS table (sub-pass retries, split by key).
Each case runs COUNT(*) TUMBLING + HAVING and SUM of a BIGINT + HAVING over HOPPING (panes).
Dense and sparse key ranges, several pushes (resident rows), late records (the pipeline declines),
and one push of many distinct keys ("many": 3.4 M for COUNT(*), ~1660 groups per partition at the
2048 partitions of its hint; 1.2 M of them for the HOPPING SUM, whose hint starts every partition
with 4 sub-items: ~146 keys each, a pane and 3 windows per key, ~586 entries): the three other
cases stay far below the small tables (about 49 groups per partition against 1536; the value
pipeline's sub-items from the hint hold well under 384 entries), so only this one makes
KHIP_C1_LOG2H=11 / KHIP_C1V_LOG2H=9 retry.  The child runs with
KHIP_C1_TRACE=1 (one line per merge pass on stderr) and for those two knob sets the test asserts
that the matching pipeline shows a pass with failed partitions.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE_LIB = os.path.join(REPO, "ksql_amd", "libksqldb_hip_tune.so")

KNOBS = [
    {"KHIP_C1P": "0"},
    {"KHIP_C1P": "0", "KHIP_R8K": "0"},
    {"KHIP_C1P": "0", "KHIP_R8_U": "4"},
    {"KHIP_C1P": "0", "KHIP_SCATTER2": "0"},
    {"KHIP_C1P": "0", "KHIP_R8": "0"},
    {"KHIP_C1P": "0", "KHIP_C1_AU": "4"},
    {"KHIP_C1_LOG2H": "13"},
    {"KHIP_C1_LOG2H": "11"},
    {"KHIP_C1V": "0"},
    {"KHIP_C1V_SPEC": "0"},
    {"KHIP_C1V_LOG2H": "9"},
]


def _check():
    """Child process: every case against the oracle; prints OK."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from ksql_amd import abi
    from test_gpu_parity import assert_snap_equal
    prod, orc = abi.load_product(), abi.load_oracle()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    having = {"agg": 0, "op": "GT", "value": 2}
    for case in ("dense", "sparse", "late"):
        rng = np.random.default_rng(len(case))
        batches = []
        t0 = 0
        for b in range(3):
            n = 600_000
            if case == "sparse":
                k = rng.integers(0, 50_000, n) * 7919 + (1 << 45)
            else:
                k = rng.integers(0, 50_000, n)
            ts = t0 + (np.arange(n) * 20_000) // n + rng.integers(0, 400, n)
            if case == "late":
                ts[rng.random(n) < 0.02] -= 15_000
            t0 += 20_000
            v = rng.integers(-1000, 1000, n)
            batches.append(abi.HostBatch(ts, keys=k, cols=[v], col_valid=[rng.random(n) > 0.02]))
        grace = 2000 if case == "late" else -1
        kws = [dict(window_kind="TUMBLING", size_ms=5000, grace_ms=grace, aggs=[("COUNT_STAR", -1)], having=having,
                    capacity_hint=1 << 22),
               dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, grace_ms=grace, col_types=["INT64"],
                    aggs=[("SUM", 0)], having={"agg": 0, "op": "GT", "value": 0},
                    capacity_hint=1 << 22)]
        for kw in kws:
            gd, od = abi.make_agg_desc(**kw), abi.make_agg_desc(**kw)
            g, o = abi.AggHandle(prod, gd), abi.AggHandle(orc, od)
            for b in batches:
                gs, os_ = g.push(b), o.push(b)
                assert gs == os_, (case, gs, os_)
            assert_snap_equal(g.snapshot(), o.snapshot(), gd)
            assert g.count_rows(kw["having"]) == o.snapshot(kw["having"])["n"], case
            g.close()
            o.close()
    # "many": one push, more groups per partition than the small tables take
    rng = np.random.default_rng(4)
    n = 3_400_000
    k = rng.permutation(n)
    ts = (np.arange(n) * 4900) // n + rng.integers(0, 100, n)
    v = rng.integers(-1000, 1000, n)
    vv = rng.random(n) > 0.02
    m = 1_200_000  # HOPPING: ts from 4000 on, so every record has its pane and 3 windows in the table
    th = 4000 + (np.arange(m) * 4900) // m + rng.integers(0, 100, m)
    runs = [(dict(window_kind="TUMBLING", size_ms=5000, aggs=[("COUNT_STAR", -1)], having=having, capacity_hint=1 << 21),
             abi.HostBatch(ts, keys=k)),
            (dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, col_types=["INT64"], aggs=[("SUM", 0)],
                  having={"agg": 0, "op": "GT", "value": 0}, capacity_hint=1 << 21),
             abi.HostBatch(th, keys=k[:m], cols=[v[:m]], col_valid=[vv[:m]]))]
    for kw, b in runs:
        gd, od = abi.make_agg_desc(**kw), abi.make_agg_desc(**kw)
        g, o = abi.AggHandle(prod, gd), abi.AggHandle(orc, od)
        gs, os_ = g.push(b), o.push(b)
        assert gs == os_, ("many", gs, os_)
        assert_snap_equal(g.snapshot(), o.snapshot(), gd)
        assert g.count_rows(kw["having"]) == o.snapshot(kw["having"])["n"], "many"
        g.close()
        o.close()
    print("OK")


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_knob_paths_match_oracle(knobs):
    if not os.path.exists(TUNE_LIB):
        pytest.skip("tuning build not present (make -C ksql_amd TUNING=1)")
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_C1_TRACE="1", **knobs)
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_knobs as t; t._check()"
                        % os.path.join(REPO, "tests")], cwd=REPO, env=env, capture_output=True, text=True, timeout=200)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])
    # the knob sets that promise sub-pass retries: their pipeline shows a pass with failed partitions
    val = {("KHIP_C1_LOG2H", "11"): 0, ("KHIP_C1V_LOG2H", "9"): 1}.get(tuple(knobs.items())[0] if len(knobs) == 1 else None)
    if val is not None:
        failed = [int(m.group(1)) for m in re.finditer(r"^\[c1 trace\] val=%d .* failed=(\d+) " % val, p.stderr, re.M)]
        assert failed and max(failed) > 0, p.stderr[-3000:]
