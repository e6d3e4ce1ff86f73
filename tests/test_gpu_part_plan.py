"""Which kernels a handle runs on the general path (part_push, khip_agg_part.hip).

part_plan computes every host-known decision of a push (PartGeo); in the tuning build, under
KHIP_PART_TRACE=1, part_push prints it as one `[part plan]` line per push, next to the per-pass
`[part trace]` lines.  The parity tests pass on every path, so a change that made a shape fall back
to a slower kernel would go unnoticed: this test pins the plan and the aggregate kernel per shape.

Each case runs in a child process on the tuning build: two pushes of 200 000 records, INT64 keys,
about 20 000 distinct, push b with timestamps in [20 000 b, 20 000 (b + 1)) plus a jitter below
400 ms.  TUMBLING 5000 ms with grace 1000 unless the case has its own window, so the second push
meets resident rows and closes windows.  After each push the statistics and the snapshot are
compared with the oracle; then the parent asserts the `[part plan]` fields and the `kernel=` values
of the `[part trace]` lines.  r12: 0 / 1 = the merge reads 12-byte records / 2 = pass A only.

window_range: 50 keys x 1000 windows of 1 ms per push: c1_plan and merge_allow hold on the host,
k_part_wrange declines more than 255 windows at P = 256 on the device, pass 0 is redone and the
only kernel traced is k_part_agg.

tile / nT (4096 records, 49 tiles) follow from the tile-halving loop with 256 CUs: the child
reports the device's CU count and the two fields are asserted only when it is 256.
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
N = 200_000
TUMBLING = dict(window_kind="TUMBLING", size_ms=5000)
COUNT = dict(aggs=[("COUNT_STAR", -1)])
SUM = dict(col_types=["INT64"], aggs=[("SUM", 0)])
TWO = dict(col_types=["INT64", "INT64"], aggs=[("SUM", 0), ("MAX", 1)])

CASES = {
    "count_tumbling": dict(q=dict(COUNT, **TUMBLING), hint=1 << 16, kernel="merge_c1",
                           plan=dict(rw=2, P=256, lvl2=0, stage=1, r8k=1, wk=0, r12=1, cnt1=1, c1_plan=1)),
    "count_none": dict(q=dict(COUNT, window_kind="NONE"), hint=1 << 16, kernel="merge",
                       plan=dict(rw=2, stage=1, r8k=0, r12=1, cnt1=1, c1_plan=0)),
    "sum_tumbling": dict(q=dict(SUM, **TUMBLING), hint=1 << 16, kernel="merge",
                         plan=dict(rw=4, stage=0, wstage=1, wk=1, r12=0, cnt1=0)),
    "count_hopping": dict(q=dict(COUNT, window_kind="HOPPING", size_ms=6000, advance_ms=2000), hint=1 << 16,
                          kernel="merge", plan=dict(rw=4, wstage=1, wk=1, cnt1=0)),
    "two_columns": dict(q=dict(TWO, **TUMBLING), hint=1 << 16, kernel="merge",
                        plan=dict(rw=6, stage=0, wstage=0, wk=0, r12=0)),
    "count_tumbling_2lvl": dict(q=dict(COUNT, **TUMBLING), hint=1 << 21, knobs={"KHIP_C1P": "0"}, kernel="merge_c1",
                                plan=dict(P=2048, lvl2=1, fbits=6, stage=1, r8k=1, r12=1, c1_plan=1)),
    "sum_tumbling_2lvl": dict(q=dict(SUM, **TUMBLING), hint=1 << 21, knobs={"KHIP_C1V": "0"}, kernel="merge",
                              plan=dict(P=2048, lvl2=1, fbits=6, wstage=1, wk=1)),
    "two_columns_2lvl": dict(q=dict(TWO, **TUMBLING), hint=1 << 20, kernel="merge",
                             plan=dict(P=2048, lvl2=1, fbits=6, stage=0, wstage=0)),
    "window_range": dict(q=dict(COUNT, window_kind="TUMBLING", size_ms=1), hint=1 << 16, kernel="agg", narrow_ts=True,
                         plan=dict(c1_plan=1, merge_allow=1)),
}
TILE = dict(tile=4096, nT=49)  # at P <= 2048 and N records, 256 CUs


def _batches(rng, case):
    from ksql_amd import abi
    out = []
    for b in range(2):
        if case.get("narrow_ts"):
            keys, ts = rng.integers(0, 50, N), rng.integers(0, 1000, N)
        else:
            keys = rng.integers(0, 20_000, N)
            ts = 20_000 * b + np.sort(rng.integers(0, 20_000, N)) + rng.integers(0, 400, N)
        cols = [rng.integers(-1 << 40, 1 << 40, N) for _ in case["q"].get("col_types", ())]
        out.append(abi.HostBatch(ts, keys=keys, cols=cols, col_valid=[rng.random(N) > 0.03 for _ in cols]))
    return out


def _child(name):
    """Child process (tuning build): the case against the oracle; prints the CU count and OK."""
    import torch
    from ksql_amd import abi
    from test_gpu_parity import assert_snap_equal
    prod, orc = abi.load_product(), abi.load_oracle()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    case = CASES[name]
    kw = dict(case["q"], grace_ms=1000, capacity_hint=case["hint"], retention_ms=600_000)
    gd, od = abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw), abi.make_agg_desc(**kw)
    g, o = abi.AggHandle(prod, gd), abi.AggHandle(orc, od)
    for i, b in enumerate(_batches(np.random.default_rng(sum(name.encode())), case)):
        gs, os_ = g.push(b), o.push(b)
        print("push", i + 1, gs, flush=True)
        assert gs == os_, (i, gs, os_)
        assert_snap_equal(g.snapshot(), o.snapshot(), gd)
    kt = g.kernel_times()
    assert kt["c1_pushes"] == 0, kt  # the general path took both pushes
    g.close()
    o.close()
    print("n_cu=%d" % torch.cuda.get_device_properties(0).multi_processor_count)
    print("OK")


def _fields(stderr, tag):
    return [dict(f.split("=") for f in m.group(1).split())
            for m in re.finditer(r"^\[%s\] (.*)$" % re.escape(tag), stderr, re.M)]


@pytest.mark.parametrize("name", list(CASES))
def test_part_plan(name):
    if not os.path.exists(TUNE_LIB):
        pytest.skip("tuning build not present (make -C ksql_amd TUNING=1)")
    case = CASES[name]
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", **case.get("knobs", {}))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_part_plan as t; "
                        "t._child(%r)" % (os.path.join(REPO, "tests"), name)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    print(p.stderr[-6000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])
    n_cu = int(re.search(r"^n_cu=(\d+)$", p.stdout, re.M).group(1))
    want = dict(case["plan"], **(TILE if n_cu == 256 else {}))
    plans = _fields(p.stderr, "part plan")
    assert len(plans) == 2, plans  # one line per general-path push
    for plan in plans:
        assert {k: int(plan[k]) for k in want} == want, (plan, want)
    kernels = [t["kernel"] for t in _fields(p.stderr, "part trace")]
    assert len(kernels) >= 2 and set(kernels) == {case["kernel"]}, kernels
