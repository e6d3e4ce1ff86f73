"""LATEST_BY_OFFSET / EARLIEST_BY_OFFSET on the device, against the reference's QTT cases and the
oracle-derived expectation of tests/offset_ref.py (MAX / MIN of a sequence column through the
unchanged oracle, translated back to values).  Values are compared bit for bit.

The QTT cases (tests/golden/qtt_offset.json): latest by offset (projected), nulls ignored - single,
nulls not ignored - single, latest by offset with all nulls, earliest by offset (projected), null
first - single - ignoring nulls, null first - single - not ignoring nulls, nulls later - single -
nulls ignored, null later - single - nulls not ignored, earliest by offset with all nulls.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import offset_ref
import qtt
from ksql_amd import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("offset")
IDS = [c["name"] for c in CASES]
ENGINES = {"part": 0, "part_claim": abi.FLAG_PART_CLAIM, "atomic": abi.FLAG_ENGINE_ATOMIC}
FORMS = list(offset_ref.OFFSET)
WINDOWS = {"none": dict(window_kind="NONE"),
           "tumb": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0),
           "hop": dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, grace_ms=0)}
KHIP_E_INVALID, KHIP_E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


@pytest.fixture(params=list(ENGINES), scope="module")
def engine(request):
    return ENGINES[request.param]


# ------------------------------------------------------------------ 1. QTT

def test_case_count():
    assert len(CASES) == 10


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_offset_golden(prod, case, split, engine):
    """The final table: the fold of the changelog on the partitioned engine's two selections, the
    snapshot on the global-atomic engine (it keeps no EMIT CHANGES log)."""
    if engine == abi.FLAG_ENGINE_ATOMIC:
        assert qtt.compare_agg(case, qtt.run_agg_store(prod, case, split, flags=engine)) == []
    else:
        assert qtt.compare_agg(case, qtt.run_agg_case(prod, case, split, flags=engine)) == []
        assert qtt.compare_agg(case, qtt.run_agg_store(prod, case, split, flags=engine)) == []


@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_offset_output_sequence(prod, case, flags):
    """Every output record of the reference, in order, from one-record pushes."""
    assert qtt.compare_outputs(case, qtt.run_agg_outputs(prod, case, 1, flags=flags)) == []


# ------------------------------------------------------------------ 2. random differential

N, NKEYS = 20_000, 300
CUTS = [1, 7, 4096]  # pushes of 1, 7, 4096 rows and the rest


def _x_values(rng, n, typ):
    if typ == "INT32":
        return rng.integers(-2**31, 2**31, n).astype(np.int32)
    if typ == "INT64":
        return rng.integers(-2**63, 2**63 - 1, n)
    x = rng.uniform(-1e6, 1e6, n)
    bits = x.view(np.int64)
    nan = rng.random(n) < 0.05  # NaNs with distinct payloads, quiet and signalling, both signs
    bits[nan] = (0x7FF0000000000000 | rng.integers(1, 1 << 52, n)[nan]) | (rng.integers(0, 2, n)[nan] << 63)
    x[rng.random(n) < 0.03] = 0.0
    x[rng.random(n) < 0.03] = -0.0
    return x


def _stream(seed, typ, n=N, nkeys=NKEYS):
    """30 % NULL arguments, 5 % null keys / null rows / negative timestamps, a disorder (8 s) above
    the windows' size at grace 0, so some records are late."""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.integers(0, 90_000, n)) + rng.integers(0, 8_000, n)
    ts = np.where(rng.random(n) < 0.05, -rng.integers(1, 100, n), ts)
    return dict(ts=ts, keys=rng.integers(-nkeys // 2, nkeys // 2, n) * 1_000_003, key_valid=rng.random(n) > 0.05,
                row_valid=rng.random(n) > 0.05,
                cols=[_x_values(rng, n, typ), rng.integers(-1000, 1000, n), rng.integers(-2**31, 2**31, n).astype(np.int32)],
                col_valid=[rng.random(n) > 0.30, rng.random(n) > 0.05, rng.random(n) > 0.05])


def _query(typ, shape):
    """(a) the offset aggregate alone; (b) all four forms beside COUNT(*), SUM and MAX of other columns."""
    if shape in FORMS:
        return [typ], [(shape, 0)]
    return [typ, "INT64", "INT32"], [("COUNT_STAR", -1), ("LATEST_BY_OFFSET", 0), ("SUM", 1), ("EARLIEST_BY_OFFSET", 0),
                                     ("MAX", 2), ("LATEST_BY_OFFSET_NULLS", 0), ("EARLIEST_BY_OFFSET_NULLS", 0)]


def _slices(n, cuts):
    out, lo = [], 0
    for c in cuts:
        out.append((lo, min(lo + c, n)))
        lo = min(lo + c, n)
    out.append((lo, n))
    return out


def _push_args(s, lo, hi, ncols):
    return dict(ts=s["ts"][lo:hi], keys=s["keys"][lo:hi], key_valid=s["key_valid"][lo:hi],
                row_valid=s["row_valid"][lo:hi], cols=[c[lo:hi] for c in s["cols"][:ncols]],
                col_valid=[v[lo:hi] for v in s["col_valid"][:ncols]])


@functools.lru_cache(maxsize=None)
def _expectation(win, typ, shape):
    """The stream and, per push of the cutting, the expected statistics, snapshot and changes
    (computed once per query, shared by the three engine selections)."""
    orc = abi.load_oracle()
    col_types, aggs = _query(typ, shape)
    s = _stream(sum((win + typ + shape).encode()), typ)
    e = offset_ref.Expect(orc, col_types, aggs, flags=abi.FLAG_CHANGELOG, **WINDOWS[win])
    per_push = []
    for lo, hi in _slices(N, CUTS):
        st = e.push(**_push_args(s, lo, hi, len(col_types)))
        per_push.append((st, e.snapshot(), e.changes()))
    e.close()
    return s, per_push


@pytest.mark.parametrize("shape", FORMS + ["beside"])
@pytest.mark.parametrize("typ", ["INT32", "INT64", "DOUBLE"])
@pytest.mark.parametrize("win", list(WINDOWS))
def test_random_vs_expectation(prod, win, typ, shape, engine):
    col_types, aggs = _query(typ, shape)
    s, per_push = _expectation(win, typ, shape)
    emits = engine != abi.FLAG_ENGINE_ATOMIC
    flags = engine | (abi.FLAG_CHANGELOG if emits else 0)
    one = abi.AggHandle(prod, abi.make_agg_desc(col_types=col_types, aggs=aggs, flags=flags, **WINDOWS[win]))
    cut = abi.AggHandle(prod, abi.make_agg_desc(col_types=col_types, aggs=aggs, flags=flags, **WINDOWS[win]))
    nc = len(col_types)
    one.push(abi.HostBatch(**_push_args(s, 0, N, nc)))
    late = 0
    for (lo, hi), (est, esnap, echg) in zip(_slices(N, CUTS), per_push):
        st = cut.push(abi.HostBatch(**_push_args(s, lo, hi, nc)))
        assert st == est, (lo, hi, st, est)
        late += st["windows_late"]
        snap = cut.snapshot()
        offset_ref.assert_same(snap, esnap, "snapshot after rows [%d, %d)" % (lo, hi))
        if emits:
            chg = cut.changes()
            offset_ref.assert_same(chg, echg, "changes of rows [%d, %d)" % (lo, hi))
            # the emitted rows are the snapshot's rows of the touched groups (where still retained)
            at = {(int(k), int(w)): i for i, (k, w) in enumerate(zip(snap["key"], snap["ws"]))}
            for r, (k, w) in enumerate(zip(chg["key"], chg["ws"])):
                i = at.get((int(k), int(w)))
                if i is None:
                    continue
                for a in range(len(aggs)):
                    assert chg["nulls"][a][r] == snap["nulls"][a][i]
                    assert chg["nulls"][a][r] or offset_ref.bits(chg["values"][a])[r] == offset_ref.bits(snap["values"][a])[i]
    if win != "none":
        assert late > 0  # grace 0 under an 8 s disorder: late records were dropped
    final = per_push[-1][1]
    assert final["n"] > 0
    offset_ref.assert_same(one.snapshot(), final, "one push")
    offset_ref.assert_same(one.snapshot(), cut.snapshot(), "one push vs cut")
    one.close()
    cut.close()


@pytest.mark.parametrize("form,typ,win", [("LATEST_BY_OFFSET", "INT64", "tumb"), ("EARLIEST_BY_OFFSET", "DOUBLE", "hop"),
                                          ("LATEST_BY_OFFSET_NULLS", "INT32", "hop"),
                                          ("EARLIEST_BY_OFFSET_NULLS", "INT64", "tumb")])
def test_value_pipeline(prod, orc, form, typ, win):
    """The offset aggregate alone, in order within the grace period, at a hint that gives the value
    pipeline its partition count: every push must take the pipeline (the hidden sequence column is
    its argument column), resident rows merged across pushes."""
    rng = np.random.default_rng(sum((form + typ + win).encode()))
    w = dict(WINDOWS[win], grace_ms=2000)
    kw = dict(col_types=[typ], aggs=[(form, 0)], capacity_hint=3_000_000, **w)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE | abi.FLAG_CHANGELOG, **kw))
    e = offset_ref.Expect(orc, flags=abi.FLAG_CHANGELOG, **kw)
    n, span = 100_000, 12_000
    for b in range(3):
        ts = b * span + (np.arange(n) * span) // n + rng.integers(0, 500, n)
        a = dict(ts=ts, keys=rng.integers(0, 20_000, n), cols=[_x_values(rng, n, typ)], col_valid=[rng.random(n) > 0.3])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        offset_ref.assert_same(g.changes(), e.changes(), "changes of push %d" % b)
        offset_ref.assert_same(g.snapshot(), e.snapshot(), "push %d" % b)
    kt = g.kernel_times()
    assert kt["c1_pushes"] == 3 and kt["c1_declined"] == 0, kt
    g.close()
    e.close()


# ------------------------------------------------------------------ 3. contention

@pytest.mark.parametrize("nkeys", [1, 2])
def test_contention(prod, nkeys, engine):
    """65 536 rows on one key (two keys) in 8 pushes: latest is the last valid row, earliest the first."""
    rng = np.random.default_rng(nkeys)
    n, col_types = 65_536, ["INT64"]
    aggs = [(f, 0) for f in FORMS]
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=col_types, aggs=aggs, flags=engine))
    keys = rng.integers(0, nkeys, n) + 40
    x = rng.integers(-2**62, 2**62, n)
    xv = rng.random(n) > 0.3
    xv[:3] = False  # the first rows are NULL: EARLIEST(x) is not row 0, EARLIEST(x, false) is NULL
    xv[-2:] = False
    for lo in range(0, n, n // 8):
        g.push(abi.HostBatch(np.zeros(n // 8, np.int64), keys=keys[lo:lo + n // 8], cols=[x[lo:lo + n // 8]],
                             col_valid=[xv[lo:lo + n // 8]]))
    snap = g.snapshot()
    g.close()
    assert snap["n"] == nkeys and list(snap["key"]) == [40, 41][:nkeys]
    for r, k in enumerate(snap["key"]):
        rows = np.flatnonzero(keys == k)
        valid = rows[xv[rows]]
        exp = {"LATEST_BY_OFFSET": valid[-1], "EARLIEST_BY_OFFSET": valid[0], "LATEST_BY_OFFSET_NULLS": rows[-1],
               "EARLIEST_BY_OFFSET_NULLS": rows[0]}
        for a, f in enumerate(FORMS):
            assert bool(snap["nulls"][a][r]) == (not xv[exp[f]]), (f, k)
            if xv[exp[f]]:
                assert snap["values"][a][r] == x[exp[f]], (f, k)


# ------------------------------------------------------------------ 4. updated and closed in one push

@pytest.mark.parametrize("emit", ["CHANGES", "FINAL"])
@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
def test_updated_and_closed_in_one_push(prod, orc, flags, emit):
    """One push holds window 0's records and then a record far enough ahead to close it (grace 0):
    the snapshot and a pull return window 0 with its values; EMIT FINAL emits the closed row."""
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0, retention_ms=600_000, col_types=["DOUBLE"],
              aggs=[(f, 0) for f in FORMS], emit=emit)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=flags, **kw))
    e = offset_ref.Expect(orc, **kw)
    a = dict(ts=[100, 200, 300, 400, 4999, 20_000], keys=[7, 7, 8, 7, 8, 9],
             cols=[np.array([1.5, 2.5, -0.0, 3.5, 4.5, 6.5])], col_valid=[[False, True, True, True, False, True]])
    assert g.push(abi.HostBatch(**a)) == e.push(**a)
    snap = g.snapshot()
    offset_ref.assert_same(snap, e.snapshot())
    assert list(snap["key"]) == [7, 8, 9] and list(snap["ws"]) == [0, 0, 20_000]
    assert [v[0] for v in snap["values"]] == [3.5, 2.5, 3.5, 0.0] and [bool(x[0]) for x in snap["nulls"]] == [False, False, False, True]
    assert np.signbit(snap["values"][0][1]) and snap["values"][0][1] == 0.0 and bool(snap["nulls"][2][1])
    got = g.get(keys=[7, 8], ws=(0, 0))
    offset_ref.assert_same(got, e.get(keys=[7, 8], ws=(0, 0)))
    assert got["n"] == 2
    if emit == "FINAL":
        chg = g.changes()
        offset_ref.assert_same(chg, e.changes())
        assert list(chg["key"]) == [7, 8] and list(chg["ws"]) == [0, 0] and chg["values"][0][0] == 3.5
    # a second push closes window 20 000 and leaves the closed rows as they are
    b = dict(ts=[40_000], keys=[7], cols=[np.array([9.5])], col_valid=[[True]])
    assert g.push(abi.HostBatch(**b)) == e.push(**b)
    offset_ref.assert_same(g.snapshot(), e.snapshot())
    if emit == "FINAL":
        offset_ref.assert_same(g.changes(), e.changes())
    g.close()
    e.close()


# ------------------------------------------------------------------ 5. retry path (child process, tuning build)

RETRY_W = (20, 20, 420)  # keys per partition: W0, W1, push 2 (420 +- 20 new groups against a 384-entry table)


def _retry_child():
    """Tuning build, KHIP_PART_LOG2=11, KHIP_C1V_LOG2H=9: push 2 overflows the merge's LDS table in
    nearly every partition and is retried with sub-passes; every push against the expectation."""
    from test_gpu_c1_retry import P, three_pushes
    prod, orc = abi.load_product(), abi.load_oracle()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    rng = np.random.default_rng(5)
    pushes, _ = three_pushes(rng, RETRY_W, P, n3=50_000)
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=1000, retention_ms=600_000, col_types=["DOUBLE"],
              aggs=[("LATEST_BY_OFFSET", 0)], capacity_hint=1 << 19)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw))
    e = offset_ref.Expect(orc, **kw)
    for i, (k, ts) in enumerate(pushes):
        os.write(2, b"[push %d]\n" % (i + 1))
        a = dict(ts=ts, keys=k, cols=[_x_values(rng, len(k), "DOUBLE")], col_valid=[rng.random(len(k)) > 0.3])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        os.write(2, b"[push end]\n")
        offset_ref.assert_same(g.snapshot(), e.snapshot(), "push %d" % (i + 1))
    kt = g.kernel_times()
    assert kt["c1_pushes"] == 3 and kt["c1_declined"] == 0, kt
    print("OK")


def test_retry_path():
    from test_gpu_c1_retry import LOG2P, TUNE_LIB, parse_trace
    assert os.path.exists(TUNE_LIB), "tuning build not present (make -C ksql_amd TUNING=1)"
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_C1_TRACE="1", KHIP_PART_LOG2=str(LOG2P), KHIP_C1V_LOG2H="9")
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_offset as t; "
                        "t._retry_child()" % (REPO, os.path.join(REPO, "tests"))], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stderr[-4000:])
    trace = parse_trace(p.stderr)
    # the trace first: a pass with failed partitions followed by another pass, in push 2
    assert 2 in trace and len(trace[2]) >= 2, (trace, p.stdout[-2000:], p.stderr[-3000:])
    assert any(t["failed"] > 0 for t in trace[2][:-1]) and all(t["val"] == 1 for t in trace[2]), trace[2]
    assert trace[2][-1]["failed"] == 0, trace[2]
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------ 6. variants

def test_utf8_keys(prod, orc, engine):
    """Dictionary keys and digit keys (inline ids) in one stream."""
    rng = np.random.default_rng(9)
    n = 6000
    ids = rng.integers(0, 200, n)
    keys = ["%d" % k if k % 3 == 0 else "00%d" % k if k % 5 == 0 else "k%d" % k if k % 7 else "éè-%d" % k for k in ids]
    kw = dict(key_type="UTF8", col_types=["INT32"], aggs=[(f, 0) for f in FORMS], **WINDOWS["tumb"])
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=engine, **kw))
    e = offset_ref.Expect(orc, **kw)
    ts = np.sort(rng.integers(0, 30_000, n)) + rng.integers(0, 6000, n)
    x, xv, kv = _x_values(rng, n, "INT32"), rng.random(n) > 0.3, rng.random(n) > 0.05
    for lo, hi in _slices(n, [1500, 1500]):
        a = dict(ts=ts[lo:hi], utf8_keys=keys[lo:hi], key_valid=kv[lo:hi], cols=[x[lo:hi]], col_valid=[xv[lo:hi]])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        offset_ref.assert_same(g.snapshot(), e.snapshot())
    g.close()
    e.close()


def test_partition_domain(prod, orc, engine):
    """KHIP_TIME_PARTITION with 4 partitions against 4 independent tasks."""
    from test_gpu_time_domains import _partition_batches, _union
    rng = np.random.default_rng(13)
    P = 4
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=1000, col_types=["INT64"], aggs=[(f, 0) for f in FORMS],
              capacity_hint=1 << 20)
    gd = abi.make_agg_desc(time_domain="PARTITION", n_partitions=P, flags=engine, **kw)
    g = abi.AggHandle(prod, gd)
    tasks = [offset_ref.Expect(orc, **kw) for _ in range(P)]
    late = 0
    for k, t, v, p in _partition_batches(rng, P, nb=3, per=4000, keys_per_part=300):
        vv = rng.random(len(k)) > 0.3
        gs = g.push(abi.HostBatch(t, keys=k, cols=[v], col_valid=[vv], partition=p))
        os_ = [tasks[q].push(t[p == q], [v[p == q]], [vv[p == q]], keys=k[p == q]) for q in range(P)]
        for f in ("rows_accepted", "windows_applied", "windows_late"):
            assert gs[f] == sum(o[f] for o in os_), f
        late += gs["windows_late"]
    assert late > 0
    offset_ref.assert_same(g.snapshot(), _union([h.snapshot() for h in tasks], gd))
    g.close()
    for h in tasks:
        h.close()


def test_supplied_domain(prod, orc, engine):
    """KHIP_TIME_SUPPLIED in one process: the stream time of khip_stream_time_scan as the column."""
    rng = np.random.default_rng(17)
    n = 8000
    kw = dict(col_types=["DOUBLE"], aggs=[(f, 0) for f in FORMS], **WINDOWS["hop"])
    g = abi.AggHandle(prod, abi.make_agg_desc(time_domain="SUPPLIED", flags=engine, **kw))
    e = offset_ref.Expect(orc, **kw)
    ts = np.sort(rng.integers(0, 40_000, n)) + rng.integers(0, 7000, n)
    keys, x, xv = rng.integers(0, 150, n), _x_values(rng, n, "DOUBLE"), rng.random(n) > 0.3
    seed, late = -1, 0
    for lo, hi in _slices(n, [3000, 3000]):
        st, seed = g.stream_time_scan(abi.HostBatch(ts[lo:hi], keys=keys[lo:hi]), seed)
        gs = g.push(abi.HostBatch(ts[lo:hi], keys=keys[lo:hi], cols=[x[lo:hi]], col_valid=[xv[lo:hi]], stream_time=np.array(st)))
        assert gs == e.push(ts[lo:hi], [x[lo:hi]], [xv[lo:hi]], keys=keys[lo:hi])
        late += gs["windows_late"]
        offset_ref.assert_same(g.snapshot(), e.snapshot())
    assert late > 0
    g.close()
    e.close()


def test_sink_encode(prod):
    """khip_sink_encode of a snapshot: a JSON value holding a NULL and a DOUBLE."""
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["DOUBLE", "INT32"],
                                              aggs=[("LATEST_BY_OFFSET", 0), ("EARLIEST_BY_OFFSET_NULLS", 1)]))
    g.push(abi.HostBatch([0, 0, 0], keys=[5, 5, 6], cols=[np.array([1.25, 2.5, 0.0]), np.array([3, 4, 9], np.int32)],
                         col_valid=[[True, True, False], [False, True, True]]))
    snap = g.snapshot()
    g.close()
    sink = abi.SinkHandle(prod, "KAFKA", [("ID", "INT64")], "JSON", [("L", "DOUBLE", 0), ("E", "INT32", 1)])
    keys, values = sink.encode(snap)
    sink.close()
    assert [int.from_bytes(k, "big", signed=True) for k in keys] == [5, 6]
    assert [json.loads(v) for v in values] == [{"L": 2.5, "E": None}, {"L": None, "E": 9}]


# ------------------------------------------------------------------ 7. rejections, reset

def _create_status(prod, desc):
    h = C.c_void_p()
    st = prod.agg_create(C.byref(desc), C.byref(h))
    msg = prod.dll.khip_last_error().decode()
    if st == 0:
        prod.agg_destroy(h)
    return st, msg


def test_rejections(prod):
    off = [("LATEST_BY_OFFSET", 0)]
    st, msg = _create_status(prod, abi.make_agg_desc(window_kind="SESSION", size_ms=1000, col_types=["INT32"], aggs=off))
    assert st == KHIP_E_UNSUPPORTED and "SESSION" in msg
    st, msg = _create_status(prod, abi.make_agg_desc(col_types=["INT32"], aggs=off, flags=abi.FLAG_TABLE_SOURCE))
    assert st == KHIP_E_UNSUPPORTED and "table source" in msg
    hav = {"agg": 1, "op": "GT", "value": 3}
    st, msg = _create_status(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[("COUNT_STAR", -1)] + off, having=hav))
    assert st == KHIP_E_UNSUPPORTED and "HAVING" in msg
    # HAVING on another aggregate of the same query stays supported
    st, _ = _create_status(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[("COUNT_STAR", -1)] + off,
                                                    having={"agg": 0, "op": "GT", "value": 3}))
    assert st == 0
    st, msg = _create_status(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[(abi.AGG["COUNT"] | abi.AGG_KEEP_NULLS, 0)]))
    assert st == KHIP_E_INVALID and "KEEP_NULLS" in msg
    st, _ = _create_status(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[(9, -1)]))
    assert st == KHIP_E_INVALID
    # 6 user columns + 3 hidden sequence columns (two arguments' validity, one without) do not fit 8
    st, msg = _create_status(prod, abi.make_agg_desc(col_types=["INT32"] * 6, aggs=[
        ("LATEST_BY_OFFSET", 0), ("LATEST_BY_OFFSET", 1), ("EARLIEST_BY_OFFSET_NULLS", 2)]))
    assert st == KHIP_E_UNSUPPORTED and "hidden" in msg
    st, _ = _create_status(prod, abi.make_agg_desc(col_types=["INT32"] * 6, aggs=[
        ("LATEST_BY_OFFSET", 0), ("EARLIEST_BY_OFFSET", 0), ("EARLIEST_BY_OFFSET_NULLS", 2)]))
    assert st == 0


def test_call_time_having_rejected(prod):
    """A khip_having given to a snapshot or a count that names an offset aggregate: refused, as at
    create; one naming another aggregate of the query filters as usual."""
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[("COUNT_STAR", -1), ("EARLIEST_BY_OFFSET", 0)]))
    g.push(abi.HostBatch([0, 0, 0], keys=[1, 1, 2], cols=[np.array([5, 6, 7], np.int32)]))
    for call in (g.snapshot, g.count_rows):
        with pytest.raises(abi.KsqlHipError, match=r"\(-4\).*HAVING"):
            call({"agg": 1, "op": "GT", "value": 0})
    snap = g.snapshot({"agg": 0, "op": "GT", "value": 1})
    assert list(snap["key"]) == [1] and list(snap["values"][1]) == [5]
    g.close()


def test_push_shuffled_rejected(prod):
    import torch
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64", "INT64"], aggs=[("LATEST_BY_OFFSET", 1)],
                                              **WINDOWS["tumb"]))
    sh = abi.ShuffleHandle(prod, 1, 0, ["INT64", "INT64"])
    rows = torch.zeros((8, prod.dll.khip_shuffle_row_words(sh.h)), dtype=torch.int64, device="cuda")
    st = prod.agg_push_shuffled(g.h, sh.h, rows.data_ptr(), 8, None)
    assert st == KHIP_E_UNSUPPORTED and "shuffled" in prod.dll.khip_last_error().decode()
    sh.close()
    g.close()


def test_reset_then_same_stream(prod, orc, engine):
    s = _stream(3, "INT64", n=5000)
    col_types, aggs = _query("INT64", "beside")
    kw = dict(col_types=col_types, aggs=aggs, **WINDOWS["hop"])
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=engine, **kw))
    e = offset_ref.Expect(orc, **kw)
    snaps = []
    for _ in range(2):
        for lo, hi in _slices(5000, [1000, 2500]):
            g.push(abi.HostBatch(**_push_args(s, lo, hi, 3)))
        snaps.append(g.snapshot())
        g.reset()
    for lo, hi in _slices(5000, [1000, 2500]):
        e.push(**_push_args(s, lo, hi, 3))
    offset_ref.assert_same(snaps[0], e.snapshot())
    offset_ref.assert_same(snaps[1], snaps[0], "after reset")
    g.close()
    e.close()
