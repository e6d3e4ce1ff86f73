"""TOPK / TOPKDISTINCT (col, k) on the device, against the reference's QTT cases and the
oracle-derived expectation of tests/topk_ref.py (TopkKudaf / TopkDistinctKudaf.aggregate restated on
Python lists, folded over the (key, window) applications the unchanged oracle reports).  Every
comparison is exact; DOUBLEs are compared on canonical bits (every NaN one value, -0.0 is not 0.0).

The QTT cases (tests/golden/qtt_topk.json): topk integer / long / double [AVRO, JSON, PROTOBUF,
PROTOBUF_NOSR], topk distinct integer, topk distinct long.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import qtt
import topk_ref as tr
from ksql_amd import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("topk")
IDS = [c["name"] for c in CASES]
ENGINES = {"part": 0, "part_claim": abi.FLAG_PART_CLAIM, "atomic": abi.FLAG_ENGINE_ATOMIC}
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

def _case_lists(case, snap):
    d = case["desc"]
    per_agg = [tr.lists_of(snap, i, d["col_types"][a["arg_col"]]) for i, a in enumerate(d["aggs"])]
    return [(int(snap["key"][r]), [per_agg[i][r] for i in range(len(d["aggs"]))]) for r in range(snap["n"])]


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_topk_golden(prod, case, split, engine):
    """The final table (the reference's last output per key) from the snapshot."""
    h = abi.AggHandle(prod, tr.case_desc(case, flags=engine, changelog=False))
    n = len(case["input"])
    step = n if not split else split
    for lo in range(0, n, step):
        h.push(qtt.case_batch(case, lo, lo + step))
    snap = h.snapshot()
    h.close()
    final = {}
    for key, lists in tr.golden_outputs(case):
        final[key] = lists
    assert _case_lists(case, snap) == sorted(final.items())


@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_topk_output_sequence(prod, case, flags):
    """Every output record of the reference, in order, from one-record pushes ("topk distinct
    integer": the repeated unchanged row included)."""
    h = abi.AggHandle(prod, tr.case_desc(case, flags=flags))
    rows = []
    for lo in range(len(case["input"])):
        h.push(qtt.case_batch(case, lo, lo + 1))
        chg = h.changes()
        assert not chg["tombstone"].any()
        rows += _case_lists(case, chg)
    h.close()
    assert rows == tr.golden_outputs(case)


# ------------------------------------------------------------------ 2. contention

CN = 4096
CWIN = {"none": dict(window_kind="NONE"), "tumb": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0)}


def _contention_stream(win, typ):
    """4096 records on 2 keys, values from the 16 of topk_ref.pool, 30 % NULL: every lane of every
    wave runs its chain on the same one or two entries (per window)."""
    rng = np.random.default_rng(sum(win.encode()) + 1)  # timestamps and keys: the same for every type
    ts = np.sort(rng.integers(0, 12_000, CN)) + rng.integers(0, 3_000, CN)
    keys = rng.integers(0, 2, CN) + 40
    rng = np.random.default_rng(sum((win + typ).encode()) + 1)
    p = tr.pool(typ)
    return dict(ts=ts, keys=keys, key_valid=np.ones(CN, bool), row_valid=np.ones(CN, bool),
                cols=[p[rng.integers(0, len(p), CN)]], col_valid=[rng.random(CN) > 0.30])


@functools.lru_cache(maxsize=None)
def _contention_applications(win):
    s = _contention_stream(win, "INT32")  # (ts and keys do not depend on the type)
    return tr.applications(abi.load_oracle(), s["ts"], s["keys"], None, None, **CWIN[win])


@functools.lru_cache(maxsize=None)
def _contention_expectation(win, typ, k):
    s = _contention_stream(win, typ)
    e = tr.Expect(abi.load_oracle(), [typ], [("TOPK", 0, k), ("TOPKDISTINCT", 0, k)], **CWIN[win])
    e.push(apps=_contention_applications(win), **tr.push_args(s, 0, CN, 1))
    snap = e.snapshot()
    e.close()
    return s, snap


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("typ", tr.TYPES)
@pytest.mark.parametrize("win", list(CWIN))
def test_contention(prod, win, typ, k, engine):
    """One push, then the same stream in pushes of 1, 7, 64 and the rest (resident slots seed the
    chain): both equal the restatement."""
    s, exp = _contention_expectation(win, typ, k)
    kw = dict(col_types=[typ], aggs=[("TOPK", 0, k), ("TOPKDISTINCT", 0, k)], flags=engine, **CWIN[win])
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(abi.HostBatch(**tr.push_args(s, 0, CN, 1)))
    tr.assert_same(one.snapshot(), exp, "one push")
    one.close()
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    for lo, hi in tr.slices(CN, [1, 7, 64]):
        cut.push(abi.HostBatch(**tr.push_args(s, lo, hi, 1)))
    tr.assert_same(cut.snapshot(), exp, "pushes of 1, 7, 64 and the rest")
    cut.close()
    assert exp["n"] >= 2 and (~exp["nulls"][0]).all(axis=1).any()  # full lists


# ------------------------------------------------------------------ 3. random differential

@pytest.mark.parametrize("shape", tr.SHAPES)
@pytest.mark.parametrize("typ", tr.TYPES)
@pytest.mark.parametrize("win", list(tr.WINDOWS))
def test_random_vs_expectation(prod, win, typ, shape, engine):
    col_types, aggs, having = tr.query(typ, shape)
    s, per_push, (pull_keys, pull_ws, pull_exp), _, _ = tr.expectation(win, typ, shape)
    emits = engine != abi.FLAG_ENGINE_ATOMIC
    flags = engine | (abi.FLAG_CHANGELOG if emits else 0)
    kw = dict(col_types=col_types, aggs=aggs, flags=flags, having=having, **tr.WINDOWS[win])
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    nc = len(col_types)
    for (lo, hi), (est, esnap, echg) in zip(tr.slices(tr.N, tr.CUTS), per_push):
        st = cut.push(abi.HostBatch(**tr.push_args(s, lo, hi, nc)))
        assert st == est, (lo, hi, st, est)
        tr.assert_same(cut.snapshot(having), esnap, "snapshot after rows [%d, %d)" % (lo, hi))
        if emits:
            tr.assert_same(cut.changes(), echg, "changes of rows [%d, %d)" % (lo, hi))
    got = cut.get(keys=pull_keys, ws=pull_ws)
    tr.assert_same(got, pull_exp, "pull")
    assert got["n"] > 0
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(abi.HostBatch(**tr.push_args(s, 0, tr.N, nc)))
    tr.assert_same(one.snapshot(having), per_push[-1][1], "one push")
    one.close()
    cut.close()


# ------------------------------------------------------------------ 4. retry (child process, tuning build)

RETRY_LOG2P, RETRY_LDS_KB, RETRY_KEYS = 8, 64, 180_000


def _retry_child():
    """Tuning build, 256 partitions, a 64 KB k_part_agg table: the rows of TOPK(x, 3), TOPKDISTINCT(x, 3)
    over a BIGINT have 11 words (key, ws, row time, count, 3 + 3 slots, the Long.MIN_VALUE flag), 92
    bytes per entry, H = 512.  Push 1 brings 40 000 keys (156 +- 12 per partition, below the split
    threshold), push 2 two records for each of 180 000 keys (703 +- 26 per partition): every
    partition's table overflows on pass 0 and the partition is retried in sub-passes, with the
    resident slots of push 1 as the chain's seeds.  A failed pass must have written nothing: TOPK is
    not idempotent, a record applied twice shows as a duplicate in the list."""
    prod = abi.load_product()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    rng = np.random.default_rng(11)
    kw = dict(col_types=["INT64"], aggs=[("TOPK", 0, 3), ("TOPKDISTINCT", 0, 3)], capacity_hint=1024)
    g = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    keys1 = rng.permutation(40_000)
    keys2 = rng.permutation(np.repeat(np.arange(RETRY_KEYS), 2))
    allk, allx, allv = [], [], []
    for i, keys in enumerate((keys1, keys2)):
        x = rng.integers(-50, 50, len(keys))  # few values: duplicates within a key's 2-3 records
        v = rng.random(len(keys)) > 0.2
        os.write(2, b"[push %d]\n" % (i + 1))
        st = g.push(abi.HostBatch(np.zeros(len(keys), np.int64), keys=keys, cols=[x], col_valid=[v]))
        os.write(2, b"[push end]\n")
        assert st["windows_applied"] == len(keys)
        allk.append(keys), allx.append(x), allv.append(v)
    snap = g.snapshot()
    g.close()
    keys, x, v = np.concatenate(allk), np.concatenate(allx), np.concatenate(allv)
    exp = {}
    for k_, x_, v_ in zip(keys.tolist(), x.tolist(), v.tolist()):  # arrival order, unwindowed: the group is the key
        lists = exp.setdefault(k_, ([], []))
        if v_:
            tr.aggregate("TOPK", 3, "INT64", x_, lists[0])
            tr.aggregate("TOPKDISTINCT", 3, "INT64", x_, lists[1])
    assert snap["n"] == RETRY_KEYS and snap["key"].tolist() == sorted(exp)
    for a in (0, 1):
        assert tr.lists_of(snap, a, "INT64") == [exp[k_][a] for k_ in snap["key"].tolist()], a
    print("OK")


def test_retry_path():
    from test_gpu_c1_retry import TUNE_LIB
    from test_gpu_part_retry import parse_trace
    assert os.path.exists(TUNE_LIB), "tuning build not present (make -C ksql_amd TUNING=1)"
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", KHIP_PART_LOG2=str(RETRY_LOG2P),
               KHIP_LDS_KB=str(RETRY_LDS_KB))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_topk as t; "
                        "t._retry_child()" % (REPO, os.path.join(REPO, "tests"))], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stderr[-4000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2], (sorted(trace), p.stdout[-2000:], p.stderr[-3000:])
    passes = trace[2]
    # the TOPK handle ran k_part_agg (never a merge), overflowed its table and went through sub-passes
    assert all(t["kernel"] == "agg" and t["H"] == 512 and t["P"] == 1 << RETRY_LOG2P for t in trace[1] + passes), trace
    assert len(passes) >= 2 and passes[0]["fail_table"] > 0 and passes[0]["sub_items"] == 0, passes
    assert any(t["sub_items"] > 0 for t in passes[1:]) and passes[-1]["failed"] == 0, passes
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------ 5. EMIT FINAL

@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
def test_emit_final(prod, orc, flags):
    """TUMBLING 5 s, grace 0, three pushes: each push's closed windows carry their final lists."""
    rng = np.random.default_rng(3)
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0, retention_ms=600_000, col_types=["DOUBLE"],
              aggs=[("TOPK", 0, 3), ("COUNT_STAR", -1), ("TOPKDISTINCT", 0, 2)], emit="FINAL")
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=flags, **kw))
    e = tr.Expect(orc, **kw)
    closed = 0
    for b in range(3):
        n = 3000
        ts = b * 6000 + np.sort(rng.integers(0, 6000, n)) + rng.integers(0, 800, n)
        a = dict(ts=ts, keys=rng.integers(0, 50, n), cols=[tr.x_values(rng, n, "DOUBLE")], col_valid=[rng.random(n) > 0.3])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        chg, echg = g.changes(), e.changes()
        tr.assert_same(chg, echg, "closed by push %d" % b)
        closed += chg["n"]
        tr.assert_same(g.snapshot(), e.snapshot(), "push %d" % b)
    assert closed > 100
    g.close()
    e.close()


# ------------------------------------------------------------------ 6. khip_agg_push_shuffled

def test_push_shuffled(prod, orc):
    """One rank: rows packed by the shuffle go through khip_agg_push_shuffled's general route (the
    value pipeline declines a TOPK handle) and equal the columnar push of the unpacked rows."""
    import torch
    rng = np.random.default_rng(17)
    types = ["INT64", "INT64"]  # user_id (the new GROUP BY key), amount
    kw = dict(col_types=types, aggs=[("TOPK", 1, 3)], window_kind="TUMBLING", size_ms=5000, grace_ms=2000)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw))
    u = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    e = tr.Expect(orc, **kw)
    sh = abi.ShuffleHandle(prod, 1, 0, types)
    for p in range(2):
        n = 20_000
        ts = p * 10_000 + (np.arange(n) * 10_000) // n + rng.integers(0, 300, n)
        cols = [rng.integers(0, 500, n), rng.integers(-1000, 1000, n)]
        valid = [rng.random(n) > 0.05, rng.random(n) > 0.3]
        tc = [torch.as_tensor(c, dtype=torch.int64, device="cuda") for c in cols]
        tv = [abi.bitmap_torch(torch.as_tensor(v, device="cuda")) for v in valid]
        send, counts = sh.pack(abi.DeviceBatch(torch.as_tensor(ts, dtype=torch.int64, device="cuda"), cols=tc, col_valid=tv))
        m = int(sum(counts))
        gs = g.push_shuffled(sh, send, m)
        key, kts, ucols, uvalid = sh.unpack(send, m)
        us = u.push(abi.DeviceBatch(kts, keys=key, cols=ucols, col_valid=uvalid))
        keep = valid[0]  # the shuffle drops rows whose new key is NULL
        es = e.push(ts=ts[keep], keys=cols[0][keep], cols=[c[keep] for c in cols], col_valid=[v[keep] for v in valid])
        assert gs == us == es, (gs, us, es)
        tr.assert_same(g.snapshot(), e.snapshot(), "shuffled, push %d" % p)
        tr.assert_same(u.snapshot(), e.snapshot(), "unpacked, push %d" % p)
    assert g.kernel_times()["c1_pushes"] == 0
    for h in (g, u, e):
        h.close()
    sh.close()


# ------------------------------------------------------------------ 7. errors and result_len

def _create_status(prod, **kw):
    d = abi.make_agg_desc(**kw)
    h = C.c_void_p()
    st = prod.agg_create(C.byref(d), C.byref(h))
    msg = prod.dll.khip_last_error()
    if st == 0:
        prod.agg_destroy(h)
    return st, msg


@pytest.mark.parametrize("kind", ["TOPK", "TOPKDISTINCT"])
def test_rejections(prod, kind):
    ok = dict(col_types=["INT64"], aggs=[(kind, 0, 3)])
    assert _create_status(prod, **ok)[0] == 0
    cases = [
        (KHIP_E_UNSUPPORTED, dict(ok, window_kind="SESSION", size_ms=1000)),
        (KHIP_E_UNSUPPORTED, dict(ok, flags=abi.FLAG_TABLE_SOURCE)),
        (KHIP_E_UNSUPPORTED, dict(ok, having={"agg": 0, "op": "GT", "value": 1})),
        (KHIP_E_INVALID, dict(ok, aggs=[(abi.AGG[kind] | abi.AGG_KEEP_NULLS, 0, 3)])),
        (KHIP_E_INVALID, dict(ok, aggs=[(kind, 0, 0)])),
        (KHIP_E_INVALID, dict(ok, aggs=[(kind, 0, -1)])),
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=[(kind, 0, 30)])),          # 30 slots > 29 state words
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=[(kind, 0, 20), (kind, 0, 10)])),
        (KHIP_E_INVALID, dict(ok, aggs=[("SUM", 0, 3)])),              # k bits on another kind
        (KHIP_E_INVALID, dict(ok, aggs=[("COUNT_STAR", -1, 1)])),
    ]
    for want, kw in cases:
        st, msg = _create_status(prod, **kw)
        assert st == want and msg, (kw, st, msg)
    # the largest k that fits: 29 words less the count word (TOPK) / the Long.MIN_VALUE flag (TOPKDISTINCT of a BIGINT)
    assert _create_status(prod, **dict(ok, aggs=[(kind, 0, 28)]))[0] == 0
    assert _create_status(prod, **dict(ok, aggs=[(kind, 0, 29)]))[0] == KHIP_E_UNSUPPORTED
    # a HAVING on another aggregate of the query is fine; asked of the TOPK aggregate later it is not
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64"], aggs=[(kind, 0, 3), ("COUNT_STAR", -1)],
                                              having={"agg": 1, "op": "GT", "value": 1}))
    h.push(abi.HostBatch([1, 2, 3], keys=[5, 5, 6], cols=[np.array([7, 8, 9])]))
    snap = h.snapshot({"agg": 1, "op": "GT", "value": 1})
    assert snap["n"] == 1 and tr.lists_of(snap, 0, "INT64") == [[8, 7]]
    with pytest.raises(abi.KsqlHipError):
        h.snapshot({"agg": 0, "op": "GT", "value": 1})
    h.close()


def test_distinct_double_fits_29_slots(prod):
    """No flag word for DOUBLE / INT: TOPKDISTINCT(x, 29) fills the 29 state words exactly."""
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["DOUBLE"], aggs=[("TOPKDISTINCT", 0, 29)]))
    x = np.arange(100, dtype=np.float64) % 40
    h.push(abi.HostBatch(np.zeros(100, np.int64), keys=np.zeros(100, np.int64), cols=[x]))
    snap = h.snapshot()
    h.close()
    assert tr.lists_of(snap, 0, "DOUBLE") == [tr.canon_list([float(v) for v in range(39, 10, -1)], "DOUBLE")]


def test_result_len_and_type(prod):
    d = abi.make_agg_desc(col_types=["INT32", "DOUBLE"], aggs=[("TOPK", 0, 3), ("COUNT_STAR", -1), ("TOPKDISTINCT", 1, 8),
                                                              ("AVG", 0), ("LATEST_BY_OFFSET_NULLS", 1)])
    lens, types = [], []
    for i in range(5):
        v = C.c_int32(-1)
        assert prod.agg_result_len(C.byref(d), i, C.byref(v)) == 0
        lens.append(v.value)
        assert prod.agg_result_type(C.byref(d), i, C.byref(v)) == 0
        types.append(v.value)
    assert lens == [3, 1, 8, 1, 1] == abi.agg_result_len(d)
    assert types == abi.result_types(d) == [abi.TYPE["INT32"], abi.TYPE["INT64"], abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"],
                                            abi.TYPE["DOUBLE"]]
    v = C.c_int32()
    assert prod.agg_result_len(C.byref(d), 5, C.byref(v)) == KHIP_E_INVALID and prod.dll.khip_last_error()
