"""STDDEV_SAMP / STDDEV_SAMPLE over INT / BIGINT on the device, against the reference's QTT cases
and the exact model of tests/stddev_ref.py (the groups' n, Σx, Σx² over the (key, window)
applications the unchanged oracle reports, decoded with one rounding).  Comparisons against the model
are bit for bit through the int64 view; against the reference's goldens within (n + 8) 2^-53.

The QTT cases (tests/golden/qtt_stddev.json): stddev_sample int / long, stddev_samp int / long.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qtt
import stddev_ref as sr
import topk_ref as tr
from ksql_amd import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("stddev")
IDS = [c["name"] for c in CASES]
ENGINES = {"part": 0, "part_claim": abi.FLAG_PART_CLAIM, "atomic": abi.FLAG_ENGINE_ATOMIC}
KHIP_E_INVALID, KHIP_E_UNSUPPORTED = -1, -4
I64_MIN, I64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


@pytest.fixture(params=list(ENGINES), scope="module")
def engine(request):
    return ENGINES[request.param]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


# ------------------------------------------------------------------ 1. QTT

def _kind(case):
    return case["desc"]["aggs"][0]["kind"]


def _check_rows(case, rows, expected):
    """rows: (key, value) from the device; expected: (key, xs, golden) — exact against the model,
    within the bound against the golden."""
    assert [k for k, _ in rows] == [k for k, _, _ in expected]
    for (key, got), (_, xs, gold) in zip(rows, expected):
        assert sr.bits(got) == sr.bits(sr.model(_kind(case), xs)), (key, xs, got, sr.model(_kind(case), xs))
        assert abs(got - gold) <= sr.rel_bound(len(xs)) * abs(gold), (key, xs, got, gold)


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_stddev_golden(prod, case, split, engine):
    """The final table (the reference's last output per key) from the snapshot."""
    h = abi.AggHandle(prod, qtt.case_desc(case, flags=engine, changelog=False))
    n = len(case["input"])
    step = n if not split else split
    for lo in range(0, n, step):
        h.push(qtt.case_batch(case, lo, lo + step))
    snap = h.snapshot()
    h.close()
    assert not snap["nulls"][0].any() and snap["values"][0].dtype == np.float64
    final = {}
    for (key, xs), o in zip(sr.case_sequences(case), case["outputs"]):
        final[key] = (key, xs, o["values"][0])
    _check_rows(case, list(zip(snap["key"].tolist(), snap["values"][0].tolist())), [final[k] for k in sorted(final)])


@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_stddev_output_sequence(prod, case, flags):
    """Every output record of the reference, in order, from one-record pushes (the record with a
    NULL argument repeats the row unchanged)."""
    h = abi.AggHandle(prod, qtt.case_desc(case, flags=flags))
    rows = []
    for lo in range(len(case["input"])):
        h.push(qtt.case_batch(case, lo, lo + 1))
        chg = h.changes()
        assert not chg["tombstone"].any() and not chg["nulls"][0].any()
        rows += list(zip(chg["key"].tolist(), chg["values"][0].tolist()))
    h.close()
    _check_rows(case, rows, [(k, xs, o["values"][0]) for (k, xs), o in zip(sr.case_sequences(case), case["outputs"])])


# ------------------------------------------------------------------ 2. contention

CN = 4096
CWIN = {"none": dict(window_kind="NONE"), "tumb": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0)}
CAGGS = [("STDDEV_SAMP", 0), ("STDDEV_SAMPLE", 0)]


def _contention_stream(win, typ):
    """4096 records on 2 keys, values from the 16 of topk_ref.pool (BIGINT: Long.MIN_VALUE,
    Long.MAX_VALUE and ±2^62 among them: 126-bit squares, signed high parts), 30 % NULL: every lane of
    every wave adds to the same one or two entries (per window)."""
    rng = np.random.default_rng(sum(win.encode()) + 1)  # timestamps and keys: the same for every type
    ts = np.sort(rng.integers(0, 12_000, CN)) + rng.integers(0, 3_000, CN)
    keys = rng.integers(0, 2, CN) + 40
    rng = np.random.default_rng(sum((win + typ).encode()) + 1)
    p = tr.pool(typ)
    return dict(ts=ts, keys=keys, key_valid=np.ones(CN, bool), row_valid=np.ones(CN, bool),
                cols=[p[rng.integers(0, len(p), CN)]], col_valid=[rng.random(CN) > 0.30])


@functools.lru_cache(maxsize=None)
def _contention_expectation(win, typ):
    s = _contention_stream(win, typ)
    e = sr.Expect(abi.load_oracle(), [typ], CAGGS, **CWIN[win])
    e.push(**tr.push_args(s, 0, CN, 1))
    snap = e.snapshot()
    e.close()
    return s, snap


@pytest.mark.parametrize("typ", sr.TYPES)
@pytest.mark.parametrize("win", list(CWIN))
def test_contention(prod, win, typ, engine):
    """One push, then the same stream in pushes of 1, 7, 64 and the rest (resident words seed the
    sums): both equal the model."""
    s, exp = _contention_expectation(win, typ)
    kw = dict(col_types=[typ], aggs=CAGGS, flags=engine, **CWIN[win])
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(abi.HostBatch(**tr.push_args(s, 0, CN, 1)))
    tr.assert_same(one.snapshot(), exp, "one push")
    one.close()
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    for lo, hi in tr.slices(CN, [1, 7, 64]):
        cut.push(abi.HostBatch(**tr.push_args(s, lo, hi, 1)))
    tr.assert_same(cut.snapshot(), exp, "pushes of 1, 7, 64 and the rest")
    cut.close()
    assert exp["n"] >= 2 and (exp["values"][0] > 0).all()
    assert np.array_equal(_bits(np.sqrt(exp["values"][0])), _bits(exp["values"][1]))


# ------------------------------------------------------------------ 3. random differential

@pytest.mark.parametrize("shape", sr.SHAPES)
@pytest.mark.parametrize("typ", sr.TYPES)
@pytest.mark.parametrize("win", list(tr.WINDOWS))
def test_random_vs_expectation(prod, win, typ, shape, engine):
    col_types, aggs, having = sr.query(typ, shape)
    s, per_push, (pull_keys, pull_ws, pull_exp), _, _ = sr.expectation(win, typ, shape)
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
    """Tuning build, 256 partitions, a 64 KB k_part_agg table: the rows of STDDEV_SAMPLE(x) over a
    BIGINT have 10 words (key, ws, row time, count, sum, the x >> 32 sum, 4 limb words), 84 bytes per
    entry, H = 512.  Push 1 brings 40 000 keys (156 +- 12 per partition, below the split threshold),
    push 2 two records for each of 180 000 keys (703 +- 26 per partition): every partition's table
    overflows on pass 0 and the partition is retried in sub-passes, with the resident words of push 1
    as the sums' seeds.  A failed pass must have written nothing: an add is not idempotent, a
    record applied twice shows in every word."""
    prod = abi.load_product()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    rng = np.random.default_rng(11)
    kw = dict(col_types=["INT64"], aggs=[("STDDEV_SAMPLE", 0), ("COUNT", 0)], capacity_hint=1024)
    g = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    keys1 = rng.permutation(40_000)
    keys2 = rng.permutation(np.repeat(np.arange(RETRY_KEYS), 2))
    allk, allx, allv = [], [], []
    for i, keys in enumerate((keys1, keys2)):
        x = rng.integers(-2**62, 2**62, len(keys))
        v = rng.random(len(keys)) > 0.2
        os.write(2, b"[push %d]\n" % (i + 1))
        st = g.push(abi.HostBatch(np.zeros(len(keys), np.int64), keys=keys, cols=[x], col_valid=[v]))
        os.write(2, b"[push end]\n")
        assert st["windows_applied"] == len(keys)
        allk.append(keys), allx.append(x), allv.append(v)
    snap = g.snapshot()
    g.close()
    keys, x, v = np.concatenate(allk), np.concatenate(allx), np.concatenate(allv)
    st = {}
    for k_, x_, v_ in zip(keys.tolist(), x.tolist(), v.tolist()):
        s = st.setdefault(k_, [0, 0, 0])
        if v_:
            s[0] += 1
            s[1] += x_
            s[2] += x_ * x_
    assert snap["n"] == RETRY_KEYS and snap["key"].tolist() == sorted(st)
    exp = np.array([sr.model_state("STDDEV_SAMPLE", *st[k_]) for k_ in snap["key"].tolist()])
    assert np.array_equal(snap["values"][1], np.array([st[k_][0] for k_ in snap["key"].tolist()]))
    assert np.array_equal(_bits(snap["values"][0]), _bits(exp)) and (exp > 0).sum() > 40_000
    print("OK")


def test_retry_path():
    from test_gpu_c1_retry import TUNE_LIB
    from test_gpu_part_retry import parse_trace
    assert os.path.exists(TUNE_LIB), "tuning build not present (make -C ksql_amd TUNING=1)"
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", KHIP_PART_LOG2=str(RETRY_LOG2P),
               KHIP_LDS_KB=str(RETRY_LDS_KB))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_stddev as t; "
                        "t._retry_child()" % (REPO, os.path.join(REPO, "tests"))], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stderr[-4000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2], (sorted(trace), p.stdout[-2000:], p.stderr[-3000:])
    passes = trace[2]
    # the STDDEV handle ran k_part_agg (never a merge), overflowed its table and went through sub-passes
    assert all(t["kernel"] == "agg" and t["H"] == 512 and t["P"] == 1 << RETRY_LOG2P for t in trace[1] + passes), trace
    assert len(passes) >= 2 and passes[0]["fail_table"] > 0 and passes[0]["sub_items"] == 0, passes
    assert any(t["sub_items"] > 0 for t in passes[1:]) and passes[-1]["failed"] == 0, passes
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------ 5. EMIT FINAL

@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
def test_emit_final(prod, orc, flags):
    """TUMBLING 5 s, grace 0, three pushes: each push's closed windows carry their final values."""
    rng = np.random.default_rng(3)
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0, retention_ms=600_000, col_types=["INT64"],
              aggs=[("STDDEV_SAMPLE", 0), ("COUNT_STAR", -1), ("STDDEV_SAMP", 0)], emit="FINAL")
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=flags, **kw))
    e = sr.Expect(orc, **kw)
    closed = 0
    for b in range(3):
        n = 3000
        ts = b * 6000 + np.sort(rng.integers(0, 6000, n)) + rng.integers(0, 800, n)
        a = dict(ts=ts, keys=rng.integers(0, 50, n), cols=[tr.x_values(rng, n, "INT64")], col_valid=[rng.random(n) > 0.3])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        chg, echg = g.changes(), e.changes()
        tr.assert_same(chg, echg, "closed by push %d" % b)
        closed += chg["n"]
        tr.assert_same(g.snapshot(), e.snapshot(), "push %d" % b)
    assert closed > 100
    g.close()
    e.close()


# ------------------------------------------------------------------ 6. carry

@pytest.mark.parametrize("typ", sr.TYPES)
def test_carry(prod, typ, engine):
    """One unwindowed group of 70 000 x Long.MAX_VALUE and 70 000 x Long.MIN_VALUE (INT: 70 000 x
    2^31 - 1, and 70 000 x -2^31 beside them under a second key): the limb words pass 2^48, the sums
    of the high parts cancel or grow past 2^47, the wrapped BIGINT sum wraps 35 000 times."""
    n = 70_000
    if typ == "INT64":
        x = np.concatenate([np.full(n, I64_MAX), np.full(n, I64_MIN)])
        keys = np.zeros(2 * n, np.int64)
    else:
        x = np.concatenate([np.full(n, 2**31 - 1), np.full(n, 2**31 - 1), np.full(n, -2**31)]).astype(np.int32)
        keys = np.concatenate([np.zeros(n, np.int64), np.ones(2 * n, np.int64)])
    rng = np.random.default_rng(2)
    order = rng.permutation(len(x))
    x, keys = x[order], keys[order]
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=[typ], aggs=[("STDDEV_SAMP", 0), ("STDDEV_SAMPLE", 0), ("COUNT", 0)],
                                              flags=engine))
    half = len(x) // 2
    for lo, hi in ((0, half), (half, len(x))):
        h.push(abi.HostBatch(np.zeros(hi - lo, np.int64), keys=keys[lo:hi], cols=[x[lo:hi]]))
    snap = h.snapshot()
    h.close()
    groups = sorted(set(keys.tolist()))
    assert snap["key"].tolist() == groups
    for r, k in enumerate(groups):
        xs = x[keys == k].tolist()
        assert int(snap["values"][2][r]) == len(xs)
        for a, kind in enumerate(sr.KINDS):
            want = sr.model(kind, xs)
            assert sr.bits(snap["values"][a][r].item()) == sr.bits(want), (typ, k, kind, snap["values"][a][r], want)
            assert want > 0 or (typ == "INT32" and k == 0)  # (the one-valued INT group: exactly 0.0)


# ------------------------------------------------------------------ 7. table source

TAGGS = [("STDDEV_SAMP", 0), ("COUNT", 0), ("SUM", 0), ("STDDEV_SAMPLE", 0), ("STDDEV_SAMPLE", 1), ("COUNT", 1)]


def test_table_source(prod, orc):
    """About 2000 PRIMARY KEYs over 40 groups, 5 pushes of 3000 changes: rows move between groups,
    tombstones delete them, one key changes several times inside a push, and group 39's rows are all
    deleted by the last push (COUNT 0 -> 0.0).  Expected: the source table replayed in a dict, each
    group's live arguments through the model; COUNT(x) / SUM(x) beside them against the oracle."""
    rng = np.random.default_rng(23)
    g = abi.AggHandle(prod, abi.make_agg_desc("NONE", "INT64", col_types=["INT64", "INT32"], aggs=TAGGS, flags=abi.FLAG_TABLE_SOURCE))
    oaggs = [("COUNT", a[1]) if sr.is_var(a) else a for a in TAGGS]
    o = abi.AggHandle(orc, abi.make_agg_desc("NONE", "INT64", col_types=["INT64", "INT32"], aggs=oaggs, flags=abi.FLAG_TABLE_SOURCE))
    table = {}
    for p in range(5):
        n = 3000
        pk = rng.integers(0, 2000, n)
        pk[rng.random(n) < 0.1] = 5  # one key, many changes inside every push
        grp = rng.integers(0, 39, n)
        grp[pk >= 1990] = 39
        live = rng.random(n) > 0.12
        if p == 4:  # the last changes of group 39's keys: tombstones
            tail = np.arange(1990, 2000)
            pk, grp, live = np.concatenate([pk, tail]), np.concatenate([grp, np.full(10, 39)]), np.concatenate([live, np.zeros(10, bool)])
            n += 10
        c0 = tr.x_values(rng, n, "INT64")
        c1 = tr.x_values(rng, n, "INT32")
        cv = [rng.random(n) > 0.1, rng.random(n) > 0.1]
        ts = np.arange(n, dtype=np.int64) + p * 10_000
        stats = [h.push_table(abi.HostBatch(ts, keys=grp, row_valid=live, cols=[c0, c1], col_valid=cv), src_keys=pk)
                 for h in (g, o)]
        assert stats[0] == stats[1]
        for i in range(n):
            if live[i]:
                table[int(pk[i])] = (int(grp[i]), int(c0[i]) if cv[0][i] else None, int(c1[i]) if cv[1][i] else None)
            else:
                table.pop(int(pk[i]), None)
        gs, os_ = g.snapshot(), o.snapshot()
        assert gs["n"] == os_["n"] and np.array_equal(gs["key"], os_["key"]) and np.array_equal(gs["rowtime"], os_["rowtime"])
        for a in (1, 2, 5):
            assert np.array_equal(gs["values"][a], os_["values"][a]), (p, a)
        for r, k in enumerate(gs["key"].tolist()):
            for a, (kind, c) in enumerate(TAGGS):
                if not sr.is_var((kind, c)):
                    continue
                xs = [row[1 + c] for row in table.values() if row[0] == k and row[1 + c] is not None]
                assert len(xs) == int(os_["values"][a][r])  # the oracle's COUNT(x) in its place
                assert not gs["nulls"][a][r]
                assert sr.bits(gs["values"][a][r].item()) == sr.bits(sr.model(kind, xs)), (p, k, kind, c, len(xs))
    r39 = gs["key"].tolist().index(39)
    assert int(gs["values"][1][r39]) == 0 and all(gs["values"][a][r39] == 0.0 for a in (0, 3, 4))
    assert max(int(v) for v in gs["values"][1]) > 20
    g.close()
    o.close()


# ------------------------------------------------------------------ 8. khip_agg_push_shuffled

def test_push_shuffled(prod, orc):
    """One rank: rows packed by the shuffle go through khip_agg_push_shuffled's general route (the
    value pipeline declines a STDDEV handle: order-free, so allowed, unlike the offset kinds) and
    equal the columnar push of the unpacked rows."""
    import torch
    rng = np.random.default_rng(17)
    types = ["INT64", "INT64"]  # user_id (the new GROUP BY key), amount
    kw = dict(col_types=types, aggs=[("STDDEV_SAMPLE", 1)], window_kind="TUMBLING", size_ms=5000, grace_ms=2000)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw))
    u = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    e = sr.Expect(orc, **kw)
    sh = abi.ShuffleHandle(prod, 1, 0, types)
    for p in range(2):
        n = 20_000
        ts = p * 10_000 + (np.arange(n) * 10_000) // n + rng.integers(0, 300, n)
        cols = [rng.integers(0, 500, n), tr.x_values(rng, n, "INT64")]
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


# ------------------------------------------------------------------ 9. rejections and metadata

def _create_status(prod, **kw):
    d = abi.make_agg_desc(**kw)
    h = C.c_void_p()
    st = prod.agg_create(C.byref(d), C.byref(h))
    msg = prod.dll.khip_last_error()
    if st == 0:
        prod.agg_destroy(h)
    return st, msg


@pytest.mark.parametrize("kind", sr.KINDS)
def test_rejections(prod, kind):
    ok = dict(col_types=["INT64"], aggs=[(kind, 0)])
    tumb = dict(window_kind="TUMBLING", size_ms=1000)
    accepted = [ok, dict(ok, col_types=["INT32"]), dict(ok, flags=abi.FLAG_TABLE_SOURCE), dict(ok, flags=abi.FLAG_ENGINE_ATOMIC),
                dict(ok, flags=abi.FLAG_PART_CLAIM), dict(ok, **tumb), dict(ok, emit="FINAL", grace_ms=0, **tumb),
                dict(ok, window_kind="HOPPING", size_ms=1000, advance_ms=500),
                dict(ok, aggs=[(kind, 0), ("COUNT_STAR", -1)], having={"agg": 1, "op": "GT", "value": 1}),
                # 3 + count, sum, hi, 4 limbs per BIGINT column: four columns fill 31 words
                dict(ok, col_types=["INT64"] * 4, aggs=[(kind, c) for c in range(4)])]
    for kw in accepted:
        assert _create_status(prod, **kw)[0] == 0, kw
    cases = [
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["DOUBLE"])),
        (KHIP_E_UNSUPPORTED, dict(ok, window_kind="SESSION", size_ms=1000)),
        (KHIP_E_UNSUPPORTED, dict(ok, having={"agg": 0, "op": "GT", "value": 1})),
        (KHIP_E_INVALID, dict(ok, aggs=[(abi.AGG[kind] | abi.AGG_KEEP_NULLS, 0)])),
        (KHIP_E_INVALID, dict(ok, aggs=[(kind, 0, 3)])),               # k bits
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["INT64"] * 5, aggs=[(kind, c) for c in range(5)])),  # 38 words
    ]
    for want, kw in cases:
        st, msg = _create_status(prod, **kw)
        assert st == want and msg, (kw, st, msg)
    # a HAVING on another aggregate of the query is fine; asked of the STDDEV aggregate later it is not
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64"], aggs=[(kind, 0), ("COUNT_STAR", -1)],
                                              having={"agg": 1, "op": "GT", "value": 1}))
    h.push(abi.HostBatch([1, 2, 3], keys=[5, 5, 6], cols=[np.array([7, 9, 9])]))
    snap = h.snapshot({"agg": 1, "op": "GT", "value": 1})
    assert snap["n"] == 1 and snap["values"][0].tolist() == [sr.model(kind, [7, 9])]
    bad = {"agg": 0, "op": "GT", "value": 1}
    for call in (lambda: h.snapshot(bad), lambda: h.get(keys=[5], having=bad), lambda: h.count_rows(bad)):
        with pytest.raises(abi.KsqlHipError):
            call()
    h.close()


def test_result_len_and_type(prod):
    d = abi.make_agg_desc(col_types=["INT32", "INT64"], aggs=[("STDDEV_SAMP", 0), ("STDDEV_SAMPLE", 1), ("SUM", 0)])
    lens, types = [], []
    for i in range(3):
        v = C.c_int32(-1)
        assert prod.agg_result_len(C.byref(d), i, C.byref(v)) == 0
        lens.append(v.value)
        assert prod.agg_result_type(C.byref(d), i, C.byref(v)) == 0
        types.append(v.value)
    assert lens == [1, 1, 1] == abi.agg_result_len(d)
    assert types == abi.result_types(d) == [abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"], abi.TYPE["INT32"]]


def test_shares_count_and_sum_words(prod):
    """COUNT / SUM / AVG of the column beside both STDDEV kinds: 3 + count + sum + 2 limbs (INT) = 7
    words, an 8-word row; the INT sum word holds the 64-bit sum, which SUM reads truncated."""
    x = np.array([2**31 - 1] * 3 + [5], np.int32)
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[("SUM", 0), ("STDDEV_SAMP", 0), ("AVG", 0), ("COUNT", 0),
                                                                        ("STDDEV_SAMPLE", 0)]))
    h.push(abi.HostBatch(np.zeros(4, np.int64), keys=np.zeros(4, np.int64), cols=[x]))
    snap = h.snapshot()
    h.close()
    xs = x.tolist()
    assert int(snap["values"][0][0]) == ((sum(xs) + 2**31) % 2**32) - 2**31 and int(snap["values"][3][0]) == 4
    assert sr.bits(snap["values"][1][0].item()) == sr.bits(sr.model("STDDEV_SAMP", xs))
    assert sr.bits(snap["values"][4][0].item()) == sr.bits(sr.model("STDDEV_SAMPLE", xs))


# ------------------------------------------------------------------ 10. sink

def test_sink_json(prod):
    """`stddev_sample int` through khip_agg_changes -> khip_sink_encode (JSON): the value bytes are the
    reference's records (the model equals the golden on this case)."""
    case = CASES[IDS.index("stddev_sample int")]
    s = abi.SinkHandle(prod, "KAFKA", [("ID", "INT64")], "JSON", [("STDDEV", "DOUBLE", 0)])
    h = abi.AggHandle(prod, qtt.case_desc(case))
    got = []
    for i in range(len(case["input"])):
        h.push(qtt.case_batch(case, i, i + 1))
        chg = h.changes()
        keys, vals = s.encode(chg, tombstone=chg["tombstone"])
        got += vals
    h.close()
    assert got[1] == b'{"STDDEV":7.0710678118654755}'
    assert [json.loads(v) for v in got] == [o["raw_value"] for o in case["outputs"]]
    assert got == [b'{"STDDEV":%s}' % repr(o["values"][0]).encode() for o in case["outputs"]]
