"""CORRELATION(x, y) over INT / BIGINT pairs on the device, against the reference's QTT cases and the
exact model of tests/correlation_ref.py (the groups' n, Σx, Σy, Σx², Σy², Σxy over the (key, window)
applications the unchanged oracle reports, decoded with one rounding per exact integer).  Every
comparison is bit for bit through the raw 64-bit view: a NaN must be the canonical quiet NaN.

The QTT cases (tests/golden/qtt_correlation.json): correlation int / long.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import correlation_ref as cr
import qtt
import topk_ref as tr
from ksql_amd import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("correlation")
IDS = [c["name"] for c in CASES]
ENGINES = {"part": 0, "part_claim": abi.FLAG_PART_CLAIM, "atomic": abi.FLAG_ENGINE_ATOMIC}
KHIP_E_INVALID, KHIP_E_UNSUPPORTED = -1, -4
EXT = {"INT32": (-2**31, 2**31 - 1), "INT64": (-2**63, 2**63 - 1)}
CORR = ("CORRELATION", 0, 1)


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


@pytest.fixture(params=list(ENGINES), scope="module")
def engine(request):
    return ENGINES[request.param]


def _same_bits(got, want, what):
    assert cr.bits(got) == cr.bits(want), (what, got, want, hex(cr.bits(got)), hex(cr.bits(want)))


# ------------------------------------------------------------------ 1. QTT

def _check_rows(rows, expected):
    """rows: (key, value) from the device; expected: (key, records, golden) — the model's bits, which on
    these cases (inside the exact domain) are the golden's; a NaN by the canonical bits."""
    assert [k for k, _ in rows] == [k for k, _, _ in expected]
    for (key, got), (_, recs, gold) in zip(rows, expected):
        want = cr.model(cr.pairs_of(recs))
        assert cr.same(want, gold)
        _same_bits(got, want, (key, recs))


@pytest.mark.parametrize("split", [None, 1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_correlation_golden(prod, case, split, engine):
    """The final table (the reference's last output per key) from the snapshot."""
    h = abi.AggHandle(prod, cr.case_desc(case, flags=engine, changelog=False))
    n = len(case["input"])
    step = n if not split else split
    for lo in range(0, n, step):
        h.push(qtt.case_batch(case, lo, lo + step))
    snap = h.snapshot()
    h.close()
    assert not snap["nulls"][0].any() and snap["values"][0].dtype == np.float64
    final = {}
    for (key, recs), o in zip(cr.case_sequences(case), case["outputs"]):
        final[key] = (key, recs, o["values"][0])
    _check_rows(list(zip(snap["key"], snap["values"][0].tolist())), [final[k] for k in sorted(final)])


@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_correlation_output_sequence(prod, case, flags):
    """Every output record of the reference, in order, from one-record pushes (a record with a NULL
    argument repeats the row unchanged)."""
    h = abi.AggHandle(prod, cr.case_desc(case, flags=flags))
    rows = []
    for lo in range(len(case["input"])):
        h.push(qtt.case_batch(case, lo, lo + 1))
        chg = h.changes()
        assert not chg["tombstone"].any() and not chg["nulls"][0].any()
        rows += list(zip(chg["key"], chg["values"][0].tolist()))
    h.close()
    _check_rows(rows, [(k, recs, o["values"][0]) for (k, recs), o in zip(cr.case_sequences(case), case["outputs"])])


# ------------------------------------------------------------------ 2. contention

CN = tr.N
CWIN = {"none": dict(window_kind="NONE"), "tumb": dict(window_kind="TUMBLING", size_ms=30_000, grace_ms=0)}
CAGGS = [CORR, ("CORRELATION", 0, 0)]


def _contention_stream(typ):
    """20 000 records on ONE key inside one window, values from the 16 of topk_ref.pool (the type's
    extremes among them), x and y 30 % NULL each: every lane of every wave adds to the same entry."""
    rng = np.random.default_rng(sum(typ.encode()) + 3)
    p = tr.pool(typ)
    return dict(ts=np.sort(rng.integers(0, 25_000, CN)), keys=np.full(CN, 40, np.int64), key_valid=np.ones(CN, bool),
                row_valid=np.ones(CN, bool), cols=[p[rng.integers(0, len(p), CN)], p[rng.integers(0, len(p), CN)]],
                col_valid=[rng.random(CN) > 0.30, rng.random(CN) > 0.30])


@functools.lru_cache(maxsize=None)
def _contention_expectation(win, typ):
    s = _contention_stream(typ)
    e = cr.Expect(abi.load_oracle(), [typ, typ], CAGGS, **CWIN[win])
    e.push(**tr.push_args(s, 0, CN, 2))
    snap = e.snapshot()
    e.close()
    return s, snap


@pytest.mark.parametrize("typ", cr.TYPES)
@pytest.mark.parametrize("win", list(CWIN))
def test_contention(prod, win, typ, engine):
    """One push, then the same stream in pushes of 1, 7, 64 and the rest (resident words seed the
    sums): both equal the model."""
    s, exp = _contention_expectation(win, typ)
    assert exp["n"] == 1 and np.isfinite(exp["values"][0]).all() and exp["values"][1][0] == 1.0
    kw = dict(col_types=[typ, typ], aggs=CAGGS, flags=engine, **CWIN[win])
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(abi.HostBatch(**tr.push_args(s, 0, CN, 2)))
    cr.assert_same(one.snapshot(), exp, "one push")
    one.close()
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    for lo, hi in tr.slices(CN, [1, 7, 64]):
        cut.push(abi.HostBatch(**tr.push_args(s, lo, hi, 2)))
    cr.assert_same(cut.snapshot(), exp, "pushes of 1, 7, 64 and the rest")
    cut.close()


# ------------------------------------------------------------------ 3. random differential

RANDOM = [(win, typ, shape) for win in tr.WINDOWS for typ in cr.TYPES for shape in cr.shapes(typ)]


@pytest.mark.parametrize("win,typ,shape", RANDOM, ids=["-".join(c) for c in RANDOM])
def test_random_vs_expectation(prod, win, typ, shape, engine):
    col_types, aggs, having = cr.query(typ, shape)
    s, per_push, (pull_keys, pull_ws, pull_exp), _, _ = cr.expectation(win, typ, shape)
    emits = engine != abi.FLAG_ENGINE_ATOMIC
    flags = engine | (abi.FLAG_CHANGELOG if emits else 0)
    kw = dict(col_types=col_types, aggs=aggs, flags=flags, having=having, **tr.WINDOWS[win])
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    nc = len(col_types)
    for (lo, hi), (est, esnap, echg) in zip(tr.slices(tr.N, tr.CUTS), per_push):
        st = cut.push(abi.HostBatch(**tr.push_args(s, lo, hi, nc)))
        assert st == est, (lo, hi, st, est)
        cr.assert_same(cut.snapshot(having), esnap, "snapshot after rows [%d, %d)" % (lo, hi))
        if emits:
            cr.assert_same(cut.changes(), echg, "changes of rows [%d, %d)" % (lo, hi))
    got = cut.get(keys=pull_keys, ws=pull_ws)
    cr.assert_same(got, pull_exp, "pull")
    assert got["n"] > 0
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(abi.HostBatch(**tr.push_args(s, 0, tr.N, nc)))
    cr.assert_same(one.snapshot(having), per_push[-1][1], "one push")
    one.close()
    cut.close()


# ------------------------------------------------------------------ 4. retry (child process, tuning build)

RETRY_LOG2P, RETRY_LDS_KB, RETRY_KEYS = 8, 64, 180_000


def _retry_child():
    """Tuning build, 256 partitions, a 64 KB k_part_agg table: the rows of CORRELATION(x, y) over an
    INT pair have 12 words (key, ws, row time, 9 state words), 100 bytes per entry, H = 512.  Push 1
    brings 40 000 keys (156 +- 12 per partition, below the split threshold), push 2 two records for each
    of 180 000 keys (703 +- 26 per partition): every partition's table overflows on pass 0 and the
    partition is retried in sub-passes, with the resident words of push 1 as the sums' seeds.  A
    failed pass must have written nothing: an add is not idempotent, a pair applied twice shows in
    every word (n = 4 would still be finite, but Σ and the count beside it would not match)."""
    prod = abi.load_product()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    rng = np.random.default_rng(12)
    kw = dict(col_types=["INT32", "INT32"], aggs=[CORR, ("COUNT", 0), ("COUNT", 1)], capacity_hint=1024)
    g = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    keys1 = rng.permutation(40_000)
    keys2 = rng.permutation(np.repeat(np.arange(RETRY_KEYS), 2))
    parts = []
    for i, keys in enumerate((keys1, keys2)):
        x, y = tr.x_values(rng, len(keys), "INT32"), tr.x_values(rng, len(keys), "INT32")
        vx, vy = rng.random(len(keys)) > 0.15, rng.random(len(keys)) > 0.15
        os.write(2, b"[push %d]\n" % (i + 1))
        st = g.push(abi.HostBatch(np.zeros(len(keys), np.int64), keys=keys, cols=[x, y], col_valid=[vx, vy]))
        os.write(2, b"[push end]\n")
        assert st["windows_applied"] == len(keys)
        parts.append((keys, x, y, vx, vy))
    snap = g.snapshot()
    g.close()
    keys, x, y, vx, vy = (np.concatenate([p[i] for p in parts]) for i in range(5))
    st = {}
    for k_, x_, y_, a_, b_ in zip(keys.tolist(), x.tolist(), y.tolist(), vx.tolist(), vy.tolist()):
        s = st.setdefault(k_, [[0] * 6, 0, 0])
        s[1] += a_
        s[2] += b_
        if a_ and b_:
            for i, v in enumerate((1, x_, y_, x_ * x_, y_ * y_, x_ * y_)):
                s[0][i] += v
    assert snap["n"] == RETRY_KEYS and snap["key"].tolist() == sorted(st)
    order = snap["key"].tolist()
    exp = np.array([cr.model_state(*st[k_][0]) for k_ in order])
    assert np.array_equal(snap["values"][1], np.array([st[k_][1] for k_ in order]))
    assert np.array_equal(snap["values"][2], np.array([st[k_][2] for k_ in order]))
    assert np.array_equal(cr.raw_bits(snap["values"][0]), cr.raw_bits(exp)) and np.isfinite(exp).sum() > 40_000
    print("OK")


def test_retry_path():
    from test_gpu_c1_retry import TUNE_LIB
    from test_gpu_part_retry import parse_trace
    assert os.path.exists(TUNE_LIB), "tuning build not present (make -C ksql_amd TUNING=1)"
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", KHIP_PART_LOG2=str(RETRY_LOG2P),
               KHIP_LDS_KB=str(RETRY_LDS_KB))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_correlation as t; "
                        "t._retry_child()" % (REPO, os.path.join(REPO, "tests"))], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stderr[-4000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2], (sorted(trace), p.stdout[-2000:], p.stderr[-3000:])
    passes = trace[2]
    # the CORRELATION handle ran k_part_agg (never a merge), overflowed its table and went through sub-passes
    assert all(t["kernel"] == "agg" and t["H"] == 512 and t["P"] == 1 << RETRY_LOG2P for t in trace[1] + passes), trace
    assert len(passes) >= 2 and passes[0]["fail_table"] > 0 and passes[0]["sub_items"] == 0, passes
    assert any(t["sub_items"] > 0 for t in passes[1:]) and passes[-1]["failed"] == 0, passes
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------ 5. EMIT FINAL

@pytest.mark.parametrize("flags", [0, abi.FLAG_PART_CLAIM], ids=["part", "part_claim"])
def test_emit_final(prod, orc, flags):
    """TUMBLING 5 s, grace 0, three pushes: each push's closed windows carry their final values."""
    rng = np.random.default_rng(3)
    kw = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0, retention_ms=600_000, col_types=["INT64", "INT64"],
              aggs=[CORR, ("COUNT_STAR", -1)], emit="FINAL")
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=flags, **kw))
    e = cr.Expect(orc, **kw)
    closed = 0
    for b in range(3):
        n = 3000
        ts = b * 6000 + np.sort(rng.integers(0, 6000, n)) + rng.integers(0, 800, n)
        a = dict(ts=ts, keys=rng.integers(0, 50, n), cols=[tr.x_values(rng, n, "INT64"), tr.x_values(rng, n, "INT64")],
                 col_valid=[rng.random(n) > 0.3, rng.random(n) > 0.3])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        chg, echg = g.changes(), e.changes()
        cr.assert_same(chg, echg, "closed by push %d" % b)
        closed += chg["n"]
        cr.assert_same(g.snapshot(), e.snapshot(), "push %d" % b)
    assert closed > 100
    g.close()
    e.close()


# ------------------------------------------------------------------ 6. carry

def _carry_rows(typ):
    """A handful of records of the extremes in all four sign combinations, 3 x 40 of them: every limb
    word crosses 2^32 (a limb near 2^32 added three times), the signed top words go negative (MIN x
    MAX) and back (MIN x MIN), the low-limb sums of a negative product carry."""
    lo, hi = EXT[typ]
    quad = [(lo, lo), (lo, hi), (hi, lo), (hi, hi), (lo + 1, hi - 1), (-1, 1), (hi, -1), (0, lo)]
    return quad * 15


@pytest.mark.parametrize("typ", cr.TYPES)
def test_carry(prod, typ, engine):
    rows = _carry_rows(typ)
    rng = np.random.default_rng(2)
    order = rng.permutation(len(rows))
    dt = abi.NP_TYPE[abi.TYPE[typ]]
    x, y = np.array([rows[i][0] for i in order], dt), np.array([rows[i][1] for i in order], dt)
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=[typ, typ], aggs=[CORR, ("CORRELATION", 1, 0), ("COUNT_STAR", -1)],
                                              flags=engine))
    seen = []
    for lo, hi in tr.slices(len(rows), [1, 2, 4, 5, 40]):  # the running state after every push: words go up and down
        h.push(abi.HostBatch(np.zeros(hi - lo, np.int64), keys=np.zeros(hi - lo, np.int64), cols=[x[lo:hi], y[lo:hi]]))
        snap = h.snapshot()
        pairs = list(zip(x[:hi].tolist(), y[:hi].tolist()))
        want = cr.model(pairs)
        assert int(snap["values"][2][0]) == hi
        for a in (0, 1):
            _same_bits(snap["values"][a][0].item(), want, (typ, hi, a))
        seen.append(want)
    h.close()
    assert any(v != v for v in seen) and any(v < 0 for v in seen) and np.isfinite(seen[-1])


@pytest.mark.parametrize("typ", cr.TYPES)
def test_carry_table_source(prod, typ):
    """The same rows as upserts of distinct PRIMARY KEYs, then every other row deleted again."""
    rows = _carry_rows(typ)
    dt = abi.NP_TYPE[abi.TYPE[typ]]
    x, y = np.array([r[0] for r in rows], dt), np.array([r[1] for r in rows], dt)
    n = len(rows)
    h = abi.AggHandle(prod, abi.make_agg_desc("NONE", "INT64", col_types=[typ, typ], aggs=[CORR, ("COUNT_STAR", -1)],
                                              flags=abi.FLAG_TABLE_SOURCE))
    h.push_table(abi.HostBatch(np.arange(n), keys=np.zeros(n, np.int64), cols=[x, y]), src_keys=np.arange(n))
    snap = h.snapshot()
    _same_bits(snap["values"][0][0].item(), cr.model(rows), (typ, "upserts"))
    gone = np.arange(0, n, 2)
    h.push_table(abi.HostBatch(np.arange(len(gone)) + n, keys=np.zeros(len(gone), np.int64), row_valid=np.zeros(len(gone), bool),
                               cols=[x[gone], y[gone]]), src_keys=gone)
    snap = h.snapshot()
    h.close()
    assert int(snap["values"][1][0]) == n - len(gone)
    _same_bits(snap["values"][0][0].item(), cr.model([r for i, r in enumerate(rows) if i % 2]), (typ, "deletes"))


# ------------------------------------------------------------------ 7. table source

TAGGS = [CORR, ("COUNT", 0), ("SUM", 0), ("CORRELATION", 2, 2), ("COUNT", 1), ("CORRELATION", 1, 0)]


def test_table_source(prod, orc):
    """About 2000 PRIMARY KEYs over 40 groups, 5 pushes of 3000 changes: rows move between groups,
    tombstones delete them, x alone changes (every fourth change keeps the key's previous y), y turns
    NULL and back, one key changes several times inside a push, and group 39's rows are all deleted
    by the last push (no pair: NaN again).  Expected: the source table replayed in a dict, each
    group's live pairs through the model; COUNT / SUM beside them against the oracle."""
    rng = np.random.default_rng(29)
    types = ["INT64", "INT64", "INT32"]
    g = abi.AggHandle(prod, abi.make_agg_desc("NONE", "INT64", col_types=types, aggs=TAGGS, flags=abi.FLAG_TABLE_SOURCE))
    oaggs = [("COUNT", a[1]) if cr.is_corr(a) else a for a in TAGGS]
    o = abi.AggHandle(orc, abi.make_agg_desc("NONE", "INT64", col_types=types, aggs=oaggs, flags=abi.FLAG_TABLE_SOURCE))
    table, x_only, y_flips = {}, 0, 0
    for p in range(5):
        n = 3000
        pk = rng.integers(0, 2000, n)
        pk[rng.random(n) < 0.1] = 5  # one key, many changes inside every push
        grp = np.where(rng.random(n) < 0.2, rng.integers(0, 39, n), pk % 39)  # a key mostly stays in its group
        grp[pk >= 1990] = 39
        live = rng.random(n) > 0.12
        if p == 4:  # the last changes of group 39's keys: tombstones
            tail = np.arange(1990, 2000)
            pk, grp, live = np.concatenate([pk, tail]), np.concatenate([grp, np.full(10, 39)]), np.concatenate([live, np.zeros(10, bool)])
            n += 10
        c0, c1, c2 = tr.x_values(rng, n, "INT64"), tr.x_values(rng, n, "INT64"), tr.x_values(rng, n, "INT32")
        cv = [rng.random(n) > 0.1, rng.random(n) > 0.25, rng.random(n) > 0.1]
        keep_y = rng.random(n) < 0.25
        ts = np.arange(n, dtype=np.int64) + p * 10_000
        for i in range(n):  # (before the push: a change that keeps y needs the key's current row)
            k = int(pk[i])
            if not live[i]:
                table.pop(k, None)
                continue
            old = table.get(k)
            if old is not None and keep_y[i] and old[0] == int(grp[i]):
                c1[i], cv[1][i] = (0 if old[2] is None else old[2]), old[2] is not None
                x_only += 1
            new = (int(grp[i]), int(c0[i]) if cv[0][i] else None, int(c1[i]) if cv[1][i] else None, int(c2[i]) if cv[2][i] else None)
            if old is not None and old[0] == new[0] and (old[2] is None) != (new[2] is None):
                y_flips += 1
            table[k] = new
        stats = [h.push_table(abi.HostBatch(ts, keys=grp, row_valid=live, cols=[c0, c1, c2], col_valid=cv), src_keys=pk)
                 for h in (g, o)]
        assert stats[0] == stats[1]
        gs, os_ = g.snapshot(), o.snapshot()
        assert gs["n"] == os_["n"] and np.array_equal(gs["key"], os_["key"]) and np.array_equal(gs["rowtime"], os_["rowtime"])
        for a in (1, 2, 4):
            assert np.array_equal(gs["values"][a], os_["values"][a]), (p, a)
        for r, k in enumerate(gs["key"].tolist()):
            for a, agg in enumerate(TAGGS):
                if not cr.is_corr(agg):
                    continue
                pairs = cr.pairs_of([(row[1 + agg[1]], row[1 + agg[2]]) for row in table.values() if row[0] == k])
                assert not gs["nulls"][a][r]
                _same_bits(gs["values"][a][r].item(), cr.model(pairs), (p, k, agg, len(pairs)))
    r39 = gs["key"].tolist().index(39)
    assert int(gs["values"][1][r39]) == 0 and all(cr.bits(gs["values"][a][r39].item()) == cr.NAN_BITS for a in (0, 3, 5))
    assert np.isfinite(gs["values"][0]).sum() > 20 and x_only > 500 and y_flips > 200
    g.close()
    o.close()


# ------------------------------------------------------------------ 8. khip_agg_push_shuffled

def test_push_shuffled(prod, orc):
    """One rank: rows packed by the shuffle go through khip_agg_push_shuffled's general route (the
    value pipeline declines a CORRELATION handle: order-free, so allowed, like STDDEV) and equal the
    columnar push of the unpacked rows."""
    import torch
    rng = np.random.default_rng(18)
    types = ["INT64", "INT64", "INT64"]  # user_id (the new GROUP BY key), x, y
    kw = dict(col_types=types, aggs=[("CORRELATION", 1, 2)], window_kind="TUMBLING", size_ms=5000, grace_ms=2000)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw))
    u = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    e = cr.Expect(orc, **kw)
    sh = abi.ShuffleHandle(prod, 1, 0, types)
    for p in range(2):
        n = 20_000
        ts = p * 10_000 + (np.arange(n) * 10_000) // n + rng.integers(0, 300, n)
        cols = [rng.integers(0, 500, n), tr.x_values(rng, n, "INT64"), tr.x_values(rng, n, "INT64")]
        valid = [rng.random(n) > 0.05, rng.random(n) > 0.3, rng.random(n) > 0.3]
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
        cr.assert_same(g.snapshot(), e.snapshot(), "shuffled, push %d" % p)
        cr.assert_same(u.snapshot(), e.snapshot(), "unpacked, push %d" % p)
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


def test_rejections(prod):
    ok = dict(col_types=["INT64", "INT64"], aggs=[CORR])
    tumb = dict(window_kind="TUMBLING", size_ms=1000)
    accepted = [ok, dict(ok, col_types=["INT32", "INT32"]), dict(ok, flags=abi.FLAG_TABLE_SOURCE), dict(ok, flags=abi.FLAG_ENGINE_ATOMIC),
                dict(ok, flags=abi.FLAG_PART_CLAIM), dict(ok, **tumb), dict(ok, emit="FINAL", grace_ms=0, **tumb),
                dict(ok, window_kind="HOPPING", size_ms=1000, advance_ms=500),
                dict(ok, aggs=[("CORRELATION", 1, 0)]), dict(ok, aggs=[("CORRELATION", 1, 1)]),   # y = column 0; x == y
                dict(ok, aggs=[CORR, ("COUNT_STAR", -1)], having={"agg": 1, "op": "GT", "value": 1}),
                dict(ok, time_domain="SUPPLIED", **tumb),
                # 17 words of the pair, none for (y, x), 11 for (x, x), COUNT(*)
                dict(ok, aggs=[CORR, ("CORRELATION", 1, 0), ("CORRELATION", 0, 0), ("COUNT_STAR", -1)]),   # 29 words
                dict(ok, col_types=["INT32"] * 4, aggs=[CORR, ("CORRELATION", 2, 3), ("CORRELATION", 0, 2)])]  # 27 words
    for kw in accepted:
        assert _create_status(prod, **kw)[0] == 0, kw
    cases = [
        (KHIP_E_INVALID, dict(ok, aggs=[("CORRELATION", 0, 2)])),                                    # y out of range
        (KHIP_E_INVALID, dict(ok, aggs=[("CORRELATION", 0, -1)])),
        (KHIP_E_INVALID, dict(ok, aggs=[("CORRELATION", 2, 0)])),                                    # x out of range
        (KHIP_E_INVALID, dict(ok, aggs=[(abi.AGG["CORRELATION"] | abi.AGG_KEEP_NULLS, 0, 1)])),
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["DOUBLE", "DOUBLE"])),
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["INT64", "DOUBLE"])),
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["INT32", "INT64"])),                                # mixed: the caller casts
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["INT64", "INT32"])),
        (KHIP_E_UNSUPPORTED, dict(ok, window_kind="SESSION", size_ms=1000)),
        (KHIP_E_UNSUPPORTED, dict(ok, having={"agg": 0, "op": "GT", "value": 0})),
        # the GPU tests' BIGINT "beside" list in one query: 11 + 17 + 11 = 39 words
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=cr.BESIDE)),
        (KHIP_E_UNSUPPORTED, dict(ok, col_types=["INT64"] * 3, aggs=[CORR, ("CORRELATION", 1, 2)])),  # 34 words
    ]
    for want, kw in cases:
        st, msg = _create_status(prod, **kw)
        assert st == want and msg, (kw, st, msg)
    # a HAVING on another aggregate of the query is fine; asked of the CORRELATION aggregate later it is not
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64", "INT64"], aggs=[CORR, ("COUNT_STAR", -1)],
                                              having={"agg": 1, "op": "GT", "value": 2}))
    h.push(abi.HostBatch([1, 2, 3, 4], keys=[5, 5, 5, 6], cols=[np.array([7, 9, 8, 1]), np.array([1, 5, 2, 1])]))
    snap = h.snapshot({"agg": 1, "op": "GT", "value": 2})
    assert snap["n"] == 1 and snap["values"][0].tolist() == [cr.model([(7, 1), (9, 5), (8, 2)])]
    bad = {"agg": 0, "op": "GT", "value": 0}
    for call in (lambda: h.snapshot(bad), lambda: h.get(keys=[5], having=bad), lambda: h.count_rows(bad)):
        with pytest.raises(abi.KsqlHipError):
            call()
        assert prod.dll.khip_last_error()
    h.close()


def test_result_len_and_type(prod):
    d = abi.make_agg_desc(col_types=["INT32", "INT32", "INT64"], aggs=[CORR, ("CORRELATION", 2, 2), ("SUM", 0)])
    lens, types = [], []
    for i in range(3):
        v = C.c_int32(-1)
        assert prod.agg_result_len(C.byref(d), i, C.byref(v)) == 0
        lens.append(v.value)
        assert prod.agg_result_type(C.byref(d), i, C.byref(v)) == 0
        types.append(v.value)
    assert lens == [1, 1, 1] == abi.agg_result_len(d)
    assert types == abi.result_types(d) == [abi.TYPE["DOUBLE"], abi.TYPE["DOUBLE"], abi.TYPE["INT32"]]


def test_word_sharing(prod):
    """What is implemented (DESIGN.md "CORRELATION aggregate"): an identical spec adds no state words,
    CORRELATION(y, x) shares every word of CORRELATION(x, y), CORRELATION(x, x) keeps 6 (INT) / 11
    (BIGINT); none is shared with COUNT / SUM / STDDEV of a column.  Measured by what still fits the 29
    words of a row: a BIGINT pair takes 17, so a second, different pair does not fit, but any number of
    copies and the swapped spec do."""
    big = dict(col_types=["INT64"] * 3)
    assert _create_status(prod, aggs=[CORR] * 8 + [("CORRELATION", 1, 0)] * 8, **big)[0] == 0           # 17 words
    assert _create_status(prod, aggs=[CORR, ("CORRELATION", 0, 2)], **big)[0] == KHIP_E_UNSUPPORTED    # 34
    assert _create_status(prod, aggs=[CORR, ("CORRELATION", 0, 0), ("COUNT_STAR", -1)], **big)[0] == 0  # 17 + 11 + 1
    assert _create_status(prod, aggs=[CORR, ("CORRELATION", 0, 0), ("COUNT_STAR", -1), ("COUNT", 0)],
                          **big)[0] == KHIP_E_UNSUPPORTED                                               # 30: COUNT(x) is its own word
    # 17 + STDDEV(x)'s count, sum, hi, 4 limbs = 24; SUM(x) and AVG(x) share STDDEV's; + 5 more counts = 29
    fit = [CORR, ("STDDEV_SAMP", 0), ("SUM", 0), ("AVG", 0), ("COUNT", 1), ("COUNT", 2), ("COUNT_STAR", -1), ("MAX", 2), ("MIN", 2)]
    assert _create_status(prod, aggs=fit, **big)[0] == 0
    assert _create_status(prod, aggs=fit + [("SUM", 1)], **big)[0] == KHIP_E_UNSUPPORTED
    # and the values: the copies agree, COUNT(x) / SUM(x) keep counting the records whose y is NULL
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT32", "INT32"], aggs=[CORR, ("COUNT", 0), CORR, ("SUM", 0),
                                                                                 ("CORRELATION", 1, 0), ("COUNT", 1)]))
    x, y = np.array([1, -1, -4, 13, 5], np.int32), np.array([8, -2, -1, 0, -6], np.int32)
    h.push(abi.HostBatch(np.zeros(5, np.int64), keys=np.zeros(5, np.int64), cols=[x, y],
                         col_valid=[[True, True, True, True, False], [True, True, True, False, True]]))
    snap = h.snapshot()
    h.close()
    assert [int(snap["values"][a][0]) for a in (1, 3, 5)] == [4, 9, 4]
    assert [snap["values"][a][0] for a in (0, 2, 4)] == [0.7455284088780169] * 3


# ------------------------------------------------------------------ 10. sink

def test_sink_json(prod):
    """`correlation int` through khip_agg_changes -> khip_sink_encode (JSON): the value bytes are the
    reference's records; a NaN is written as the sink writes any DOUBLE NaN (the JSON string "NaN")."""
    case = CASES[IDS.index("correlation int")]
    s = abi.SinkHandle(prod, "KAFKA", [("ID", "STRING")], "JSON", [("CORRELATION", "DOUBLE", 0)])
    h = abi.AggHandle(prod, cr.case_desc(case))
    got = []
    for i in range(len(case["input"])):
        h.push(qtt.case_batch(case, i, i + 1))
        chg = h.changes()
        keys, vals = s.encode(chg, tombstone=chg["tombstone"])
        got += vals
    h.close()
    assert got[0] == b'{"CORRELATION":"NaN"}' and got[3] == b'{"CORRELATION":0.7455284088780169}'
    assert [json.loads(v) for v in got] == [o["raw_value"] for o in case["outputs"]]
