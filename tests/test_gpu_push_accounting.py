"""What a push accounts for besides its results: the profile counters bench.py divides by
(kernel_times()["records"], ["apply_launches"], dict_ms), the statistics of every entry point, and the
empty pushes.  The parity tests compare tables; none of them looks at these.

Handles: FLAG_PROFILE, TUMBLING 5000 ms (grace 1000), INT64 keys, COUNT(*) + SUM(BIGINT); pushes of
4096 rows over 200 keys, timestamps advancing 20 s per push, so every push after the first closes
windows.  Engine 0 adds `records` and one apply launch per push; engine 1 adds the records on its
first pass and a launch per pass (a resume pass after a table doubling is legal: >=).

Every case is a function of (prod, orc), so that one case can also be run alone under a profiler."""
import numpy as np
import pytest

from ksql_amd import abi
from test_gpu_parity import assert_snap_equal
from test_gpu_time_domains import _np_stream_time

pytestmark = pytest.mark.gpu

N, KEYS, PUSHES = 4096, 200, 3
Q = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=1000, col_types=["INT64"],
         aggs=[("COUNT_STAR", -1), ("SUM", 0)])
HINT0, HINT1 = 1 << 16, 16 * 4096  # engine 1: 16 x the groups (200 keys x 13 windows = 2600 < 4096)
HINT_ROWS = 1 << 22  # the value pipeline needs 2048 partitions or more (c1v_eligible), as in test_gpu_push_shuffled.py


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


def _columns():
    """The three pushes as numpy columns: (keys, ts, values, value validity)."""
    rng = np.random.default_rng(20)
    out = []
    for b in range(PUSHES):
        ts = 20_000 * b + np.sort(rng.integers(0, 20_000, N)) + rng.integers(0, 400, N)
        out.append((rng.integers(0, KEYS, N), ts, rng.integers(-1 << 40, 1 << 40, N), rng.random(N) > 0.03))
    return out


def _host(c):
    return abi.HostBatch(c[1], keys=c[0], cols=[c[2]], col_valid=[c[3]])


def _device(c):
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return abi.DeviceBatch(d(c[1]), keys=d(c[0]), cols=[d(c[2])], col_valid=[abi.bitmap_torch(d(c[3]))])


def _utf8_key(k):
    """Even keys: up to 17 digits (inline ids); odd keys: longer (the dictionary)."""
    return str(10**9 + k) if k % 2 == 0 else "key-%020d" % k


def _utf8(c):
    return abi.HostBatch(c[1], utf8_keys=[_utf8_key(int(k)) for k in c[0]], cols=[c[2]], col_valid=[c[3]])


def _empty(utf8=False):
    z = np.zeros(0, np.int64)
    return abi.HostBatch(z, utf8_keys=[], cols=[z]) if utf8 else abi.HostBatch(z, keys=z, cols=[z])


def _pushes(lib, batches, flags=0, hint=HINT0, **kw):
    """Push the batches into a fresh handle: ([(stats, snapshot)] per push, kernel times, desc)."""
    desc = abi.make_agg_desc(flags=flags, capacity_hint=hint, **dict(Q, **kw))
    h = abi.AggHandle(lib, desc)
    out = [(h.push(b), h.snapshot()) for b in batches]
    kt = h.kernel_times() if flags & abi.FLAG_PROFILE else None
    h.close()
    return out, kt, desc


def _assert_same(got, exp, desc):
    assert len(got) == len(exp)
    for i, ((gs, gsnap), (es, esnap)) in enumerate(zip(got, exp)):
        assert gs == es, (i, gs, es)
        assert_snap_equal(gsnap, esnap, desc)


def case_engine0_host(prod, orc):
    cols = _columns()
    got, kt, desc = _pushes(prod, [_host(c) for c in cols], abi.FLAG_PROFILE)
    exp, _, _ = _pushes(orc, [_host(c) for c in cols])
    assert kt["records"] == PUSHES * N and kt["apply_launches"] == PUSHES, kt
    _assert_same(got, exp, desc)
    assert got[-1][0]["windows_applied"] > 0 and got[-1][1]["n"] > KEYS  # several windows per key


def case_engine0_device(prod, orc):
    cols = _columns()
    host, hkt, desc = _pushes(prod, [_host(c) for c in cols], abi.FLAG_PROFILE)
    dev, dkt, _ = _pushes(prod, [_device(c) for c in cols], abi.FLAG_PROFILE)
    assert dkt["records"] == hkt["records"] == PUSHES * N, (dkt, hkt)
    assert dkt["apply_launches"] == hkt["apply_launches"] == PUSHES, (dkt, hkt)
    _assert_same(dev, host, desc)


def case_engine0_utf8(prod, orc):
    cols = _columns()
    got, kt, desc = _pushes(prod, [_utf8(c) for c in cols], abi.FLAG_PROFILE, key_type="UTF8")
    exp, _, _ = _pushes(orc, [_utf8(c) for c in cols], key_type="UTF8")
    assert kt["records"] == PUSHES * N and kt["apply_launches"] == PUSHES, kt
    assert kt["dict_ms"] > 0, kt
    _assert_same(got, exp, desc)


def case_engine1(prod, orc):
    cols = _columns()
    got, kt, desc = _pushes(prod, [_host(c) for c in cols], abi.FLAG_PROFILE | abi.FLAG_ENGINE_ATOMIC, hint=HINT1)
    exp, _, _ = _pushes(orc, [_host(c) for c in cols])
    assert kt["records"] == PUSHES * N and kt["apply_launches"] >= PUSHES, kt
    _assert_same(got, exp, desc)


def _case_empty(prod, flags, hint):
    cols = _columns()
    h = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE | flags, capacity_hint=hint, **Q))
    s0 = h.push(_host(cols[0]))
    snap0, kt0 = h.snapshot(), h.kernel_times()
    se = h.push(_empty())
    assert se["rows_in"] == 0 and se["stream_time"] == s0["stream_time"], (se, s0)
    assert se == dict(s0, rows_in=0, rows_accepted=0, windows_applied=0, windows_late=0,
                      dropped_null_key=0, dropped_null_row=0, dropped_bad_ts=0), (se, s0)
    kt1 = h.kernel_times()
    assert (kt1["records"], kt1["apply_launches"]) == (kt0["records"], kt0["apply_launches"]) == (N, kt0["apply_launches"])
    assert_snap_equal(h.snapshot(), snap0, h.desc)
    if flags & abi.FLAG_CHANGELOG:
        assert h.changes()["n"] == 0
    s1 = h.push(_host(cols[1]))
    assert s1["rows_in"] == N and s1["stream_time"] > s0["stream_time"]
    kt2 = h.kernel_times()
    assert kt2["records"] == 2 * N and kt2["apply_launches"] > kt1["apply_launches"], kt2
    if flags & abi.FLAG_CHANGELOG:
        assert h.changes()["n"] > 0
    h.close()


def case_empty_engine0(prod, orc):
    _case_empty(prod, abi.FLAG_CHANGELOG, HINT0)


def case_empty_engine1(prod, orc):
    _case_empty(prod, abi.FLAG_ENGINE_ATOMIC, HINT1)


def _case_shuffled(prod, win, late, pipeline):
    """One rank: the packed rows through khip_agg_push_shuffled (profiled handle) and, unpacked,
    through khip_agg_push; SUM(BIGINT) alone is the value pipeline's query.  late: records four spans
    back, which (grace 0) the pipeline declines."""
    from test_gpu_push_shuffled import _dev, _source
    types = ["INT64", "INT64"]
    kw = dict(key_type="INT64", col_types=types, aggs=[("SUM", 1)], capacity_hint=HINT_ROWS, **win)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_PROFILE, **kw))
    u = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    sh = abi.ShuffleHandle(prod, 1, 0, types)
    rng = np.random.default_rng(21 + pipeline)
    rows = 0
    for p in range(PUSHES):
        ts, cols, valid = _source(rng, N, KEYS, 20_000, 20_000 * p, types, late=late)
        cols[0] = rng.integers(0, KEYS, N)
        send, counts = sh.pack(_dev(ts, cols, valid, types))
        m = int(sum(counts))
        gs = g.push_shuffled(sh, send, m)
        key, kts, ucols, uvalid = sh.unpack(send, m)
        us = u.push(abi.DeviceBatch(kts, keys=key, cols=ucols, col_valid=uvalid))
        assert gs == us, (p, gs, us)
        rows += m
        kt = g.kernel_times()
        assert kt["records"] == rows and kt["apply_launches"] == p + 1, (p, kt)
    assert 0 < rows <= PUSHES * N
    assert (kt["c1_pushes"] == PUSHES) == pipeline, kt
    assert_snap_equal(g.snapshot(), u.snapshot(), g.desc)
    for h in (g, u, sh):
        h.close()


def case_shuffled_pipeline(prod, orc):
    _case_shuffled(prod, dict(window_kind="TUMBLING", size_ms=5000), 0.0, True)


def case_shuffled_declined(prod, orc):
    _case_shuffled(prod, dict(window_kind="TUMBLING", size_ms=5000, grace_ms=0), 0.02, False)


SIZE, GRACE = 5000, 1000  # EMIT FINAL: retention = size + grace


def _np_lost(ts, valid, seed):
    """k_emit_lost's rule, record by record (khip_agg.hip): a record that moves the stream time from mp
    to t into a later advance bucket loses the window starts in
    [mp - size - grace + 1 rounded up to the advance, min(t - size - grace, bucket start - retention - 1)]."""
    sg, adv, ret, mp, out = SIZE + GRACE, SIZE, SIZE + GRACE, seed, []
    for t, v in zip(ts.tolist(), valid.tolist()):
        if not v or t <= mp:
            continue
        if t // adv > (-1 if mp < 0 else mp // adv):
            lo = -(-max(mp - sg + 1, 0) // adv) * adv
            hi = min(t - sg, t // adv * adv - ret - 1)
            if lo <= hi:
                out.append((lo, hi))
        mp = t
    merged = []
    for lo, hi in sorted(out):
        if merged and lo <= merged[-1][1] + 1:
            merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
        else:
            merged.append((lo, hi))
    return merged


def case_lost_windows_and_scan(prod, orc):
    """4096 ordered rows whose last 64 jump 100 s ahead: the window that was open at the jump closes
    after it expired.  Host batch = device batch = the numpy rules; and the oracle's EMIT FINAL task
    emits every closed window with records but the ones in the lost ranges."""
    import torch
    rng = np.random.default_rng(22)
    ts = np.sort(rng.integers(0, 20_000, N))
    ts[-64:] += 100_000
    keys, kv, seed = rng.integers(0, KEYS, N), rng.random(N) > 0.03, -1
    vals = rng.integers(0, 1000, N)
    kw = dict(Q, emit="FINAL", capacity_hint=HINT0)
    h = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    hb = abi.HostBatch(ts, keys=keys, key_valid=kv, cols=[vals])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    db = abi.DeviceBatch(d(ts), keys=d(keys), key_valid=abi.bitmap_torch(d(kv)), cols=[d(vals)])
    # the stream time at every row
    ref = _np_stream_time(ts, kv, seed)
    hout, hmx = h.stream_time_scan(hb, seed)
    dout, dmx = h.stream_time_scan(db, seed, out=torch.empty(N, dtype=torch.int64, device="cuda"))
    assert np.array_equal(hout, ref) and np.array_equal(dout.cpu().numpy(), ref)
    assert hmx == dmx == ref[-1]
    # the lost window starts
    hl, dl = h.lost_windows(hb, seed), h.lost_windows(db, seed)
    assert hl == dl == _np_lost(ts, kv, seed) and len(hl) >= 1, (hl, dl)
    h.close()
    o = abi.AggHandle(orc, abi.make_agg_desc(**kw))
    o.push(hb)
    emitted = set(o.changes()["ws"].tolist())
    o.close()
    ws = set((ts[kv] // SIZE * SIZE).tolist())
    closed = {w for w in ws if w + SIZE + GRACE <= ref[-1]}
    in_lost = {w for w in closed if any(lo <= w <= hi for lo, hi in hl)}
    assert in_lost and closed - emitted == in_lost, (sorted(closed), sorted(emitted), hl)


CASES = [case_engine0_host, case_engine0_device, case_engine0_utf8, case_engine1, case_empty_engine0,
         case_empty_engine1, case_shuffled_pipeline, case_shuffled_declined, case_lost_windows_and_scan]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_push_accounting(prod, orc, case):
    case(prod, orc)
