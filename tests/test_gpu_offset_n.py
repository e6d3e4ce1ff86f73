"""The N forms LATEST_BY_OFFSET(col, N[, ignoreNulls]) / EARLIEST_BY_OFFSET(col, N[, ignoreNulls]) on
the device, against the reference's QTT cases and the oracle-derived expectation of
tests/offset_n_ref.py (latestTN / earliestTN.aggregate restated on Python lists, folded over the
(key, window) applications the unchanged oracle reports).  Every comparison is bit for bit (a
DOUBLE's int64 view: NaN payloads, -0.0) and checks the null bytes exactly: 0 present, 1 past the
end, 2 a NULL element.

The QTT cases (tests/golden/qtt_offset_n.json): the twelve non-SESSION N-form cases of
latest-offset-udaf.json / earliest-offset-udaf.json.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import offset_n_ref as nr
import qtt
import topk_ref as tr
from ksql_amd import abi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = qtt.load_cases("offset_n")
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
    per_agg = [nr.lists_of(snap, i) for i in range(len(case["desc"]["aggs"]))]
    return [(int(snap["key"][r]), [per_agg[i][r] for i in range(len(per_agg))]) for r in range(snap["n"])]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_one_push(prod, case, engine):
    """The final table (the reference's last output per key) from one push."""
    h = abi.AggHandle(prod, nr.case_desc(case, flags=engine, changelog=False))
    h.push(qtt.case_batch(case))
    snap = h.snapshot()
    h.close()
    assert _case_lists(case, snap) == sorted(dict(nr.golden_outputs(case)).items())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_qtt_output_sequence(prod, case, engine):
    """Every output record of the reference, in order, from one-record pushes: EMIT CHANGES on the
    partitioned engines, the snapshot's row of the record's key on the global-atomic engine (it
    keeps no changelog)."""
    emits = engine != abi.FLAG_ENGINE_ATOMIC
    h = abi.AggHandle(prod, nr.case_desc(case, flags=engine, changelog=emits))
    rows = []
    for lo, r in enumerate(case["input"]):
        h.push(qtt.case_batch(case, lo, lo + 1))
        if emits:
            chg = h.changes()
            assert not chg["tombstone"].any()
            rows += _case_lists(case, chg)
        elif r["key"] is not None and r["row_valid"] and r["ts"] >= 0:
            rows += [x for x in _case_lists(case, h.snapshot()) if x[0] == r["key"]]
    h.close()
    assert rows == nr.golden_outputs(case)


# ------------------------------------------------------------------ 2. synthetic streams

# (window, N, type, shape, device batches): every window with every N, every type with both null
# handlings, host and device batches on every window
COMBOS = [(w, n, nr.TYPES[(i + j) % 3], ("ignore", "keep")[(i + j) % 2], (i + j // 2) % 2 == 0)
          for i, w in enumerate(nr.WINDOWS) for j, n in enumerate(nr.NS)]


def _batch(s, lo, hi, nc, device):
    a = tr.push_args(s, lo, hi, nc)
    if not device:
        return abi.HostBatch(**a)
    import torch
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64}
    # (DOUBLE columns travel as their int64 bits: no conversion may touch a NaN's payload)
    cols = [t(c.view(np.int64), torch.int64).view(torch.float64) if c.dtype == np.float64 else t(c, tdt[c.dtype])
            for c in map(np.ascontiguousarray, a["cols"])]
    bm = lambda v: abi.bitmap_torch(t(v, torch.bool))
    return abi.DeviceBatch(t(a["ts"], torch.int64), keys=t(a["keys"], torch.int64), key_valid=bm(a["key_valid"]),
                           row_valid=bm(a["row_valid"]), cols=cols, col_valid=[bm(v) for v in a["col_valid"]])


def _run_cut(prod, engine, win, typ, shape, n, device):
    col_types, aggs, having = nr.query(typ, shape, n)
    s, per_push, (pull_keys, pull_ws, pull_exp), _, _ = nr.expectation(win, typ, shape, n)
    emits = engine != abi.FLAG_ENGINE_ATOMIC
    flags = engine | (abi.FLAG_CHANGELOG if emits else 0)
    kw = dict(col_types=col_types, aggs=aggs, flags=flags, having=having, **nr.WINDOWS[win])
    cut = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    nc = len(col_types)
    for (lo, hi), (est, esnap, echg) in zip(tr.slices(nr.N_REC, nr.CUTS), per_push):
        st = cut.push(_batch(s, lo, hi, nc, device))
        assert st == est, (lo, hi, st, est)
        nr.assert_same(cut.snapshot(having), esnap, "snapshot after rows [%d, %d)" % (lo, hi))
        if emits:
            nr.assert_same(cut.changes(), echg, "changes of rows [%d, %d)" % (lo, hi))
        if esnap["n"]:  # a non-empty pull after every push: the rows of three keys the table holds
            ks = sorted(set(esnap["key"].tolist()))[:3]
            got = cut.get(keys=ks)
            assert got["n"] > 0
            if having is None:
                m = np.isin(esnap["key"], ks)
                nr.assert_same(got, dict(esnap, n=int(m.sum()), **{f: esnap[f][m] for f in ("key", "ws", "we", "rowtime")},
                                         values=[v[m] for v in esnap["values"]], null_bytes=[v[m] for v in esnap["null_bytes"]]),
                               "pull after rows [%d, %d)" % (lo, hi))
    got = cut.get(keys=pull_keys, ws=pull_ws)
    nr.assert_same(got, pull_exp, "pull")
    assert got["n"] > 0
    # the same records as one push: the cutting does not matter
    one = abi.AggHandle(prod, abi.make_agg_desc(**kw))
    one.push(_batch(s, 0, nr.N_REC, nc, device))
    nr.assert_same(one.snapshot(having), per_push[-1][1], "one push")
    one.close()
    return cut


@pytest.mark.parametrize("win,n,typ,shape,device", COMBOS)
def test_synthetic_vs_expectation(prod, win, n, typ, shape, device, engine):
    """Seven pushes (m = 0, 0 < m < N and m >= N on resident lists; windows closed and evicted
    between and within pushes): statistics, snapshot, changes and a pull after every push, then the
    same records as one push."""
    _run_cut(prod, engine, win, typ, shape, n, device).close()


@pytest.mark.parametrize("win", list(nr.WINDOWS))
def test_keep_and_ignore_of_one_column(prod, orc, win, engine):
    """The ignore-nulls and keep-nulls forms of one column in one query; groups whose arguments
    are NULL first, in the middle, last, and all NULL."""
    kw = dict(col_types=["DOUBLE"], aggs=[("LATEST_BY_OFFSET", 0, 3), ("LATEST_BY_OFFSET_NULLS", 0, 3),
                                          ("EARLIEST_BY_OFFSET", 0, 3), ("EARLIEST_BY_OFFSET_NULLS", 0, 3)],
              **nr.WINDOWS[win])
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=engine, **kw))
    e = nr.Expect(orc, **kw)
    #      key 1: NULL first    key 2: NULL in the middle    key 3: NULL last    key 4: all NULL    key 5: one record
    keys = [1, 1, 1, 1, 1,      2, 2, 2, 2, 2,               3, 3, 3, 3,         4, 4, 4, 4,        5]
    ok = [0, 0, 1, 1, 1,        1, 0, 0, 1, 1,               1, 1, 0, 0,         0, 0, 0, 0,        1]
    x = np.arange(len(keys), dtype=np.float64) - 7.0
    x[2] = -0.0
    ts = np.arange(len(keys)) * 10
    for lo, hi in ((0, 7), (7, 8), (8, len(keys))):
        a = dict(ts=ts[lo:hi], keys=np.array(keys)[lo:hi], cols=[x[lo:hi]], col_valid=[np.array(ok, bool)[lo:hi]])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        nr.assert_same(g.snapshot(), e.snapshot(), "rows [%d, %d)" % (lo, hi))
    snap = g.snapshot()
    got = {int(k): [nr.lists_of(snap, a)[r] for a in range(4)] for r, k in enumerate(snap["key"])}
    b = lambda i: nr.bits_of(float(x[i]), "DOUBLE")
    assert got[1] == [[b(2), b(3), b(4)], [b(2), b(3), b(4)], [b(2), b(3), b(4)], [None, None, b(2)]]
    assert got[2] == [[b(5), b(8), b(9)], [None, b(8), b(9)], [b(5), b(8), b(9)], [b(5), None, None]]
    assert got[3] == [[b(10), b(11)], [b(11), None, None], [b(10), b(11)], [b(10), b(11), None]]
    assert got[4] == [[], [None, None, None], [], [None, None, None]]
    assert got[5] == [[b(18)], [b(18)], [b(18)], [b(18)]]
    assert b(2) == -2**63
    g.close()
    e.close()


# ------------------------------------------------------------------ 3. sharing

@pytest.mark.parametrize("win,typ,device", [("hop", "INT32", False), ("tumb", "DOUBLE", True), ("none", "INT64", False)])
def test_shared_query(prod, win, typ, device, engine):
    """LATEST(x, 2), LATEST(x, 5), scalar LATEST(x), EARLIEST(x, 3), TOPK(x, 3) and COUNT(*) in one
    query with a HAVING on COUNT(*): the scalar LATEST and LATEST's N forms share one hidden sequence
    column, every aggregate has its own slots and words."""
    cut = _run_cut(prod, engine, win, typ, "shared", 0, device)
    with pytest.raises(abi.KsqlHipError, match=r"\(-4\).*HAVING"):
        cut.snapshot({"agg": 1, "op": "GT", "value": 0})
    cut.close()


def test_two_columns(prod, orc, engine):
    """Two N forms over two columns of different types, in the keep-nulls and ignore-nulls forms."""
    rng = np.random.default_rng(23)
    kw = dict(col_types=["INT32", "DOUBLE"], aggs=[("LATEST_BY_OFFSET_NULLS", 0, 2), ("EARLIEST_BY_OFFSET", 1, 3),
                                                   ("LATEST_BY_OFFSET", 1, 3), ("SUM", 0)], **nr.WINDOWS["tumb"])
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=engine, **kw))
    e = nr.Expect(orc, **kw)
    n = 3000
    ts = np.sort(rng.integers(0, 15_000, n)) + rng.integers(0, 2000, n)
    keys = rng.integers(0, 30, n)
    cols = [tr.x_values(rng, n, "INT32"), tr.x_values(rng, n, "DOUBLE")]
    valid = [rng.random(n) > 0.4, rng.random(n) > 0.2]
    for lo, hi in tr.slices(n, [500, 1, 1500]):
        a = dict(ts=ts[lo:hi], keys=keys[lo:hi], cols=[c[lo:hi] for c in cols], col_valid=[v[lo:hi] for v in valid])
        assert g.push(abi.HostBatch(**a)) == e.push(**a)
        nr.assert_same(g.snapshot(), e.snapshot(), "rows [%d, %d)" % (lo, hi))
    g.close()
    e.close()


# ------------------------------------------------------------------ 4. retry (child process, tuning build)

RETRY_LOG2P, RETRY_LDS_KB, RETRY_KEYS = 8, 64, 180_000
RETRY_AGGS = [("LATEST_BY_OFFSET", 0, 2), ("EARLIEST_BY_OFFSET_NULLS", 0, 2)]


def _fold(keys, x, v, aggs):
    """Unwindowed, every row accepted: the group is the key; the lists in arrival order."""
    xb = nr.col_bits(x)
    exp = {}
    for r, k in enumerate(keys.tolist()):
        lists = exp.setdefault(k, [[] for _ in aggs])
        for i, (kind, _, n) in enumerate(aggs):
            lists[i] = nr.aggregate(kind, n, xb[r] if v[r] else None, lists[i])
    return exp


def _retry_child():
    """Tuning build, 256 partitions, a 64 KB k_part_agg table (the sizes of test_gpu_topk's retry
    case): the rows of RETRY_AGGS over a BIGINT have 13 words (key, ws, row time; 2 + 2 value words,
    LATEST's mark, EARLIEST's null mask; 2 + 2 slots), 108 bytes per entry, H = 512.  Push 1 brings
    40 000 keys (156 +- 12 per partition), push 2 two records for each of 180 000 keys (703 +- 26 per
    partition): every partition's table overflows on pass 0 and the partition is retried in
    sub-passes, with the resident slots of push 1 as the chain's seeds.  A failed pass must have
    written nothing (a record applied twice shows twice in LATEST's list), and the resolve runs once
    over the rows the sub-passes left: keys of push 1 shift their resident element (LATEST(x, 2)
    drops it)."""
    prod = abi.load_product()
    assert prod.path.endswith("libksqldb_hip_tune.so"), prod.path
    rng = np.random.default_rng(11)
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64"], aggs=RETRY_AGGS, capacity_hint=1024))
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
    exp = _fold(np.concatenate(allk), np.concatenate(allx), np.concatenate(allv), RETRY_AGGS)
    assert snap["n"] == RETRY_KEYS and snap["key"].tolist() == sorted(exp)
    for a in range(len(RETRY_AGGS)):
        assert nr.lists_of(snap, a) == [exp[k][a] for k in snap["key"].tolist()], a
    print("OK")


def test_retry_path():
    from test_gpu_c1_retry import TUNE_LIB
    from test_gpu_part_retry import parse_trace
    assert os.path.exists(TUNE_LIB), "tuning build not present (make -C ksql_amd TUNING=1)"
    env = dict(os.environ, KSQL_AMD_LIB_VARIANT="tune", KHIP_PART_TRACE="1", KHIP_PART_LOG2=str(RETRY_LOG2P),
               KHIP_LDS_KB=str(RETRY_LDS_KB))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_offset_n as t; "
                        "t._retry_child()" % (REPO, os.path.join(REPO, "tests"))], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stderr[-4000:])
    trace = parse_trace(p.stderr)
    assert sorted(trace) == [1, 2], (sorted(trace), p.stdout[-2000:], p.stderr[-3000:])
    passes = trace[2]
    # the handle ran k_part_agg (never a merge), overflowed its table and went through sub-passes
    assert all(t["kernel"] == "agg" and t["H"] == 512 and t["P"] == 1 << RETRY_LOG2P for t in trace[1] + passes), trace
    assert len(passes) >= 2 and passes[0]["fail_table"] > 0 and passes[0]["sub_items"] == 0, passes
    assert any(t["sub_items"] > 0 for t in passes[1:]) and passes[-1]["failed"] == 0, passes
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------ 5. the global-atomic engine's table doubling

def test_atomic_table_doubles_within_a_push(prod):
    """capacity_hint 64 and 6000 keys in one push: the table doubles several times while records
    are applied (a record resumes at its first unapplied window), then the resolve's re-probe runs
    on the final table.  A second push finds resident lists."""
    rng = np.random.default_rng(31)
    aggs = [("LATEST_BY_OFFSET_NULLS", 0, 3), ("EARLIEST_BY_OFFSET", 0, 2), ("LATEST_BY_OFFSET", 0, 1)]
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["DOUBLE"], aggs=aggs, capacity_hint=64,
                                              flags=abi.FLAG_ENGINE_ATOMIC))
    allk, allx, allv = [], [], []
    for n, nkeys in ((30_000, 6000), (20_000, 9000)):
        keys = rng.integers(0, nkeys, n)
        x, v = tr.x_values(rng, n, "DOUBLE"), rng.random(n) > 0.3
        st = g.push(abi.HostBatch(np.zeros(n, np.int64), keys=keys, cols=[x], col_valid=[v]))
        assert st["windows_applied"] == n
        allk.append(keys), allx.append(x), allv.append(v)
        exp = _fold(np.concatenate(allk), np.concatenate(allx), np.concatenate(allv), aggs)
        snap = g.snapshot()
        assert snap["key"].tolist() == sorted(exp)
        for a in range(len(aggs)):
            assert nr.lists_of(snap, a) == [exp[k][a] for k in snap["key"].tolist()], a
    g.close()


# ------------------------------------------------------------------ 6. errors, result_len, reset

def _create_status(prod, **kw):
    d = abi.make_agg_desc(**kw)
    h = C.c_void_p()
    st = prod.agg_create(C.byref(d), C.byref(h))
    msg = prod.dll.khip_last_error()
    if st == 0:
        prod.agg_destroy(h)
    return st, msg


@pytest.mark.parametrize("kind", list(nr.NFORM))
def test_rejections(prod, kind):
    ok = dict(col_types=["INT64"], aggs=[(kind, 0, 3)])
    assert _create_status(prod, **ok)[0] == 0
    assert _create_status(prod, **dict(ok, aggs=[(kind, 0, 1)]))[0] == 0       # N = 1: an array of length <= 1
    assert _create_status(prod, **dict(ok, aggs=[(kind, 0, 0)]))[0] == 0       # no k bits: the scalar form
    cases = [
        (KHIP_E_INVALID, dict(ok, aggs=[(kind, 0, -1)])),
        (KHIP_E_INVALID, dict(ok, aggs=[(kind, 0, -32768)])),
        (KHIP_E_UNSUPPORTED, dict(ok, window_kind="SESSION", size_ms=1000)),
        (KHIP_E_UNSUPPORTED, dict(ok, flags=abi.FLAG_TABLE_SOURCE)),
        (KHIP_E_UNSUPPORTED, dict(ok, having={"agg": 0, "op": "GT", "value": 1})),
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=[(kind, 0, 30)])),
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=[(kind, 0, 32767)])),
        (KHIP_E_UNSUPPORTED, dict(ok, aggs=[(kind, 0, 8), (kind, 0, 7)])),     # 2 x 15 + words > 29
        # 6 user columns + 3 hidden columns (seq and ~seq of column 0's validity, one without) do not fit 8
        (KHIP_E_UNSUPPORTED, dict(col_types=["INT64"] * 6, aggs=[("LATEST_BY_OFFSET", 0, 2), ("EARLIEST_BY_OFFSET", 0, 2),
                                                                 ("LATEST_BY_OFFSET_NULLS", 1, 2)])),
    ]
    for want, kw in cases:
        st, msg = _create_status(prod, **kw)
        assert st == want and msg, (kw, st, msg)
    # the largest N that fits the 29 state words: 2 N, + 1 null mask (KEEP_NULLS), + 1 mark (LATEST)
    latest, ignore = nr.NFORM[kind]
    most = (29 - (0 if ignore else 1) - (1 if latest else 0)) // 2
    assert most in (13, 14)
    assert _create_status(prod, **dict(ok, aggs=[(kind, 0, most)]))[0] == 0
    st, msg = _create_status(prod, **dict(ok, aggs=[(kind, 0, most + 1)]))
    assert st == KHIP_E_UNSUPPORTED and b"state words" in msg
    # a HAVING on another aggregate of the query is fine; asked of the N form later it is not
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64"], aggs=[(kind, 0, 3), ("COUNT_STAR", -1)],
                                              having={"agg": 1, "op": "GT", "value": 1}))
    h.push(abi.HostBatch([1, 2, 3], keys=[5, 5, 6], cols=[np.array([7, 8, 9])]))
    snap = h.snapshot({"agg": 1, "op": "GT", "value": 1})
    assert snap["n"] == 1 and nr.lists_of(snap, 0) == [[7, 8]]
    with pytest.raises(abi.KsqlHipError, match=r"\(-4\).*HAVING"):
        h.snapshot({"agg": 0, "op": "GT", "value": 1})
    h.close()


def test_largest_n_runs(prod, engine):
    """EARLIEST(x, 14) and LATEST(x, 14) each fill the row: 20 records of one key through both."""
    x = np.arange(20, dtype=np.int64) * 3 - 5
    for kind, want in (("EARLIEST_BY_OFFSET", x[:14]), ("LATEST_BY_OFFSET", x[-14:])):
        h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64"], aggs=[(kind, 0, 14)], flags=engine))
        for lo, hi in ((0, 3), (3, 4), (4, 20)):
            h.push(abi.HostBatch(np.zeros(hi - lo, np.int64), keys=np.zeros(hi - lo, np.int64), cols=[x[lo:hi]]))
        snap = h.snapshot()
        h.close()
        assert nr.lists_of(snap, 0) == [want.tolist()], kind


def test_push_shuffled_rejected(prod):
    import torch
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT64", "INT64"], aggs=[("LATEST_BY_OFFSET", 1, 3)],
                                              **nr.WINDOWS["tumb"]))
    sh = abi.ShuffleHandle(prod, 1, 0, ["INT64", "INT64"])
    rows = torch.zeros((8, prod.dll.khip_shuffle_row_words(sh.h)), dtype=torch.int64, device="cuda")
    st = prod.agg_push_shuffled(g.h, sh.h, rows.data_ptr(), 8, None)
    assert st == KHIP_E_UNSUPPORTED and "shuffled" in prod.dll.khip_last_error().decode()
    sh.close()
    g.close()


def test_result_len_and_type(prod):
    d = abi.make_agg_desc(col_types=["INT32", "DOUBLE"], aggs=[
        ("LATEST_BY_OFFSET", 0, 3), ("COUNT_STAR", -1), ("EARLIEST_BY_OFFSET_NULLS", 1, 5), ("LATEST_BY_OFFSET", 1),
        ("EARLIEST_BY_OFFSET", 0, 1), ("TOPK", 0, 2)])
    lens, types = [], []
    for i in range(6):
        v = C.c_int32(-1)
        assert prod.agg_result_len(C.byref(d), i, C.byref(v)) == 0
        lens.append(v.value)
        assert prod.agg_result_type(C.byref(d), i, C.byref(v)) == 0
        types.append(v.value)
    assert lens == [3, 1, 5, 1, 1, 2] == abi.agg_result_len(d)
    assert types == abi.result_types(d)
    # N = 1 is an array all the same
    h = abi.AggHandle(prod, abi.make_agg_desc(col_types=["INT32"], aggs=[("LATEST_BY_OFFSET_NULLS", 0, 1)]))
    h.push(abi.HostBatch([0, 0, 0], keys=[1, 1, 2], cols=[np.array([4, 5, 6], np.int32)], col_valid=[[True, False, True]]))
    snap = h.snapshot()
    h.close()
    assert snap["values"][0].shape == (2, 1) and snap["null_bytes"][0].tolist() == [[2], [0]]
    assert nr.lists_of(snap, 0) == [[None], [6]]


def test_reset_then_same_stream(prod, engine):
    """After khip_agg_reset the sequences restart and the results equal a fresh handle's."""
    col_types, aggs, having = nr.query("DOUBLE", "keep", 3)
    s, per_push, _, _, _ = nr.expectation("hop", "DOUBLE", "keep", 3)
    g = abi.AggHandle(prod, abi.make_agg_desc(col_types=col_types, aggs=aggs, flags=engine, **nr.WINDOWS["hop"]))
    snaps = []
    for _ in range(2):
        for lo, hi in tr.slices(nr.N_REC, nr.CUTS):
            g.push(abi.HostBatch(**tr.push_args(s, lo, hi, 1)))
        snaps.append(g.snapshot())
        g.reset()
    g.close()
    nr.assert_same(snaps[0], per_push[-1][1], "before the reset")
    nr.assert_same(snaps[1], snaps[0], "after the reset")
