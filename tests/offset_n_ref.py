"""Reference models of the N forms LATEST_BY_OFFSET(col, N[, ignoreNulls]) / EARLIEST_BY_OFFSET(col,
N[, ignoreNulls]) for the tests.

1. `aggregate`: latestTN.aggregate (function/udaf/offset/LatestByOffset.java:149-218) and
   earliestTN.aggregate (EarliestByOffset.java:162-228), line by line on Python lists.  An element is
   the argument (None = NULL); the tests carry DOUBLEs as their int64 bits, so a NaN payload and
   -0.0 survive every step.
2. `Expect`, built like topk_ref.Expect: windows, late records, dropped rows, row times, retention
   and the changelog's row set are NOT restated.  The unchanged oracle runs the query with COUNT(x)
   (ignore-nulls forms) or COUNT(*) (keep-nulls forms) in each folded aggregate's place: that gives
   the rows, and a cross-check of every list's length.  A second oracle handle (COUNT(*) with a
   changelog) takes the records one at a time, and the rows it emits per record are the (key,
   window)s that record was applied to.  The lists are folded with `aggregate` in arrival order over
   exactly those applications.  Scalar offset aggregates and TOPK / TOPKDISTINCT of the same query
   are folded the same way with offset_ref.aggregate / topk_ref.aggregate.
Results are compared bit for bit, null bytes (0 present, 1 past the end, 2 NULL element) exactly.
"""
import functools

import numpy as np

import offset_ref
import topk_ref as tr
from ksql_amd import abi

NFORM = {"LATEST_BY_OFFSET": (True, True), "EARLIEST_BY_OFFSET": (False, True),
         "LATEST_BY_OFFSET_NULLS": (True, False), "EARLIEST_BY_OFFSET_NULLS": (False, False)}  # (latest, ignoreNulls)
PRESENT, PAST_END, NULL_ELEMENT = 0, 1, 2


def is_nform(agg):
    return agg[0] in NFORM and len(agg) > 2


def is_scalar_offset(agg):
    return agg[0] in NFORM and len(agg) == 2


def aggregate(kind, n, current, agg):
    """One record (current: the argument, None = NULL) into the list `agg`; returns the new list."""
    latest, ignore_nulls = NFORM[kind]
    if current is None and ignore_nulls:
        return agg
    if latest:
        agg.append(current)
        current_size = len(agg)
        if current_size > n:
            return agg[current_size - n:current_size]
        return agg
    if len(agg) < n:
        agg.append(current)
    return agg


def bits_of(v, typ):
    """A fixture value (a Python number) as the int the device returns: a DOUBLE's int64 bits."""
    if v is None:
        return None
    if typ != "DOUBLE":
        return int(v)
    return int(np.array([v], np.float64).view(np.int64)[0])


def col_bits(col):
    """A column as Python ints: DOUBLEs as their int64 bits (no conversion touches a NaN)."""
    col = np.ascontiguousarray(col)
    return (col.view(np.int64) if col.dtype == np.float64 else col).tolist()


def case_aggs(case):
    return [(a["kind"], a["arg_col"], a["k"]) if "k" in a else (a["kind"], a["arg_col"]) for a in case["desc"]["aggs"]]


def case_desc(case, flags=0, changelog=True):
    d = case["desc"]
    return abi.make_agg_desc(d["window_kind"], d["key_type"], d["size_ms"], d["advance_ms"], d["grace_ms"], d["col_types"],
                             case_aggs(case), flags=flags | (abi.FLAG_CHANGELOG if changelog else 0),
                             retention_ms=d.get("retention_ms", -1), emit=d.get("emit", "CHANGES"), having=d["having"])


def model_outputs(case):
    """A qtt_offset_n.json case (unwindowed) through `aggregate`: per accepted input record the
    (key, [list of bits / None per aggregate]) the reference emits."""
    d = case["desc"]
    assert d["window_kind"] == "NONE" and d["having"] is None
    state, out = {}, []
    for r in case["input"]:
        if r["key"] is None or not r["row_valid"] or r["ts"] < 0:
            continue
        st = state.setdefault(r["key"], [[] for _ in d["aggs"]])
        for i, a in enumerate(d["aggs"]):
            typ = d["col_types"][a["arg_col"]]
            st[i] = aggregate(a["kind"], a["k"], bits_of(r["cols"][a["arg_col"]], typ), st[i])
        out.append((r["key"], [list(x) for x in st]))
    return out


def golden_outputs(case):
    """The reference's output records of a case in the same form."""
    d = case["desc"]
    return [(o["key"], [[bits_of(v, d["col_types"][a["arg_col"]]) for v in o["values"][i]] for i, a in enumerate(d["aggs"])])
            for o in case["outputs"]]


def lists_of(snap, a):
    """Aggregate a of a snapshot / change set in the array layout → one list per row (bits, None for a
    NULL element).  Checks the layout: elements with null byte 0 or 2 first, then null byte 1; value 0
    wherever the byte is not 0; and that abi.array_row reads the same list."""
    vals, nb = snap["values"][a], np.asarray(snap["null_bytes"][a])
    assert vals.ndim == 2 and nb.shape == vals.shape and nb.dtype == np.uint8, (vals.shape, nb.shape, nb.dtype)
    vb = vals.view(np.int64) if vals.dtype == np.float64 else vals
    out = []
    for r in range(snap["n"]):
        ln = int((nb[r] != PAST_END).sum())
        assert (nb[r, :ln] != PAST_END).all() and (nb[r, ln:] == PAST_END).all(), ("hole in the list", a, r, nb[r])
        assert np.isin(nb[r], (PRESENT, PAST_END, NULL_ELEMENT)).all(), (a, r, nb[r])
        assert not vb[r][nb[r] != PRESENT].any(), ("value in a null slot", a, r)
        out.append([None if nb[r, j] == NULL_ELEMENT else int(vb[r, j]) for j in range(ln)])
        row = abi.array_row(vals, nb, r)
        assert [None if v is None else bits_of(v, "DOUBLE" if vals.dtype == np.float64 else "INT64") for v in row] == out[-1]
    return out


class Expect:
    """The oracle-derived expectation (module docstring, 2).  aggs: (kind, col) or (kind, col, N / k);
    kw: make_agg_desc arguments but col_types / aggs.  push() takes the arrays of a HostBatch (INT64
    keys); snapshot() / changes() / get() return the handle's layout, array aggregates as (rows, L)
    values with "null_bytes" (and "nulls" = bytes != 0)."""

    WINDOW_KW = tr.Expect.WINDOW_KW

    def __init__(self, orc, col_types, aggs, **kw):
        self.orc, self.col_types, self.aggs = orc, list(col_types), [tuple(a) for a in aggs]
        self.folded = [i for i, a in enumerate(self.aggs) if a[0] in NFORM or tr.is_topk(a)]
        oaggs = list(self.aggs)
        for i in self.folded:  # in place: the positions (a HAVING's index) stay
            a = self.aggs[i]
            keep = a[0] in NFORM and not NFORM[a[0]][1]
            oaggs[i] = ("COUNT_STAR", -1) if keep else ("COUNT", a[1])
        self.h = abi.AggHandle(orc, abi.make_agg_desc(col_types=col_types, aggs=oaggs, **kw))
        mkw = {k: kw[k] for k in self.WINDOW_KW if k in kw}
        self.m = abi.AggHandle(orc, abi.make_agg_desc(aggs=[("COUNT_STAR", -1)], flags=abi.FLAG_CHANGELOG, **mkw))
        self.state = {}  # (key, ws) -> {aggregate index: list (N forms, TOPK) or value / offset_ref.UNSET}
        # per push and N-form aggregate: how many groups saw m = 0 on a non-empty list / 0 < m < N / m >= N
        self.m_classes = {"zero": 0, "some": 0, "full": 0}

    def _fresh(self):
        return {i: (offset_ref.UNSET if is_scalar_offset(self.aggs[i]) else []) for i in self.folded}

    def push(self, ts, cols, col_valid, keys=None, key_valid=None, row_valid=None, apps=None):
        n = len(ts)
        col_valid = [np.ones(n, bool) if v is None else np.asarray(v, bool) for v in col_valid]
        st = self.h.push(abi.HostBatch(ts, keys=keys, key_valid=key_valid, row_valid=row_valid, cols=cols,
                                       col_valid=col_valid))
        if apps is None:
            apps = tr.record_applications(self.orc, self.m.h, ts, keys, key_valid, row_valid)
        assert sum(len(a) for a in apps) == st["windows_applied"]
        pybits = [col_bits(c) for c in cols]
        pyvals = [np.asarray(c).tolist() for c in cols]
        before = {g: {i: len(s[i]) for i in self.folded if is_nform(self.aggs[i])} for g, s in self.state.items()}
        taken = {}
        for r, groups in enumerate(apps):
            for g in groups:
                s = self.state.setdefault(g, self._fresh())
                for i in self.folded:
                    a = self.aggs[i]
                    c = a[1]
                    ok = bool(col_valid[c][r])
                    if tr.is_topk(a):
                        if ok:
                            tr.aggregate(a[0], a[2], self.col_types[c], pyvals[c][r], s[i])
                    elif is_scalar_offset(a):
                        s[i] = offset_ref.aggregate(a[0], pybits[c][r] if ok else None, s[i])
                    else:
                        s[i] = aggregate(a[0], a[2], pybits[c][r] if ok else None, s[i])
                        if ok or not NFORM[a[0]][1]:
                            taken[(g, i)] = taken.get((g, i), 0) + 1
        for g, lens in before.items():
            for i, ln in lens.items():
                m = taken.get((g, i), 0)
                if ln:
                    self.m_classes["zero" if m == 0 else ("some" if m < self.aggs[i][2] else "full")] += 1
        return st

    def reset(self):
        self.h.reset()
        self.m.reset()
        self.state.clear()

    def _translate(self, snap):
        out = dict(snap, values=list(snap["values"]), nulls=list(snap["nulls"]),
                   null_bytes=[np.asarray(x, bool).astype(np.uint8) for x in snap["nulls"]])
        for i in self.folded:
            a = self.aggs[i]
            typ = self.col_types[a[1]]
            dt = abi.NP_TYPE[abi.TYPE[typ]]
            rows = [self.state.get((int(snap["key"][r]), int(snap["ws"][r])), self._fresh())[i] for r in range(snap["n"])]
            cnt = snap["values"][i]  # the oracle's COUNT(x) / COUNT(*) of the same group
            if is_scalar_offset(a):
                vals, nb = np.zeros(snap["n"], np.int64), np.zeros(snap["n"], np.uint8)
                for r, v in enumerate(rows):
                    assert (v is offset_ref.UNSET) == (int(cnt[r]) == 0), (a, r)
                    if v is offset_ref.UNSET or v is None:
                        nb[r] = 1
                    else:
                        vals[r] = v
                vals = vals.view(np.float64) if typ == "DOUBLE" else vals.astype(dt)
            else:
                L = a[2]
                vals, nb = np.zeros((snap["n"], L), np.int64), np.full((snap["n"], L), PAST_END, np.uint8)
                for r, lst in enumerate(rows):
                    if tr.is_topk(a):
                        lst = [tr.canon(v, typ) for v in lst]
                        assert len(lst) <= min(int(cnt[r]), L) and (a[0] != "TOPK" or len(lst) == min(int(cnt[r]), L))
                    else:
                        assert len(lst) == min(int(cnt[r]), L), (a, r, lst, int(cnt[r]))
                    for j, v in enumerate(lst):
                        nb[r, j] = NULL_ELEMENT if v is None else PRESENT
                        vals[r, j] = 0 if v is None else v
                vals = vals.view(np.float64) if typ == "DOUBLE" else vals.astype(dt)
            out["values"][i], out["null_bytes"][i], out["nulls"][i] = vals, nb, nb != 0
        return out

    def snapshot(self, having=None):
        return self._translate(self.h.snapshot(having))

    def changes(self):
        return self._translate(self.h.changes())

    def get(self, keys, ws):
        """A pull query's rows (the oracle has none): the snapshot's rows of `keys` with the window
        start inside the closed bounds ws = (lo, hi)."""
        s = self.snapshot()
        m = np.isin(s["key"], np.asarray(keys, np.int64)) & (s["ws"] >= ws[0]) & (s["ws"] <= ws[1])
        return {"n": int(m.sum()), "key": s["key"][m], "ws": s["ws"][m], "we": s["we"][m], "rowtime": s["rowtime"][m],
                "values": [v[m] for v in s["values"]], "nulls": [v[m] for v in s["nulls"]],
                "null_bytes": [v[m] for v in s["null_bytes"]]}

    def close(self):
        self.h.close()
        self.m.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(got, exp, what=""):
    """Two snapshots / change sets: keys, windows, row times, the null bytes exactly (0 / 1 / 2), the
    values bit for bit where the byte is 0 and zero elsewhere in an array."""
    assert got["n"] == exp["n"], (what, got["n"], exp["n"])
    assert np.array_equal(got["key"], exp["key"]), what
    for f in ("ws", "we", "rowtime"):
        assert np.array_equal(got[f], exp[f]), (what, f)
    if "tombstone" in exp:
        assert np.array_equal(got["tombstone"], exp["tombstone"]), what
    assert len(got["values"]) == len(exp["values"])
    for a, (gv, ev) in enumerate(zip(got["values"], exp["values"])):
        gn, en = np.asarray(got["null_bytes"][a]), np.asarray(exp["null_bytes"][a])
        assert gv.shape == ev.shape and gn.shape == en.shape == gv.shape, (what, a, gv.shape, ev.shape, gn.shape, en.shape)
        assert gn.dtype == np.uint8 and np.array_equal(gn, en), (what, "null bytes of agg %d" % a, np.argwhere(gn != en)[:5])
        assert gv.dtype == ev.dtype, (what, a, gv.dtype, ev.dtype)
        ok = bits(gv)[en == 0] == bits(ev)[en == 0]
        assert ok.all(), (what, "agg %d" % a, np.argwhere(en == 0)[~ok][:5])
        if gv.ndim == 2:
            assert not bits(gv)[en != 0].any(), (what, "agg %d: value in a null slot" % a)


# ------------------------------------------------------------------ the streams of the GPU tests
# (here, not in tests/test_gpu_offset_n.py: tests/test_offset_n_ref.py asserts on the CPU that the
# same expectations cover what the lists can get wrong)

WINDOWS = {"none": dict(window_kind="NONE"),
           "tumb": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=1000),
           "hop": dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, grace_ms=1000)}
TYPES = tr.TYPES
NS = (1, 2, 3, 5)
N_REC, N_KEYS = 4000, 40
CUTS = [1, 300, 700, 37, 1200, 900]  # 7 pushes: these and the rest
SPAN_MS = 24_000


def base_stream(win):
    """4000 records over 40 keys in 24 s of event time, 3 s of disorder (grace 1 s: some are late).
    Keys 0-3 take 60 % of the records (many more than N per push and window), keys 4-19 most of the
    rest, keys 20-39 about one record in 50 (none, or fewer than N, per push).  3 % null keys, null
    rows and negative timestamps each."""
    rng = np.random.default_rng(sum(win.encode()) + 5)
    ts = np.sort(rng.integers(0, SPAN_MS, N_REC)) + rng.integers(0, 3_000, N_REC)
    ts = np.where(rng.random(N_REC) < 0.03, -rng.integers(1, 100, N_REC), ts)
    u = rng.random(N_REC)
    keys = np.where(u < 0.60, rng.integers(0, 4, N_REC), np.where(u < 0.98, rng.integers(4, 20, N_REC),
                                                                  rng.integers(20, N_KEYS, N_REC)))
    return dict(ts=ts, keys=(keys - 7) * 1_000_003, key_valid=rng.random(N_REC) > 0.03, row_valid=rng.random(N_REC) > 0.03)


def stream(win, typ):
    """base_stream + the columns x (typ, 30 % NULL, topk_ref.x_values: extremes, NaN payloads, -0.0)
    and y BIGINT (5 % NULL)."""
    rng = np.random.default_rng(sum((win + typ).encode()) + 5)
    return dict(base_stream(win), cols=[tr.x_values(rng, N_REC, typ), rng.integers(-1000, 1000, N_REC)],
                col_valid=[rng.random(N_REC) > 0.30, rng.random(N_REC) > 0.05])


SHAPES = ("ignore", "keep", "shared")
HAVING = {"agg": 5, "op": "GE", "value": 2}  # on COUNT(*), the "shared" shape


def query(typ, shape, n):
    """(col_types, aggs, having).  ignore / keep: LATEST and EARLIEST (x, n) in the ignore-nulls or
    the keep-nulls form, beside COUNT(*).  shared: LATEST(x, 2), LATEST(x, 5), scalar LATEST(x),
    EARLIEST(x, 3), TOPK(x, 3) and COUNT(*) with a HAVING on it (n is not used)."""
    if shape == "ignore":
        return [typ], [("LATEST_BY_OFFSET", 0, n), ("COUNT_STAR", -1), ("EARLIEST_BY_OFFSET", 0, n)], None
    if shape == "keep":
        return [typ], [("LATEST_BY_OFFSET_NULLS", 0, n), ("EARLIEST_BY_OFFSET_NULLS", 0, n), ("COUNT_STAR", -1)], None
    return [typ], [("LATEST_BY_OFFSET", 0, 2), ("LATEST_BY_OFFSET", 0, 5), ("LATEST_BY_OFFSET", 0), ("EARLIEST_BY_OFFSET", 0, 3),
                   ("TOPK", 0, 3), ("COUNT_STAR", -1)], HAVING


@functools.lru_cache(maxsize=None)
def stream_applications(win):
    b = base_stream(win)
    return tr.applications(abi.load_oracle(), b["ts"], b["keys"], b["key_valid"], b["row_valid"], **WINDOWS[win])


@functools.lru_cache(maxsize=None)
def expectation(win, typ, shape, n):
    """The stream and, per push of the cutting, the expected statistics, snapshot and changes; a pull;
    the whole table; the m classes seen; and how many (group, push) pairs were updated and closed by
    the same push (the push's last stream time is past the window's end + grace)."""
    col_types, aggs, having = query(typ, shape, n)
    s = stream(win, typ)
    apps = stream_applications(win)
    e = Expect(abi.load_oracle(), col_types, aggs, flags=abi.FLAG_CHANGELOG, having=having, **WINDOWS[win])
    per_push, same_push_closed = [], 0
    w = WINDOWS[win]
    for lo, hi in tr.slices(N_REC, CUTS):
        st = e.push(apps=apps[lo:hi], **tr.push_args(s, lo, hi, len(col_types)))
        per_push.append((st, e.snapshot(having), e.changes()))
        if win != "none":
            seen = s["ts"][:hi][(s["ts"][:hi] >= 0) & s["key_valid"][:hi] & s["row_valid"][:hi]]
            groups = {g for a in apps[lo:hi] for g in a}
            same_push_closed += sum(g[1] + w["size_ms"] + w["grace_ms"] <= seen.max() for g in groups) if len(seen) else 0
    everything = e.snapshot()
    pull_keys = sorted(set(everything["key"].tolist()))[:6]
    bounds = (int(np.median(everything["ws"])), int(everything["ws"].max()))
    pull = (pull_keys, bounds, e.get(pull_keys, bounds))
    classes = dict(e.m_classes, same_push_closed=same_push_closed)
    e.close()
    return s, per_push, pull, everything, classes
