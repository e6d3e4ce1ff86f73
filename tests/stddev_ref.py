"""Reference models of STDDEV_SAMP / STDDEV_SAMPLE over INT / BIGINT for the tests.

(a) `model`: the value the device path defines (include/ksqldb_hip.h, csrc/khip_variance.hpp), from
    a group's exact integer state n, T = Σx, Q = Σx²:
        n < 2 -> 0.0;  M2 = RN((n Q - T²) / n);  STDDEV_SAMP = M2 / (double)(n - 1);
        STDDEV_SAMPLE = sqrt(STDDEV_SAMP).
    Python's int / int is correctly rounded (round half to even) and math.sqrt is IEEE, so the GPU
    tests compare bit for bit.
(b) `Fold`: the reference's arithmetic restated operation by operation —
    function/udaf/stddev/StandardDeviationSampUdaf.java:124-144 (aggregate), :170-176 (map),
    :179-196 (undo), and StandardDeviationSampleUdaf.java (the same, map with Math.sqrt) — with
    int32 / int64 integer operations, the long -> double conversion of delta and the same
    evaluation order.  It RAISES `Wrap` when any Java integer operation would wrap: past that
    point the reference's value is meaningless and the device path deliberately differs.
(c) `Expect`: windows, late records, dropped rows, row times, retention and the changelog's row set
    are not restated.  As tests/topk_ref.py does, the unchanged oracle runs the query with COUNT(x)
    in each STDDEV's place, and the per-record (key, window) applications it reports
    (topk_ref.applications / record_applications, imported, not modified) say which groups take
    each record; the groups' (n, T, Q) go through `model`.
"""
import functools
import math
import struct

import numpy as np

import topk_ref as tr
from ksql_amd import abi

KINDS = ("STDDEV_SAMP", "STDDEV_SAMPLE")
U = 2.0 ** -53


def is_var(agg):
    return agg[0] in KINDS


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


# ------------------------------------------------------------------ (a) the exact model

def model_state(kind, n, T, Q):
    if n < 2:
        return 0.0
    d = n * Q - T * T
    assert d >= 0
    v = (d / n) / float(n - 1)
    return math.sqrt(v) if kind == "STDDEV_SAMPLE" else v


def model(kind, xs):
    """xs: the group's non-null arguments (Python ints)."""
    return model_state(kind, len(xs), sum(xs), sum(x * x for x in xs))


# ------------------------------------------------------------------ (b) the reference's fold

class Wrap(Exception):
    """A Java int / long operation of the reference wrapped."""


def _chk(v, bits_):
    if not -(1 << (bits_ - 1)) <= v < (1 << (bits_ - 1)):
        raise Wrap("%d-bit overflow: %d" % (bits_, v))
    return v


class Fold:
    """One group's aggregate Struct {SUM, COUNT, M2}.  typ: "INT32" | "INT64" (SUM's Java type)."""

    def __init__(self, typ):
        self.w = 32 if typ == "INT32" else 64
        self.sum, self.count, self.m2 = 0, 0, 0.0
        self.A = 0.0   # Σ |newM2| of every term added or removed
        self.ops = 0   # aggregate / undo calls with a non-null argument

    def _delta(self, x):
        # newValue * (agg.getInt64(COUNT) + 1) - (agg.get(SUM) + newValue), then Double.valueOf(long)
        a = _chk(x * _chk(self.count + 1, 64), 64)     # int * long: a long product
        b = _chk(self.sum + x, self.w)                 # in SUM's own type
        return float(_chk(a - b, 64))                  # (long -> double: round half even, as Python's)

    def aggregate(self, x):
        if x is None:
            return
        new_count = _chk(self.count + 1, 64)
        if new_count - 1 > 0:
            delta = self._delta(x)
            new_m2 = delta * delta / float(_chk(new_count * (new_count - 1), 64))
        else:
            new_m2 = 0.0
        new_sum = _chk(x + self.sum, self.w)
        self.count, self.sum, self.m2 = new_count, new_sum, new_m2 + self.m2
        self.A += abs(new_m2)
        self.ops += 1

    def undo(self, x):
        if x is None:
            return
        new_count = self.count - 1
        if new_count > 0:
            delta = self._delta(x)
            new_m2 = delta * delta / float(_chk(new_count * (new_count + 1), 64))
        else:
            new_m2 = 0.0
        new_sum = _chk(self.sum - x, self.w)
        self.count, self.sum, self.m2 = new_count, new_sum, self.m2 - new_m2
        self.A += abs(new_m2)
        self.ops += 1

    def map(self, kind):
        if self.count < 2:
            return 0.0
        v = self.m2 / float(self.count - 1)
        return math.sqrt(v) if kind == "STDDEV_SAMPLE" else v


def fold(kind, typ, xs):
    f = Fold(typ)
    for x in xs:
        f.aggregate(x)
    return f.map(kind)


def rel_bound(n):
    """|model - fold| <= rel_bound(n) * |value|, n = the group's non-null count: each fold term carries
    at most 4 roundings (the conversion of delta, the product, the conversion's partner the divisor
    is exact below 2^53, the division), the n - 2 additions of non-negative terms add at most
    (n - 2) u, the model's one rounding, the division by n - 1 and the sqrt at most 3 u; the rest is
    second-order margin."""
    return (n + 8) * U


def case_sequences(case):
    """A qtt_stddev.json case (unwindowed, every row valid): per input record (key, the group's
    non-null arguments so far), as the reference emits one output per record."""
    d = case["desc"]
    assert d["window_kind"] == "NONE" and d["having"] is None and len(d["aggs"]) == 1
    state, out = {}, []
    for r in case["input"]:
        if r["key"] is None or not r["row_valid"] or r["ts"] < 0:
            continue
        xs = state.setdefault(r["key"], [])
        x = r["cols"][d["aggs"][0]["arg_col"]]
        if x is not None:
            xs.append(x)
        out.append((r["key"], list(xs)))
    return out


# ------------------------------------------------------------------ (c) the oracle-derived expectation

class Expect:
    """aggs: (kind, col) with kind possibly STDDEV_SAMP / STDDEV_SAMPLE; kw: make_agg_desc arguments
    but col_types / aggs.  push() takes the arrays of a HostBatch (INT64 keys); snapshot() /
    changes() / get() return the handle's layout with the STDDEV columns as DOUBLEs."""

    def __init__(self, orc, col_types, aggs, **kw):
        self.orc, self.col_types, self.aggs = orc, list(col_types), [tuple(a) for a in aggs]
        self.var = [i for i, a in enumerate(self.aggs) if is_var(a)]
        oaggs = [("COUNT", a[1]) if is_var(a) else a for a in self.aggs]
        self.h = abi.AggHandle(orc, abi.make_agg_desc(col_types=col_types, aggs=oaggs, **kw))
        mkw = {k: kw[k] for k in tr.Expect.WINDOW_KW if k in kw}
        self.m = abi.AggHandle(orc, abi.make_agg_desc(aggs=[("COUNT_STAR", -1)], flags=abi.FLAG_CHANGELOG, **mkw))
        self.cols = sorted({self.aggs[i][1] for i in self.var})
        self.state = {}  # (key, ws) -> {column: [n, T, Q]}
        self.stats = {"n0": 0, "n1": 0, "n2": 0, "n1000": 0}

    def push(self, ts, cols, col_valid, keys=None, key_valid=None, row_valid=None, apps=None):
        n = len(ts)
        col_valid = [np.ones(n, bool) if v is None else np.asarray(v, bool) for v in col_valid]
        st = self.h.push(abi.HostBatch(ts, keys=keys, key_valid=key_valid, row_valid=row_valid, cols=cols,
                                       col_valid=col_valid))
        if apps is None:
            apps = tr.record_applications(self.orc, self.m.h, ts, keys, key_valid, row_valid)
        assert sum(len(a) for a in apps) == st["windows_applied"]
        py = {c: np.asarray(cols[c]).tolist() for c in self.cols}
        for r, groups in enumerate(apps):
            for g in groups:
                s = self.state.setdefault(g, {c: [0, 0, 0] for c in self.cols})
                for c in self.cols:
                    if col_valid[c][r]:
                        x = py[c][r]
                        s[c][0] += 1
                        s[c][1] += x
                        s[c][2] += x * x
        return st

    def _translate(self, snap, count=True):
        out = dict(snap, values=list(snap["values"]), nulls=list(snap["nulls"]))
        for i in self.var:
            kind, c = self.aggs[i]
            vals = np.zeros(snap["n"], np.float64)
            for r in range(snap["n"]):
                n, T, Q = self.state.get((int(snap["key"][r]), int(snap["ws"][r])), {c: [0, 0, 0]})[c]
                assert n == int(snap["values"][i][r])  # the oracle's COUNT(x) of the same group
                vals[r] = model_state(kind, n, T, Q)
                bucket = "n%d" % n if n <= 2 else ("n1000" if n >= 1000 else None)
                if count and bucket:
                    self.stats[bucket] += 1
            out["values"][i], out["nulls"][i] = vals, np.zeros(snap["n"], bool)
        return out

    def snapshot(self, having=None):
        return self._translate(self.h.snapshot(having))

    def changes(self):
        return self._translate(self.h.changes(), count=False)

    def get(self, keys, ws):
        s = self._translate(self.h.snapshot(), count=False)
        m = np.isin(s["key"], np.asarray(keys, np.int64)) & (s["ws"] >= ws[0]) & (s["ws"] <= ws[1])
        return {"n": int(m.sum()), "key": s["key"][m], "ws": s["ws"][m], "we": s["we"][m], "rowtime": s["rowtime"][m],
                "values": [v[m] for v in s["values"]], "nulls": [v[m] for v in s["nulls"]]}

    def close(self):
        self.h.close()
        self.m.close()


# ------------------------------------------------------------------ the streams of the GPU tests
# (here, not in tests/test_gpu_stddev.py: tests/test_stddev_ref.py asserts on the CPU that the same
# expectations are not vacuous)

TYPES = ("INT32", "INT64")
SHAPES = ("STDDEV_SAMP", "STDDEV_SAMPLE", "beside")
HAVING = {"agg": 0, "op": "GE", "value": 2}  # on COUNT(*), the "beside" shape


def query(typ, shape):
    """(col_types, aggs, having): the aggregate alone, or both kinds beside COUNT(*), COUNT(x), AVG(x),
    SUM(x) and MAX(y), with a HAVING on COUNT(*)."""
    if shape != "beside":
        return [typ], [(shape, 0)], None
    return [typ, "INT64"], [("COUNT_STAR", -1), ("STDDEV_SAMPLE", 0), ("COUNT", 0), ("AVG", 0), ("SUM", 0),
                            ("STDDEV_SAMP", 0), ("MAX", 1)], HAVING


def stream(win, typ):
    """topk_ref.stream's shape: 20 000 records, 300 keys, late records, null keys / rows, x 30 % NULL
    with half its values from topk_ref.pool (the type's extremes).  One key in twelve takes the hot
    key's place so that some groups reach a thousand records."""
    s = tr.stream(win, typ)
    rng = np.random.default_rng(sum(win.encode()) + 5)  # (the keys do not depend on the type)
    hot = rng.random(tr.N) < (0.30 if win == "none" else 0.5)
    keys = np.where(hot, 7 * 1_000_003, s["keys"])
    return dict(s, keys=keys)


@functools.lru_cache(maxsize=None)
def stream_applications(win):
    s = stream(win, "INT32")  # (timestamps, keys and validity do not depend on the type)
    assert np.array_equal(s["keys"], stream(win, "INT64")["keys"])
    return tr.applications(abi.load_oracle(), s["ts"], s["keys"], s["key_valid"], s["row_valid"], **tr.WINDOWS[win])


@functools.lru_cache(maxsize=None)
def expectation(win, typ, shape):
    """The stream and, per push of the cutting, the expected statistics, snapshot and changes; a pull
    query; the counters of the group sizes seen."""
    col_types, aggs, having = query(typ, shape)
    s = stream(win, typ)
    apps = stream_applications(win)
    e = Expect(abi.load_oracle(), col_types, aggs, flags=abi.FLAG_CHANGELOG, having=having, **tr.WINDOWS[win])
    per_push = []
    for lo, hi in tr.slices(tr.N, tr.CUTS):
        st = e.push(apps=apps[lo:hi], **tr.push_args(s, lo, hi, len(col_types)))
        per_push.append((st, e.snapshot(having), e.changes()))
    everything = e.snapshot()
    pull_keys = sorted(set(sorted(set(everything["key"].tolist()))[:5] + [7 * 1_000_003]))
    bounds = (int(np.median(everything["ws"])), int(everything["ws"].max()))
    pull = (pull_keys, bounds, e.get(pull_keys, bounds))
    stats = dict(e.stats)
    e.close()
    return s, per_push, pull, everything, stats
