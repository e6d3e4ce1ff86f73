"""Reference models of CORRELATION(x, y) over INT / BIGINT pairs for the tests.

(a) `model`: the value the device path defines (include/ksqldb_hip.h, csrc/khip_correlation.hpp),
    from a group's exact integer state n, Sx, Sy, Sxx, Syy, Sxy over its pairs (records whose x and
    y are both non-null):
        N = n Sxy - Sx Sy,  DX = n Sxx - Sx²,  DY = n Syy - Sy²
        n = 0 or float(DX) * float(DY) = 0 -> the canonical NaN;  else float(N) / sqrt(float(DX) * float(DY))
    Python's int -> float conversion is correctly rounded (round half to even) and math.sqrt is
    IEEE, so the GPU tests compare bit for bit.
(b) `Fold`: the reference's arithmetic restated operation by operation in Python floats —
    function/udaf/correlation/CorrelationUdaf.java:86-102 (aggregate), :136-152 (undo), :115-134 (map),
    with Integer / Long::doubleValue as float(int) and Java's 0.0 / 0.0 = NaN, x / 0.0 = +-Infinity,
    sqrt(negative) = NaN.
(c) `exact_domain`: every quantity the reference forms for the group stays below 2^53 in magnitude
    (its five running sums, count * sum, the products of sums in map), whatever the record order: its
    doubles are then the integers and the model equals the fold bit for bit.
(d) `Expect`: windows, late records, dropped rows, row times, retention and the changelog's row set
    are not restated.  As tests/stddev_ref.py does, the unchanged oracle runs the query with COUNT(x)
    in each CORRELATION's place, and the per-record (key, window) applications it reports
    (topk_ref.applications / record_applications, imported, not modified) say which groups take each
    record; the groups' pair states go through `model`, the STDDEV aggregates beside them through
    stddev_ref's model.
"""
import functools
import math
import struct

import numpy as np

import stddev_ref as sr
import topk_ref as tr
from ksql_amd import abi

KIND = "CORRELATION"
U = 2.0 ** -53
NAN_BITS = 0x7FF8000000000000
NAN = struct.unpack("<d", struct.pack("<Q", NAN_BITS))[0]


def is_corr(agg):
    return agg[0] == KIND


def bits(x):
    """The double's bits, unsigned: a NaN is compared by its bits, not canonicalised."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def raw_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ (a) the exact model

def exact_terms(n, Sx, Sy, Sxx, Syy, Sxy):
    return n * Sxy - Sx * Sy, n * Sxx - Sx * Sx, n * Syy - Sy * Sy


def model_state(n, Sx, Sy, Sxx, Syy, Sxy):
    if n == 0:
        return NAN
    N, DX, DY = exact_terms(n, Sx, Sy, Sxx, Syy, Sxy)
    den2 = float(DX) * float(DY)
    if den2 == 0.0 or den2 < 0.0:  # (negative only for words past the 2^32 - 1 limit: sqrt -> NaN)
        return NAN
    r = float(N) / math.sqrt(den2)
    return NAN if r != r else r


def state_of(pairs):
    """pairs: the group's (x, y) with both non-null (Python ints)."""
    return (len(pairs), sum(x for x, _ in pairs), sum(y for _, y in pairs), sum(x * x for x, _ in pairs),
            sum(y * y for _, y in pairs), sum(x * y for x, y in pairs))


def model(pairs):
    return model_state(*state_of(pairs))


# ------------------------------------------------------------------ (b) the reference's fold

def _div(a, b):  # Java's double division
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):  # Math.sqrt
    return math.nan if a != a or a < 0.0 else math.sqrt(a)


class Fold:
    """One group's aggregate Struct {X_SUM, Y_SUM, X_SQUARED_SUM, Y_SQUARED_SUM, XY_SUM, COUNT}."""

    def __init__(self):
        self.sx = self.sy = self.sxx = self.syy = self.sxy = 0.0
        self.count = 0

    def aggregate(self, x, y):
        if x is None or y is None:
            return
        x, y = float(x), float(y)  # Integer / Long::doubleValue: round half even, as Python's
        self.sx = self.sx + x
        self.sy = self.sy + y
        self.sxx = self.sxx + x * x
        self.syy = self.syy + y * y
        self.sxy = self.sxy + x * y
        self.count = self.count + 1

    def undo(self, x, y):
        if x is None or y is None:
            return
        x, y = float(x), float(y)
        self.sx = self.sx - x
        self.sy = self.sy - y
        self.sxx = self.sxx - x * x
        self.syy = self.syy - y * y
        self.sxy = self.sxy - x * y
        self.count = self.count - 1

    def map(self):
        c = float(self.count)  # (long * double: the long is converted)
        numerator = c * self.sxy - self.sx * self.sy
        denominator_x = c * self.sxx - self.sx * self.sx
        denominator_y = c * self.syy - self.sy * self.sy
        denominator = _sqrt(denominator_x * denominator_y)
        return _div(numerator, denominator)


def fold(records):
    f = Fold()
    for x, y in records:
        f.aggregate(x, y)
    return f.map()


# ------------------------------------------------------------------ (c) the exact domain

def exact_domain(pairs):
    """Order-free and conservative: with absolute values in the sums' places, every partial sum, every
    product map forms and both sides of its subtractions are integers below 2^53."""
    n = len(pairs)
    ax, ay = sum(abs(x) for x, _ in pairs), sum(abs(y) for _, y in pairs)
    qx, qy, qxy = sum(x * x for x, _ in pairs), sum(y * y for _, y in pairs), sum(abs(x * y) for x, y in pairs)
    lim = 1 << 53
    return all(v < lim for v in (n * qxy + ax * ay, n * qx + ax * ax, n * qy + ay * ay))


def same(a, b):
    """Bit for bit; any NaN matches any NaN (the reference's NaN is the JVM's)."""
    return (a != a and b != b) or bits(a) == bits(b)


def true_coefficient(pairs, digits=120):
    """The Pearson coefficient to `digits` significant digits (decimal), or None where undefined."""
    import decimal
    N, DX, DY = exact_terms(*state_of(pairs))
    if DX * DY == 0:
        return None
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        return decimal.Decimal(N) / (decimal.Decimal(DX) * decimal.Decimal(DY)).sqrt()


# ------------------------------------------------------------------ the QTT cases

def case_desc(case, flags=0, changelog=True):
    d = case["desc"]
    aggs = [(a["kind"], a["arg_col"], a["arg_col2"]) if a["kind"] == KIND else (a["kind"], a["arg_col"]) for a in d["aggs"]]
    return abi.make_agg_desc(d["window_kind"], d["key_type"], d["size_ms"], d["advance_ms"], d["grace_ms"], d["col_types"],
                             aggs, flags=flags | (abi.FLAG_CHANGELOG if changelog else 0), having=d["having"])


def case_sequences(case):
    """A qtt_correlation.json case (unwindowed, every row valid, one CORRELATION): per input record
    (key, the group's records so far as (x, y) with None for NULL), as the reference emits one output
    per record."""
    d = case["desc"]
    assert d["window_kind"] == "NONE" and d["having"] is None and len(d["aggs"]) == 1
    a = d["aggs"][0]
    state, out = {}, []
    for r in case["input"]:
        assert r["key"] is not None and r["row_valid"] and r["ts"] >= 0
        recs = state.setdefault(r["key"], [])
        recs.append((r["cols"][a["arg_col"]], r["cols"][a["arg_col2"]]))
        out.append((r["key"], list(recs)))
    return out


def pairs_of(records):
    return [(x, y) for x, y in records if x is not None and y is not None]


# ------------------------------------------------------------------ (d) the oracle-derived expectation

class Expect:
    """aggs: (kind, col) or ("CORRELATION", x, y), STDDEV kinds allowed beside; kw: make_agg_desc
    arguments but col_types / aggs.  push() takes the arrays of a HostBatch (INT64 keys); snapshot() /
    changes() / get() return the handle's layout with the CORRELATION (and STDDEV) columns as DOUBLEs."""

    def __init__(self, orc, col_types, aggs, **kw):
        self.orc, self.col_types, self.aggs = orc, list(col_types), [tuple(a) for a in aggs]
        self.corr = [i for i, a in enumerate(self.aggs) if is_corr(a)]
        self.var = [i for i, a in enumerate(self.aggs) if sr.is_var(a)]
        oaggs = [("COUNT", a[1]) if is_corr(a) or sr.is_var(a) else a for a in self.aggs]
        self.h = abi.AggHandle(orc, abi.make_agg_desc(col_types=col_types, aggs=oaggs, **kw))
        mkw = {k: kw[k] for k in tr.Expect.WINDOW_KW if k in kw}
        self.m = abi.AggHandle(orc, abi.make_agg_desc(aggs=[("COUNT_STAR", -1)], flags=abi.FLAG_CHANGELOG, **mkw))
        self.pairs = sorted({(self.aggs[i][1], self.aggs[i][2]) for i in self.corr})
        self.vcols = sorted({self.aggs[i][1] for i in self.var})
        self.used = sorted({c for p in self.pairs for c in p} | set(self.vcols))
        self.state = {}   # (key, ws) -> {(x, y): [n, Sx, Sy, Sxx, Syy, Sxy]}
        self.vstate = {}  # (key, ws) -> {column: [n, T, Q]}
        self.stats = {"n0": 0, "n1": 0, "n2": 0, "n1000": 0, "nan": 0, "finite": 0, "pos": 0, "neg": 0, "counts_differ": 0}

    def push(self, ts, cols, col_valid, keys=None, key_valid=None, row_valid=None, apps=None):
        n = len(ts)
        col_valid = [np.ones(n, bool) if v is None else np.asarray(v, bool) for v in col_valid]
        st = self.h.push(abi.HostBatch(ts, keys=keys, key_valid=key_valid, row_valid=row_valid, cols=cols,
                                       col_valid=col_valid))
        if apps is None:
            apps = tr.record_applications(self.orc, self.m.h, ts, keys, key_valid, row_valid)
        assert sum(len(a) for a in apps) == st["windows_applied"]
        py = {c: np.asarray(cols[c]).tolist() for c in self.used}
        for r, groups in enumerate(apps):
            for g in groups:
                s = self.state.setdefault(g, {p: [0, 0, 0, 0, 0, 0] for p in self.pairs})
                for (cx, cy) in self.pairs:
                    if col_valid[cx][r] and col_valid[cy][r]:
                        x, y = py[cx][r], py[cy][r]
                        w = s[(cx, cy)]
                        w[0] += 1
                        w[1] += x
                        w[2] += y
                        w[3] += x * x
                        w[4] += y * y
                        w[5] += x * y
                v = self.vstate.setdefault(g, {c: [0, 0, 0] for c in self.vcols})
                for c in self.vcols:
                    if col_valid[c][r]:
                        x = py[c][r]
                        v[c][0] += 1
                        v[c][1] += x
                        v[c][2] += x * x
        return st

    def _translate(self, snap, count=True):
        out = dict(snap, values=list(snap["values"]), nulls=list(snap["nulls"]))
        for i in self.corr:
            p = (self.aggs[i][1], self.aggs[i][2])
            vals = np.zeros(snap["n"], np.float64)
            for r in range(snap["n"]):
                w = self.state.get((int(snap["key"][r]), int(snap["ws"][r])), {p: [0] * 6})[p]
                assert w[0] <= int(snap["values"][i][r])  # the oracle's COUNT(x) of the same group
                vals[r] = model_state(*w)
                if count:
                    n = w[0]
                    bucket = "n%d" % n if n <= 2 else ("n1000" if n >= 1000 else None)
                    if bucket:
                        self.stats[bucket] += 1
                    nan = vals[r] != vals[r]
                    self.stats["nan" if nan else "finite"] += 1
                    self.stats["pos"] += (not nan) and vals[r] > 0
                    self.stats["neg"] += (not nan) and vals[r] < 0
            out["values"][i], out["nulls"][i] = vals, np.zeros(snap["n"], bool)
        for i in self.var:
            kind, c = self.aggs[i]
            vals = np.zeros(snap["n"], np.float64)
            for r in range(snap["n"]):
                n, T, Q = self.vstate.get((int(snap["key"][r]), int(snap["ws"][r])), {c: [0, 0, 0]})[c]
                assert n == int(snap["values"][i][r])
                vals[r] = sr.model_state(kind, n, T, Q)
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


def assert_same(got, exp, what=""):
    """topk_ref.assert_same, and then every DOUBLE column by its raw bits where not NULL: a NaN must be
    the canonical quiet NaN the expectation holds, which assert_same alone would canonicalise away."""
    tr.assert_same(got, exp, what)
    for a, (gv, ev) in enumerate(zip(got["values"], exp["values"])):
        if gv.dtype == np.float64 and gv.ndim == 1:
            keep = ~np.asarray(exp["nulls"][a], bool)
            assert np.array_equal(raw_bits(gv)[keep], raw_bits(ev)[keep]), (what, "agg %d: raw bits" % a)


# ------------------------------------------------------------------ the streams of the GPU tests
# (here, not in tests/test_gpu_correlation.py: tests/test_correlation_ref.py asserts on the CPU that
# the same expectations are not vacuous)

TYPES = ("INT32", "INT64")
SHAPES = ("alone", "beside")
HAVING = {"agg": 0, "op": "GE", "value": 2}  # on COUNT(*), the "beside" shape

# CORRELATION(x, y) beside COUNT(*), COUNT(x), COUNT(y), SUM(x), AVG(y), STDDEV_SAMPLE(x), MAX(y),
# CORRELATION(y, x) and CORRELATION(x, x), with a HAVING on COUNT(*).  INT: one query (23 state
# words: 8 of the ordinary aggregates and STDDEV, 9 of the pair, none for (y, x), 6 for (x, x)).  BIGINT:
# the same list needs 11 + 17 + 11 = 39 words, past the 29 a row holds (KHIP_E_UNSUPPORTED, asserted in
# test_rejections), so it is cut into two queries that both keep COUNT(*) (the HAVING) and
# CORRELATION(x, y): "beside" with every ordinary aggregate, STDDEV and CORRELATION(y, x) (28 words),
# "beside2" with CORRELATION(y, x) and CORRELATION(x, x) (29 words).  Every listed aggregate is covered.
BESIDE = [("COUNT_STAR", -1), ("CORRELATION", 0, 1), ("COUNT", 0), ("COUNT", 1), ("SUM", 0), ("AVG", 1),
          ("STDDEV_SAMPLE", 0), ("MAX", 1), ("CORRELATION", 1, 0), ("CORRELATION", 0, 0)]
BESIDE_BIG_A = [("COUNT_STAR", -1), ("CORRELATION", 0, 1), ("COUNT", 0), ("COUNT", 1), ("SUM", 0), ("AVG", 1),
                ("STDDEV_SAMPLE", 0), ("MAX", 1), ("CORRELATION", 1, 0)]
BESIDE_BIG_B = [("COUNT_STAR", -1), ("CORRELATION", 0, 1), ("CORRELATION", 1, 0), ("CORRELATION", 0, 0)]


def shapes(typ):
    return ("alone", "beside") if typ == "INT32" else ("alone", "beside", "beside2")


def query(typ, shape):
    """(col_types, aggs, having)."""
    if shape == "alone":
        return [typ, typ], [("CORRELATION", 0, 1)], None
    if typ == "INT32":
        return [typ, typ], BESIDE, HAVING
    return [typ, typ], (BESIDE_BIG_A if shape == "beside" else BESIDE_BIG_B), HAVING


HOT = 7 * 1_000_003


def stream(win, typ):
    """topk_ref.stream's shape: 20 000 records, 300 keys, late records, null keys / rows; x and y of
    `typ`, each 30 % NULL independently, half their values from topk_ref.pool (the type's extremes).
    One key takes a share of the records so that some groups reach a thousand pairs."""
    b = tr.base_stream(win)
    rng = np.random.default_rng(sum((win + typ).encode()) + 12)
    x, y = tr.x_values(rng, tr.N, typ), tr.x_values(rng, tr.N, typ)
    vx, vy = rng.random(tr.N) > 0.30, rng.random(tr.N) > 0.30
    hrng = np.random.default_rng(sum(win.encode()) + 5)  # (the keys do not depend on the type)
    hot = hrng.random(tr.N) < (0.30 if win == "none" else 0.5)
    return dict(b, keys=np.where(hot, HOT, b["keys"]), cols=[x, y], col_valid=[vx, vy])


@functools.lru_cache(maxsize=None)
def stream_applications(win):
    s = stream(win, "INT32")  # (timestamps, keys and validity of keys / rows do not depend on the type)
    assert np.array_equal(s["keys"], stream(win, "INT64")["keys"])
    return tr.applications(abi.load_oracle(), s["ts"], s["keys"], s["key_valid"], s["row_valid"], **tr.WINDOWS[win])


@functools.lru_cache(maxsize=None)
def expectation(win, typ, shape):
    """The stream and, per push of the cutting, the expected statistics, snapshot and changes; a pull
    query; the whole table; the counters of the groups seen."""
    col_types, aggs, having = query(typ, shape)
    s = stream(win, typ)
    apps = stream_applications(win)
    e = Expect(abi.load_oracle(), col_types, aggs, flags=abi.FLAG_CHANGELOG, having=having, **tr.WINDOWS[win])
    per_push = []
    for lo, hi in tr.slices(tr.N, tr.CUTS):
        st = e.push(apps=apps[lo:hi], **tr.push_args(s, lo, hi, len(col_types)))
        per_push.append((st, e.snapshot(having), e.changes()))
    everything = e.snapshot()
    pull_keys = sorted(set(sorted(set(everything["key"].tolist()))[:5] + [HOT]))
    bounds = (int(np.median(everything["ws"])), int(everything["ws"].max()))
    pull = (pull_keys, bounds, e.get(pull_keys, bounds))
    if "COUNT" in [a[0] for a in aggs]:  # a group where COUNT(x), COUNT(y) and the pair count all differ
        ix, iy = aggs.index(("COUNT", 0)), aggs.index(("COUNT", 1))
        for r in range(everything["n"]):
            w = e.state.get((int(everything["key"][r]), int(everything["ws"][r])), {(0, 1): [0] * 6})[(0, 1)]
            cx, cy = int(everything["values"][ix][r]), int(everything["values"][iy][r])
            e.stats["counts_differ"] += len({cx, cy, w[0]}) == 3
    stats = dict(e.stats)
    e.close()
    return s, per_push, pull, everything, stats
