"""Streams whose DOUBLE aggregates have ONE possible bit pattern, a numpy model of them, and a
bit-for-bit comparator.

1. The exact class.  Every DOUBLE addend of a group is m * 2^e with one e per group and integer
   |m| <= 2^20; a group has fewer than 2^22 rows.  Every partial sum in every association order is
   then an integer below 2^42 times 2^e: exactly representable (subnormals included: e = -1074),
   so SUM does not depend on the order of the adds and AVG is one correctly rounded division.
2. The special groups (special_groups): dedicated keys whose result does not depend on the order
   either: NaNs of four kinds, +Inf and -Inf, signed zeros, an overflow to +Inf, subnormals,
   all-NULL arguments, the BIGINT / INTEGER extremes (the MIN / MAX planes' sentinels; wrapping sums).
3. model(): the closed form (int64 sum of m, ldexp, one division; the special classes from their
   definition) for unwindowed and TUMBLING queries with no late record.  It calls neither the
   oracle nor the product.
4. assert_exact(): offset_ref.assert_same with one exception: two NaNs are equal whatever their
   sign and payload (the NaN payload is unpinned: test_gpu_parity.py's docstring, f64_order_key).
   -0.0 and 0.0 differ.
"""
import numpy as np

from ksql_amd import abi

SCALES = [-1074, -10, 0, 960]
M_MAX = 1 << 20
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
DAY_MS = 24 * 3600 * 1000
NO_E = -(1 << 20)  # the exponent of a row without a finite addend

COL_TYPE = {"i32": "INT32", "i64": "INT64", "x": "DOUBLE"}
COL_DTYPE = {"i32": np.int32, "i64": np.int64, "x": np.float64}


# the NaN kinds, as bits (a float object is not trusted to carry a signalling NaN unchanged)
NANS = {"quiet": 0x7ff8000000000000, "signalling": 0x7ff0000000000001,
        "negative": 0xfff8000000000000, "payload": 0x7ff8dead0000beef}


def exact_stream(rng, n, nkeys, e, null_frac=0.1):
    """n rows of the exact class: keys in [0, nkeys) with key 0 hot (about 10 % of the rows:
    same-entry atomic contention), x = m * 2^e with about null_frac NULL and some m = 0 rows turned
    into -0.0, an INT32 and an INT64 column (wrapping sums) with their own NULLs."""
    keys = rng.integers(0, nkeys, n)
    keys[rng.random(n) < 0.1] = 0
    m = rng.integers(-M_MAX, M_MAX + 1, n)
    m[rng.random(n) < 0.02] = 0
    x = np.ldexp(m.astype(np.float64), e)
    x[(m == 0) & (rng.random(n) < 0.5)] = -0.0
    return {"keys": keys, "m": m, "e": np.full(n, e, np.int64), "x": x, "xv": rng.random(n) >= null_frac,
            "i32": rng.integers(I32_MIN, I32_MAX + 1, n).astype(np.int32), "i32v": rng.random(n) >= null_frac,
            "i64": rng.integers(-2**62, 2**62, n) * rng.integers(-1, 2, n), "i64v": rng.random(n) >= null_frac}


def special_groups(e):
    """{name: [(push, x, m, e, x valid, i64, i64 valid, i32, i32 valid, x bits or None), ...]}: the
    rows of each dedicated key, push 0 / 1 / 2 = P1 / P2 / P3.  m None = a non-finite x; x bits: the
    NaN's bit pattern.  What each group must give is in model()'s docstring."""
    def fin(p, m, ee=e, neg_zero=False):
        x = -0.0 if neg_zero else float(np.ldexp(float(m), ee))
        return (p, x, m, ee, True, m, True, m & 0xffff, True, None)

    def raw(p, x, xbits=None):
        return (p, x, None, NO_E, True, 1, True, 1, True, xbits)

    def ints(p, i64, i32):
        return (p, 0.0, None, NO_E, False, 0 if i64 is None else i64, i64 is not None,
                0 if i32 is None else i32, i32 is not None, None)

    g = {}
    for kind, nan in NANS.items():
        g["nan_" + kind] = [fin(0, 5), fin(0, -3), raw(1, np.nan, nan), fin(1, 9), fin(2, 4)]
    g["inf_cancel"] = [raw(0, np.inf), raw(1, -np.inf)]
    g["inf_pos"] = [raw(0, np.inf), fin(0, 7), fin(1, -2), fin(2, 11)]
    g["inf_neg"] = [fin(0, 7), raw(1, -np.inf), fin(1, -2), fin(2, 11)]
    g["neg_zero"] = [fin(p, 0, neg_zero=True) for p in (0, 0, 1, 1, 2)]
    g["zeros"] = [fin(0, 0), fin(0, 0, neg_zero=True), fin(1, 0, neg_zero=True), fin(2, 0)]
    # 80 rows of k * 2^1020: partial sums are exact below 16 * 2^1020 = 2^1024 and +Inf from there
    g["overflow"] = [fin(0 if r < 32 else 1 if r < 64 else 2, 1 + r % 7, 1020) for r in range(80)]
    g["subnormal"] = [fin(r % 3, (r * 7919 + 13) % (2 * M_MAX) - M_MAX, -1074) for r in range(12)] + \
                     [fin(0, 1, -1074), fin(1, 1, -1074), fin(2, -3, -1074)]
    g["all_null"] = [ints(p, None, None) for p in (0, 1, 1, 2)]
    g["int_max"] = [ints(0, I64_MAX, I32_MAX), ints(1, I64_MAX, I32_MAX)]  # sums wrap to -2
    g["int_min"] = [ints(0, I64_MIN, I32_MIN), ints(1, I64_MIN, I32_MIN), ints(2, I64_MIN, I32_MIN)]
    g["int_both"] = [ints(0, I64_MAX, I32_MAX), ints(1, I64_MIN, I32_MIN), ints(2, I64_MAX, I32_MAX)]
    return g


class Stream:
    """Pushes of rows: arrays ts, keys, m, e, x, xv, i32, i32v, i64, i64v per push, and the
    special groups' keys (special: name -> key)."""

    def __init__(self, pushes, special):
        self.pushes, self.special = pushes, special

    def batch(self, p, cols):
        d = self.pushes[p]
        return abi.HostBatch(d["ts"], keys=d["keys"], cols=[d[c] for c in cols], col_valid=[d[c + "v"] for c in cols])

    def special_keys(self):
        return np.array(sorted(self.special.values()), np.int64)


def make_stream(rng, pushes, n, nkeys, e, step, disorder, jump=0, jump_half=False, t0=0, key_pool=None,
                null_frac=0.1, spread=0, crowd=()):
    """`pushes` pushes of n exact-class rows plus the special groups' rows.  Push p's times lie in
    [t0 + p * step, t0 + (p + 1) * step): sorted with `disorder` ms of jitter, so within a grace
    period >= disorder nothing is late.  The special rows come first in their push, at t0 + p * step
    + r (r < 128): they are never late, and a window that holds t0 and t0 + 2 * step + 128 holds a
    special group's rows of all three pushes (P1, P2, P3 = pushes 0, 1, 2).  jump > 0: the last
    push moves jump ms ahead and closes the early windows; jump_half (for paths that take a
    stream-time jump inside a push): only its later half does, and every 16th row of that half
    stays behind, late for the windows the jump closed.  key_pool: the values the key indices
    0 .. nkeys + #special map to.  spread > 0 (<= t0; for grace periods past spread + step): the
    exact-class rows of push p are unsorted over [t0 + p * step - spread, t0 + (p + 1) * step), so
    every push spans spread / size windows while the special rows stay in one.  crowd: names of
    special groups (whose finite rows share the stream's e) that also take 5 % of each push's
    exact-class rows: a special group as hot as the hot key."""
    groups = special_groups(e)
    names = list(groups)
    special = {name: nkeys + j for j, name in enumerate(names)}
    out = []
    for p in range(pushes):
        d = exact_stream(rng, n, nkeys, e, null_frac)
        if spread:
            assert spread <= t0
            ts = t0 + p * step + rng.integers(-spread, step, n)
        else:
            ts = t0 + p * step + np.sort(rng.integers(0, step - disorder, n)) + rng.integers(0, max(disorder, 1), n)
        for name in crowd:
            d["keys"][rng.random(n) < 0.05] = special[name]
        if jump and p == pushes - 1 and jump_half:  # (every 16th row stays behind: late after the jump)
            ts[n // 2:] += np.where(np.arange(n - n // 2) % 16 == 7, 0, jump)
        elif jump and p == pushes - 1:
            ts += jump
        rows = [(special[name],) + r[1:] for name in names for r in groups[name] if r[0] == p]
        assert len(rows) < 128
        s = {"keys": np.array([r[0] for r in rows], np.int64),
             "x": np.array([r[1] for r in rows], np.float64),
             "m": np.array([0 if r[2] is None else r[2] for r in rows], np.int64),
             "e": np.array([r[3] for r in rows], np.int64),
             "xv": np.array([r[4] for r in rows], bool),
             "i64": np.array([r[5] for r in rows], np.int64), "i64v": np.array([r[6] for r in rows], bool),
             "i32": np.array([r[7] for r in rows], np.int64).astype(np.int32),
             "i32v": np.array([r[8] for r in rows], bool)}
        for i, r in enumerate(rows):
            if r[9] is not None:
                s["x"].view(np.uint64)[i] = r[9]
        sts = t0 + p * step + np.arange(len(rows), dtype=np.int64)
        d = {k: np.concatenate([s[k], d[k]]) for k in s}
        d["e"] = np.where(d["xv"] & np.isfinite(d["x"]), d["e"], NO_E)
        d["ts"] = np.concatenate([sts, ts])
        if key_pool is not None:
            d["keys"] = np.asarray(key_pool, np.int64)[d["keys"]]
        out.append(d)
    if key_pool is not None:
        special = {k: int(key_pool[v]) for k, v in special.items()}
    return Stream(out, special)


def plant_signalling(stream):
    """The special NaNs as the stream holds them (a test's check that no copy quieted them)."""
    k = stream.special["nan_signalling"]
    d = stream.pushes[1]
    return d["x"][(d["keys"] == k) & np.isnan(d["x"])].view(np.uint64)


# ------------------------------------------------------------------ the model

def order_key(x):
    """Double.compare's order as int64 (NaN canonical and greatest, -0.0 < 0.0)."""
    b = np.ascontiguousarray(x, np.float64).view(np.int64).copy()
    b[np.isnan(x)] = 0x7ff8000000000000
    return np.where(b >= 0, b, b ^ I64_MAX)


def order_key_inv(k):
    return np.where(k >= 0, k, k ^ I64_MAX).astype(np.int64).view(np.float64)


def _having_mask(res, having):
    """Rows of a result that pass HAVING {"agg", "op", "value"}: NULL never, NaN only "NE"."""
    v, null = res["values"][having["agg"]], res["nulls"][having["agg"]]
    c = having["value"]
    with np.errstate(invalid="ignore"):
        m = {"GT": v > c, "GE": v >= c, "LT": v < c, "LE": v <= c, "EQ": v == c, "NE": v != c}[having["op"]]
    return m & ~null


def filter_rows(res, mask):
    out = {"n": int(mask.sum()), "values": [v[mask] for v in res["values"]], "nulls": [v[mask] for v in res["nulls"]]}
    for f in ("key", "ws", "we", "rowtime", "tombstone"):
        if f in res:
            out[f] = res[f][mask]
    return out


def model(stream, size_ms=0, cols=("x",), aggs=(("SUM", 0),), grace_ms=-1, having=None):
    """The expected table after every push and the rows every push emits (EMIT CHANGES, no HAVING
    in the descriptor), for an unwindowed (size_ms = 0) or TUMBLING query over `stream` with the
    columns `cols` (names of Stream arrays) and `aggs` [(kind, column index)]: a list of
    {"snapshot", "changes"} per push, in the handle's layout.  having: the snapshot's filter.

    Groups are (key, ts // size * size).  Per group and DOUBLE column: a NaN among the valid
    arguments gives NaN, +Inf and -Inf together NaN, one of them that one; otherwise SUM =
    ldexp(int64 sum of m, e) (which overflows to Inf exactly where every order of the adds does:
    the overflow group's addends share a sign), +0.0 when no addend or only zeros; AVG = SUM /
    COUNT(x), 0.0 when the count is 0.  MIN / MAX follow Double.compare (NaN greatest, -0.0 < 0.0)
    and are NULL without a valid argument, whatever the values (the BIGINT extremes included).
    Integer sums wrap at their width.  The store keeps windows from (largest start) - (size +
    grace) on; a missing grace is 24 h - size."""
    res = []
    P = len(stream.pushes)
    cat = {k: np.concatenate([d[k] for d in stream.pushes]) for k in stream.pushes[0]}
    push_of = np.concatenate([np.full(len(d["ts"]), p) for p, d in enumerate(stream.pushes)])
    ts = cat["ts"]
    assert (ts >= 0).all()
    ws = ts // size_ms * size_ms if size_ms else np.zeros_like(ts)
    grace = 0 if not size_ms else grace_ms if grace_ms >= 0 else max(DAY_MS - size_ms, 0)
    if size_ms:  # the model holds only while nothing is late
        assert (ws + size_ms > np.maximum.accumulate(ts) - grace).all(), "a late record"
    order = np.lexsort((ws, cat["keys"]))
    for p in range(P):
        sel = order[push_of[order] <= p]
        k, w = cat["keys"][sel], ws[sel]
        first = np.flatnonzero(np.r_[True, (k[1:] != k[:-1]) | (w[1:] != w[:-1])])
        G = len(first)
        gid = np.cumsum(np.r_[True, (k[1:] != k[:-1]) | (w[1:] != w[:-1])]) - 1
        red = lambda f, a: f.reduceat(a, first)
        values, nulls = [], []
        for kind, c in aggs:
            no = np.zeros(G, bool)
            if kind == "COUNT_STAR":
                values.append(red(np.add, np.ones(len(sel), np.int64)))
                nulls.append(no)
                continue
            name = cols[c]
            v, valid = cat[name][sel], cat[name + "v"][sel]
            cnt = red(np.add, valid.astype(np.int64))
            if kind == "COUNT":
                values.append(cnt)
                nulls.append(no)
            elif kind in ("SUM", "AVG"):
                if name == "x":
                    s = _double_sum(cat, sel, v, valid, first, gid, G)
                else:
                    s = red(np.add, np.where(valid, v, 0).astype(np.int64))  # wraps at 64 bits
                    if name == "i32":
                        s = s.astype(np.int32)  # (fewer than 2^22 rows: the int64 sum itself did not wrap)
                if kind == "AVG":
                    with np.errstate(invalid="ignore", divide="ignore"):
                        s = np.where(cnt == 0, 0.0, s.astype(np.float64) / np.maximum(cnt, 1))
                values.append(s)
                nulls.append(no)
            else:
                null = cnt == 0
                if name == "x":
                    ok = order_key(v)
                    r = red(np.minimum, np.where(valid, ok, I64_MAX)) if kind == "MIN" else \
                        red(np.maximum, np.where(valid, ok, I64_MIN))
                    r = np.where(null, 0.0, order_key_inv(r))
                else:
                    info = np.iinfo(COL_DTYPE[name])
                    r = red(np.minimum, np.where(valid, v, info.max)) if kind == "MIN" else \
                        red(np.maximum, np.where(valid, v, info.min))
                    r = np.where(null, 0, r).astype(COL_DTYPE[name])
                values.append(r)
                nulls.append(null)
        gws = w[first]
        table = {"n": G, "key": k[first], "ws": gws, "we": gws + size_ms, "rowtime": red(np.maximum, ts[sel]),
                 "values": values, "nulls": nulls}
        touched = red(np.maximum, (push_of[sel] == p).astype(np.int64)) > 0
        changes = filter_rows(table, touched)
        changes["tombstone"] = np.zeros(changes["n"], bool)
        vis = gws >= gws.max() - (size_ms + grace) if size_ms else np.ones(G, bool)
        snap = filter_rows(table, vis)
        if having is not None:
            snap = filter_rows(snap, _having_mask(snap, having))
        res.append({"snapshot": snap, "changes": changes})
    return res


def _double_sum(cat, sel, v, valid, first, gid, G):
    fin = valid & np.isfinite(v)
    e = cat["e"][sel]
    ge = np.maximum.reduceat(np.where(fin, e, NO_E), first)
    assert (~fin | (e == ge[gid])).all(), "a group mixes exponents"
    m = np.where(fin, cat["m"][sel], 0)
    M = np.add.reduceat(m, first)
    assert (np.add.reduceat(np.abs(m), first) < 1 << 52).all()
    big = ge == 1020  # an overflow group: one sign, or the order of the adds would matter
    assert ((np.minimum.reduceat(m, first) >= 0) | (np.maximum.reduceat(m, first) <= 0) | ~big).all()
    with np.errstate(over="ignore"):
        s = np.ldexp(M.astype(np.float64), np.where(ge == NO_E, 0, ge))
    any_ = lambda mask: np.add.reduceat((valid & mask).astype(np.int64), first) > 0
    nan, pinf, ninf = any_(np.isnan(v)), any_(v == np.inf), any_(v == -np.inf)
    s = np.where(pinf, np.inf, s)
    s = np.where(ninf, -np.inf, s)
    return np.where(nan | (pinf & ninf), np.nan, s)


# ------------------------------------------------------------------ the comparator

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_exact(got, exp, what=""):
    """Two snapshots / change sets: keys, windows, row times, null flags, tombstones, and where not
    NULL the values through their int64 view (-0.0 != 0.0).  The one exception: NaN equals NaN,
    whatever sign and payload."""
    assert got["n"] == exp["n"], (what, got["n"], exp["n"])
    if isinstance(exp["key"], list):
        assert list(got["key"]) == list(exp["key"]), what
    else:
        assert np.array_equal(got["key"], exp["key"]), what
    for f in ("ws", "we", "rowtime"):
        assert np.array_equal(got[f], exp[f]), (what, f)
    if "tombstone" in exp:
        assert np.array_equal(got["tombstone"], exp["tombstone"]), (what, "tombstones")
    assert len(got["values"]) == len(exp["values"])
    for a, (gv, ev) in enumerate(zip(got["values"], exp["values"])):
        gn, en = np.asarray(got["nulls"][a], bool), np.asarray(exp["nulls"][a], bool)
        assert np.array_equal(gn, en), (what, "nulls of agg %d" % a)
        assert gv.dtype == ev.dtype, (what, a, gv.dtype, ev.dtype)
        same = bits(gv) == bits(ev)
        if gv.dtype == np.float64:
            same |= np.isnan(gv) & np.isnan(ev)
        bad = np.flatnonzero(~same & ~en)
        assert len(bad) == 0, (what, "agg %d: %d rows differ, first at row %d (key %s, ws %d): got %r (%#x) want %r (%#x)"
                               % (a, len(bad), bad[0], exp["key"][bad[0]], exp["ws"][bad[0]], gv[bad[0]],
                                  int(bits(gv)[bad[0]]) & (2**64 - 1), ev[bad[0]], int(bits(ev)[bad[0]]) & (2**64 - 1)))


def rows_of_keys(snap, keys):
    """The rows of INT64 `keys` of a snapshot (a pull query's expectation)."""
    m = np.isin(snap["key"], np.asarray(keys, np.int64))
    return filter_rows(snap, m)


# ------------------------------------------------------------------ table-source changelogs

TABLE_GROUPS = ["inf_mid", "nan_mid", "inf_stored", "inf_move_from", "inf_move_to", "neg_zero", "subnormal_a",
                "subnormal_b", "overflow", "finite_mid"]


def table_changelog(rng, pushes, nsrc, ngroups, e, null_frac=0.07):
    """A source table's changelog for khip_agg_push_table, SUM / AVG / COUNT of one DOUBLE argument
    x = m * 2^e: `pushes` pushes of 20,000 - 60,000 updates of nsrc PRIMARY KEYs that move between
    ngroups groups, delete keys (tombstones), repeat a key inside one push and carry NULL GROUP BY
    values, NULL arguments, NULL PRIMARY KEYs and negative times.  Every add and undo is exact, so
    the reference's sum - old + new has one possible result.  Planted after the random rows' ids
    (PRIMARY KEYs nsrc + j, groups ngroups + TABLE_GROUPS.index(name), in this arrival order):

      inf_mid     push 2: a key's row goes 3 -> +Inf -> 5 inside the push.  The reference adds and
                  undoes +Inf: Inf - Inf, a sticky NaN
      nan_mid     the same with a NaN as the intermediate row: NaN
      finite_mid  the same with a finite intermediate row (what netting may skip): 5 + the bystander
      inf_stored  +Inf stored by push 1, replaced by 4 in push 3: NaN from push 3 on
      inf_move    -Inf stored in group inf_move_from by push 1, moved to inf_move_to as 1 in push 2:
                  NaN in the group it left, 1 in the other
      neg_zero    -0.0 rows, updated to -0.0 again, one deleted: +0.0 throughout
      subnormal   m * 2^-1074 rows that move between two groups
      overflow    24 keys of 7 * 2^1020 (push 1), one deleted (push 2), one replaced (push 3): +Inf

    Every planted group but neg_zero also holds a bystander key with a finite row from push 1 on.
    Returns [{"batch": HostBatch, "src": push_table's key arguments, "rows": the arrays}], and
    {name: group key}."""
    gkey = {name: ngroups + j for j, name in enumerate(TABLE_GROUPS)}
    planted = {0: [], 1: [], 2: []}
    next_pk = [nsrc]

    def pk():
        next_pk[0] += 1
        return next_pk[0] - 1

    def row(p, k, group, x=None, m=None, ee=e, live=True):
        """x given: a non-finite (or -0.0) value; else m * 2^ee."""
        if x is None:
            x = float(np.ldexp(float(m), ee))
        planted[p].append((k, gkey[group], x, live, 0 if m is None else m, ee))

    for name in TABLE_GROUPS:  # the bystanders
        if name == "neg_zero":
            continue
        row(0, pk(), name, m=7 if name != "overflow" else 1, ee=1020 if name == "overflow" else
            -1074 if name.startswith("subnormal") else e)
    for name, mid in (("inf_mid", np.inf), ("nan_mid", np.nan), ("finite_mid", None)):
        k = pk()
        row(1, k, name, m=3)
        if mid is None:
            row(1, k, name, m=11)
        else:
            row(1, k, name, x=mid)
        row(1, k, name, m=5)
    k = pk()
    row(0, k, "inf_stored", x=np.inf)
    row(2, k, "inf_stored", m=4)
    k = pk()
    row(0, k, "inf_move_from", x=-np.inf)
    row(1, k, "inf_move_to", m=1)
    ks = [pk() for _ in range(3)]
    for k in ks:
        row(0, k, "neg_zero", x=-0.0)
    row(1, ks[0], "neg_zero", x=-0.0)
    row(1, ks[1], "neg_zero", x=-0.0, live=False)
    row(2, ks[2], "neg_zero", x=-0.0)
    ks = [pk() for _ in range(8)]
    for j, k in enumerate(ks):
        row(0, k, "subnormal_a", m=(j * 7919 + 13) % M_MAX - M_MAX // 2, ee=-1074)
    for j, k in enumerate(ks[:4]):
        row(1, k, "subnormal_b", m=j - 2, ee=-1074)
    row(2, ks[5], "subnormal_b", m=-1, ee=-1074)
    row(2, ks[0], "subnormal_a", m=1, ee=-1074, live=False)
    ks = [pk() for _ in range(24)]
    for k in ks:
        row(0, k, "overflow", m=7, ee=1020)
    row(1, ks[0], "overflow", m=7, ee=1020, live=False)
    row(2, ks[1], "overflow", m=3, ee=1020)

    out = []
    for p in range(pushes):
        n = int(rng.integers(20_000, 60_000))
        m = rng.integers(-M_MAX, M_MAX + 1, n)
        x = np.ldexp(m.astype(np.float64), e)
        x[(m == 0) & (rng.random(n) < 0.5)] = -0.0
        ts = rng.integers(0, 10**6, n)
        ts[rng.random(n) < 0.01] = -1
        d = {"pk": rng.integers(0, nsrc, n), "grp": rng.integers(0, ngroups, n), "gvalid": rng.random(n) > 0.05,
             "live": rng.random(n) > 0.12, "ts": ts, "pkv": rng.random(n) > 0.01, "x": x, "m": m,
             "e": np.full(n, e, np.int64), "xv": rng.random(n) > null_frac}
        rows = planted.get(p, [])
        if rows:
            s = {"pk": [r[0] for r in rows], "grp": [r[1] for r in rows], "gvalid": [True] * len(rows),
                 "live": [r[3] for r in rows], "ts": [500_000 + p] * len(rows), "pkv": [True] * len(rows),
                 "x": [r[2] for r in rows], "m": [r[4] for r in rows], "e": [r[5] for r in rows],
                 "xv": [True] * len(rows)}
            # the planted rows in the middle of the push, in their order
            h = n // 2
            d = {k: np.concatenate([d[k][:h], np.asarray(s[k], d[k].dtype), d[k][h:]]) for k in d}
        b = abi.HostBatch(d["ts"], keys=d["grp"], key_valid=d["gvalid"], row_valid=d["live"], cols=[d["x"]],
                          col_valid=[d["xv"]])
        out.append({"batch": b, "src": {"src_keys": d["pk"], "src_key_valid": d["pkv"]}, "rows": d})
    return out, gkey


def table_model(log, ngroups, upto):
    """The closed form of the random groups 0 .. ngroups - 1 (which never see a non-finite value)
    after pushes [0, upto]: per group over the PRIMARY KEYs whose last accepted record is a live row
    with that GROUP BY value, (COUNT(*), COUNT(x), SUM(x) = ldexp(sum m, e), AVG(x))."""
    d = {k: np.concatenate([p["rows"][k] for p in log[:upto + 1]]) for k in ("pk", "grp", "gvalid", "live", "ts",
                                                                           "pkv", "x", "m", "e", "xv")}
    acc = np.flatnonzero(d["pkv"] & (d["ts"] >= 0))
    _, first_rev = np.unique(d["pk"][acc][::-1], return_index=True)
    last = acc[len(acc) - 1 - first_rev]  # each key's last accepted record
    last = last[d["live"][last] & d["gvalid"][last] & (d["grp"][last] < ngroups)]
    g = d["grp"][last]
    star = np.bincount(g, minlength=ngroups)
    valid = d["xv"][last]
    cnt = np.bincount(g[valid], minlength=ngroups)
    M = np.zeros(ngroups, np.int64)
    np.add.at(M, g[valid], d["m"][last][valid])
    e = int(d["e"][0])
    s = np.ldexp(M.astype(np.float64), e)
    avg = np.where(cnt == 0, 0.0, s / np.maximum(cnt, 1))
    return star, cnt, s, avg
