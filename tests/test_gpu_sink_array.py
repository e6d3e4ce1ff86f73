"""ARRAY value columns in the sink (khip_sink_encode, KHIP_SINK_ARRAY; include/ksqldb_hip.h
"serialization"): the results of TOPK / TOPKDISTINCT and of the N forms of LATEST / EARLIEST_BY_
OFFSET as the JSON lists the reference writes.

1. Every byte against tests/sink_array_ref.py (pinned to the reference's raw_value by
   test_sink_array_ref.py): every element type with L in {1, 3, 8, 29} and a column of L = 100, row
   counts at the tile and wave edges, host and device outputs at several alignments, host and
   device rows.
2. Tiles whose values fit k_sink_write_arr<TextEnc>'s stage (abi.SINK_ARRAY_STAGE bytes per round) beside
   tiles that take several rounds, with rows across a round's edge.
3. KHIP_E_BUFFER, 4. the QTT cases end to end (aggregate -> changes -> sink records),
5. the rejections, 6. scalar sinks after an array sink.
"""
import ctypes as C
import re
import struct

import numpy as np
import pytest

import offset_n_ref as nr
import qtt
import sink_array_ref as ar
import sink_ref
import topk_ref as tr
from ksql_amd import abi

pytestmark = pytest.mark.gpu

KHIP_E_INVALID, KHIP_E_BUFFER, KHIP_E_UNSUPPORTED = -1, abi.KHIP_E_BUFFER, -4
STAGE = abi.SINK_ARRAY_STAGE
NP = {"INT32": np.int32, "INT64": np.int64, "DOUBLE": np.float64}


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


# ------------------------------------------------------------------ rows

def _elements(rng, typ, shape):
    """Values of every kind the printers distinguish, as an array of the column's dtype."""
    m = int(np.prod(shape))
    if typ == "DOUBLE":
        bits = rng.integers(0, 2**63, m, dtype=np.int64).astype(np.uint64) | (
            rng.integers(0, 2, m).astype(np.uint64) << np.uint64(63))
        special = np.array([0.0, -0.0, 1.0, -1.5, 0.1, 1e-3, 9.999e-4, 1e7, 9999999.0, 1e22, 5e-324, 1e-323,
                            2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308, 123456.789,
                            float("nan"), float("inf"), float("-inf"), 2.0 ** 63]).view(np.uint64)
        payload = np.array([0x7FF8_0000_DEAD_BEEF, 0xFFF0_0000_0000_0001, 0x7FF0_0000_0000_0001], np.uint64)  # NaNs
        pool = np.concatenate([special, payload])
        pick = rng.random(m) < 0.4
        bits[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
        dec = rng.random(m) < 0.3  # decimal-looking values
        bits[dec & ~pick] = np.round(rng.uniform(-1e6, 1e6, int((dec & ~pick).sum())), 2).view(np.uint64)
        return bits.view(np.float64).reshape(shape)
    info = np.iinfo(NP[typ])
    v = rng.integers(info.min, info.max, m, dtype=np.int64, endpoint=True)
    small = rng.random(m) < 0.3
    v[small] = rng.integers(-1000, 1000, int(small.sum()))
    edge = rng.random(m) < 0.1
    v[edge] = rng.choice([info.min, info.max, 0, -1], int(edge.sum()))
    return v.astype(NP[typ]).reshape(shape)


def _array_column(rng, typ, n, L, lengths=None):
    """(n, L) values and null bytes: list lengths 0..L, NULL elements (byte 2) inside the lists, the
    slots past the end filled with values and bytes a reader must not look at (the list ends at the
    first byte that is neither 0 nor 2, whatever follows)."""
    vals = _elements(rng, typ, (n, L))
    lens = rng.integers(0, L + 1, n) if lengths is None else np.asarray(lengths)
    nb = np.where(rng.random((n, L)) < 0.15, 2, 0).astype(np.uint8)
    past = np.arange(L)[None, :] >= lens[:, None]
    nb[past] = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), int(past.sum()))
    at_end = lens < L
    nb[np.nonzero(at_end)[0], lens[at_end]] = rng.choice(np.array([1, 1, 1, 3, 255], np.uint8), int(at_end.sum()))
    return vals, nb


def _py(typ, x):
    return float(x) if typ == "DOUBLE" else int(x)


class Table:
    """Seeded rows for a list of value columns [(name, type, src[, L])] and their expected bytes."""

    def __init__(self, vcols, n, seed, window="TUMBLING", full=None):
        rng = np.random.default_rng(seed)
        self.vcols, self.n, self.window = vcols, n, window
        self.keys = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
        self.ws = rng.integers(0, 2**40, n, dtype=np.int64)
        self.we = self.ws + rng.integers(1, 10**6, n, dtype=np.int64)
        self.tomb = (rng.random(n) < 0.1).astype(np.uint8)
        nsrc = 1 + max(c[2] for c in vcols if not isinstance(c[2], str))
        self.values, self.nulls = [np.zeros(n, np.int64)] * nsrc, [None] * nsrc
        for c in vcols:
            if isinstance(c[2], str):
                continue
            if len(c) > 3:
                lengths = None if full is None else np.where(full, c[3], 0)
                self.values[c[2]], self.nulls[c[2]] = _array_column(rng, c[1], n, c[3], lengths)
            else:
                self.values[c[2]], self.nulls[c[2]] = _elements(rng, c[1], n), rng.random(n) < 0.1

    def rows(self):
        return {"n": self.n, "key": self.keys, "ws": self.ws, "we": self.we, "values": self.values, "nulls": self.nulls}

    def expected(self, i):
        if self.tomb[i]:
            return None
        vals = []
        for c in self.vcols:
            if c[2] == "WS":
                vals.append(int(self.ws[i]))
            elif c[2] == "WE":
                vals.append(int(self.we[i]))
            elif len(c) > 3:
                vals.append(ar.row_list(self.values[c[2]], self.nulls[c[2]], i, c[1]))
            else:
                vals.append(None if self.nulls[c[2]][i] else _py(c[1], self.values[c[2]][i]))
        return ar.encode_value([(c[0], c[1]) + tuple(c[3:]) for c in self.vcols], vals)

    def expected_key(self, i):
        return struct.pack(">q", int(self.keys[i])) + sink_ref.window_suffix(self.window, int(self.ws[i]), int(self.we[i]))

    def sink(self, prod):
        return abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "JSON", self.vcols, window_kind=self.window)


def _sample(n):
    if n <= 600:
        return range(n)
    edges = [i for t in range(256, n, 256) for i in range(t - 3, t + 3)]
    return sorted(set(range(0, n, 13)) | set(edges) | set(range(n - 5, n)))


# ------------------------------------------------------------------ 1. bytes against the restatement

LONG_NAME = "N" * 58 + "\x01\x02\x1f"  # escaped: 58 + 3 x 6 bytes, with '{"' and '":' over SK_PRE = 72
LAYOUTS = {
    # an array first, in the middle and last; scalars and the window bounds between them
    "mixed": [("A1", "INT32", 0, 1), ("S", "DOUBLE", 1), ("WSTART", "INT64", "WS"), ("A8", "DOUBLE", 2, 8),
              ("WEND", "INT64", "WE"), ("A3", "INT64", 3, 3)],
    # a scalar first; L = 29 of every type; L = 100 under a name the per-row escaper prints
    "wide": [("S", "INT64", 0), ("D29", "DOUBLE", 1, 29), ("I29", "INT32", 2, 29), ("L29", "INT64", 3, 29),
             (LONG_NAME, "INT64", 4, 100)],
    # the remaining (type, L) pairs of {INT32, INT64, DOUBLE} x {1, 3, 8}; the long name first
    "small": [(LONG_NAME, "INT32", 0, 3), ("b", "INT64", 1, 1), ("c", "DOUBLE", 2, 3), ("d", "INT32", 3, 8),
              ("e", "INT64", 4, 8), ("f", "DOUBLE", 5, 1)],
}


def test_layouts_cover_every_type_and_length():
    got = {(c[1], c[3]) for cols in LAYOUTS.values() for c in cols if len(c) > 3}
    assert got >= {(t, L) for t in NP for L in (1, 3, 8, 29)} and ("INT64", 100) in got


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5003])
def test_bytes_against_restatement(prod, n, layout):
    t = Table(LAYOUTS[layout], n, seed=n + len(layout))
    s = t.sink(prod)
    host = s.encode(t.rows(), tombstone=t.tomb)
    for i in _sample(n):
        assert host[0][i] == t.expected_key(i), i
        assert host[1][i] == t.expected(i), (i, host[1][i], t.expected(i))
    for align in (0, 7, 13) if n < 1000 else (3,):
        assert s.encode(t.rows(), tombstone=t.tomb, device_out=True, align=align) == host, align
    assert s.encode(t.rows(), tombstone=t.tomb, device_out=True, align=9, device_rows=True) == host
    lens = {len(v) for v in host[1] if v is not None}
    assert n < 255 or (len(lens) > 20 and any(v is None for v in host[1]))
    s.close()


def test_unwindowed_string_key_and_single_array(prod):
    """No window suffix, a STRING key, one array column alone: '{' is the array's own prefix."""
    n = 300
    vals, nb = _array_column(np.random.default_rng(2), "DOUBLE", n, 3)
    keys = ["k%d" % (i % 17) * (i % 5) for i in range(n)]
    s = abi.SinkHandle(prod, "JSON", [("K", "STRING")], "JSON", [("TOPK", "DOUBLE", 0, 3)])
    rows = {"n": n, "key": keys, "ws": np.zeros(n, np.int64), "we": np.zeros(n, np.int64), "values": [vals], "nulls": [nb]}
    for kw in ({}, {"device_out": True, "align": 1}):
        kb, vb = s.encode(rows, **kw)
        for i in range(n):
            assert kb[i] == sink_ref.encode_key("JSON", [("K", "STRING")], [keys[i]])
            assert vb[i] == ar.encode_value([("TOPK", "DOUBLE", 3)], [ar.row_list(vals, nb, i, "DOUBLE")]), i
    s.close()


# ------------------------------------------------------------------ 2. one round and several, in one call

def test_tiles_on_both_sides_of_the_stage(prod):
    """All-empty lists beside all-full BIGINT lists of L = 29: tile 0 (256 x 8 bytes) is copied out
    in one round, tile 1 (128 empty rows, then 128 full ones) and tile 2 (all full, > 100 KB) take
    several, with rows that lie across a round's edge and are encoded once per round; a last partial
    tile alternates.  The device outputs' guard bytes are checked by SinkHandle._encode_device."""
    n = 3 * 256 + 100
    i = np.arange(n)
    full = np.where(i < 256, False, np.where(i < 512, i >= 384, np.where(i < 768, True, i % 2 == 0)))
    t = Table([("L", "INT64", 0, 29)], n, seed=5, full=full)
    big = np.random.default_rng(6).integers(-2**63, -2**62, (n, 29))  # 20 bytes each
    t.values[0] = np.where(t.nulls[0] == 0, big, t.values[0])
    s = t.sink(prod)
    host = s.encode(t.rows(), tombstone=t.tomb)
    for r in range(n):
        assert host[1][r] == t.expected(r), (r, host[1][r], t.expected(r))
        assert host[0][r] == t.expected_key(r)
    for align in (0, 5, 11):
        assert s.encode(t.rows(), tombstone=t.tomb, device_out=True, align=align) == host, align
    assert s.encode(t.rows(), tombstone=t.tomb, device_out=True, align=14, device_rows=True) == host
    s.close()
    # from the produced lengths: both kinds of tile occurred, and rows across a round's edge
    lens = np.array([0 if v is None else len(v) for v in host[1]])
    tiles = [lens[a:a + 256] for a in range(0, n, 256)]
    sums = [int(x.sum()) for x in tiles]
    assert sums[0] <= STAGE and 0 < sums[0], sums
    assert STAGE < sums[1] and 3 * STAGE < sums[2], sums
    across = 0
    for x in tiles:
        end = np.cumsum(x)
        start = end - x
        across += int(((x > 0) & (start // STAGE != (end - 1) // STAGE)).sum())
    assert across >= 4, across
    assert (lens[:256][t.tomb[:256] == 0] == len(b'{"L":[]}')).all()


def test_round_edge_at_every_byte_of_a_row(prod):
    """One row text of R bytes (an escaped column name, quoted non-finite doubles, null, signs,
    exponents: every run of consecutive bytes the encoder puts) in tiles of more than one round; the
    first rows of tile t are t bytes longer, so over R tiles the round's edge cuts the row text at
    every one of its R bytes.  The row across the edge is encoded once per round, each round keeping
    its part."""
    name = "\x01\x1fn"
    elems = [float("nan"), float("-inf"), None, -0.5, -1.5e-7, 1e22, 0.0, float("inf"), -123456.789, None, 5e-324, -1.0,
             2.5, -2.2250738585072014e-308, 1e7, -9999999.0]
    L = len(elems)
    cols = [("P", "INT64"), (name, "DOUBLE", L)]
    R = len(ar.encode_value(cols, [7, elems]))
    assert 256 * R > STAGE + R and 256 * R < 2 * STAGE  # one edge per tile
    n = 256 * R
    p = np.full(n, 7, np.int64)
    for t in range(R):  # t more digits over the tile's first rows, at most 18 per row
        for j in range((t + 17) // 18):
            p[256 * t + j] = 10 ** min(18, t - 18 * j)
    vals, nb = ar.pack_lists([elems], L, "DOUBLE")
    vals, nb = np.repeat(vals, n, axis=0), np.repeat(nb, n, axis=0)
    rows = {"n": n, "key": np.arange(n), "ws": np.zeros(n, np.int64), "we": np.zeros(n, np.int64),
            "values": [p, vals], "nulls": [None, nb]}
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "JSON", [("P", "INT64", 0), (name, "DOUBLE", 1, L)])
    host = s.encode(rows)
    assert s.encode(rows, device_out=True, align=3) == host
    s.close()
    text = {int(x): ar.encode_value(cols, [int(x), elems]) for x in np.unique(p)}
    assert host[1] == [text[int(x)] for x in p]
    cut = set()
    for t in range(R):
        end = np.cumsum([len(v) for v in host[1][256 * t:256 * t + 256]])
        r = int(np.searchsorted(end, STAGE, side="right"))  # the row that holds the tile's byte STAGE
        assert end[r] - len(host[1][256 * t + r]) <= STAGE < end[r] and len(host[1][256 * t + r]) == R
        cut.add(STAGE - int(end[r] - R))
    assert cut == set(range(R))


# ------------------------------------------------------------------ 3. KHIP_E_BUFFER

def test_buffer_too_small_then_retry(prod):
    import torch
    n = 700
    t = Table(LAYOUTS["mixed"], n, seed=77)
    s = t.sink(prod)
    host = s.encode(t.rows(), tombstone=t.tomb)
    need = sum(len(v) for v in host[1] if v is not None)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    keep = {k: dev(v) for k, v in dict(key=t.keys, ws=t.ws, we=t.we, tomb=t.tomb).items()}
    cols = [dev(v) for v in t.values]
    nulls = [dev(np.asarray(x, np.uint8)) for x in t.nulls]
    rows = abi.SinkRows()
    rows.n_rows, rows.mem = n, abi.MEM_DEVICE
    rows.key_i64, rows.window_start, rows.window_end = keep["key"].data_ptr(), keep["ws"].data_ptr(), keep["we"].data_ptr()
    rows.tombstone = keep["tomb"].data_ptr()
    rows.col_data = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    rows.col_null = (C.c_void_p * len(cols))(*[c.data_ptr() for c in nulls])
    koff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    voff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    vnull = torch.zeros(n, dtype=torch.uint8, device="cuda")
    kbuf = torch.full((16 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    vbuf = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    out = abi.SinkOut()
    out.mem, out.key_capacity, out.value_capacity = abi.MEM_DEVICE, 16 * n, need - 1
    out.key_offsets, out.key_bytes = koff.data_ptr(), kbuf.data_ptr()
    out.value_offsets, out.value_bytes, out.value_null = voff.data_ptr(), vbuf.data_ptr() + 16, vnull.data_ptr()
    assert prod.sink_encode(s.h, C.byref(rows), C.byref(out)) == KHIP_E_BUFFER
    assert prod.dll.khip_last_error()
    assert (out.key_len, out.value_len) == (16 * n, need)
    assert bool((vbuf == 0xAB).all()) and bool((kbuf == 0xAB).all())  # no bytes written
    out.value_capacity = out.value_len
    prod.check(prod.sink_encode(s.h, C.byref(rows), C.byref(out)), "sink_encode")
    assert out.value_len == need
    vb, vo, vn = vbuf.cpu().numpy(), voff.cpu().numpy(), vnull.cpu().numpy()
    assert (vb[:16] == 0xAB).all() and (vb[16 + need:] == 0xAB).all()
    got = [None if vn[i] else vb[16 + vo[i]:16 + vo[i + 1]].tobytes() for i in range(n)]
    assert got == host[1]
    s.close()


# ------------------------------------------------------------------ 4. the QTT cases, end to end

QTT_CASES = ar.json_cases()


@pytest.mark.parametrize("device_rows", [False, True], ids=["host_rows", "device_rows"])
@pytest.mark.parametrize("kind,case", QTT_CASES, ids=[c["name"] for _, c in QTT_CASES])
def test_qtt_changes_to_sink_records(prod, kind, case, device_rows):
    """One record per push through an aggregate with KHIP_FLAG_CHANGELOG; each push's changes() go
    to the sink.  Every emitted value parses to the reference's raw_value and is byte-identical to
    the restatement of the row the aggregate emitted; every key is the KAFKA BIGINT key."""
    cols = ar.case_columns(case)
    desc = (tr if kind == "topk" else nr).case_desc(case, changelog=True)
    assert abi.agg_result_len(desc) == [c[2] for c in cols]
    s = abi.SinkHandle(prod, "KAFKA", [("ID", "INT64")], "JSON", [(nm, typ, a, L) for a, (nm, typ, L) in enumerate(cols)])
    h = abi.AggHandle(prod, desc)
    got = []
    for lo in range(len(case["input"])):
        h.push(qtt.case_batch(case, lo, lo + 1))
        chg = h.changes()
        if chg["n"] == 0:
            continue
        keys, vals = s.encode(chg, tombstone=chg["tombstone"], device_rows=device_rows)
        for r in range(chg["n"]):
            lists = [ar.row_list(chg["values"][a], chg["null_bytes"][a], r, typ) for a, (_, typ, _) in enumerate(cols)]
            assert vals[r] == ar.encode_value(cols, lists, tombstone=bool(chg["tombstone"][r])), (lo, r, vals[r])
            got.append((keys[r], vals[r]))
    h.close()
    s.close()
    exp = case["outputs"]
    assert len(got) == len(exp), (len(got), len(exp))
    for (kb, vb), o in zip(got, exp):
        assert kb == struct.pack(">q", o["key"])
        assert not o["tombstone"] and vb is not None
        ar.assert_parses_to(vb, cols, o["raw_value"])


# ------------------------------------------------------------------ 5. rejections

def _create_error(prod, *a, **kw):
    with pytest.raises(abi.KsqlHipError) as ei:
        abi.SinkHandle(prod, *a, **kw)
    m = re.search(r"failed \((-?\d+)\): (.*)", str(ei.value), re.S)
    assert m and m.group(2).strip() and prod.dll.khip_last_error(), str(ei.value)
    return int(m.group(1))


def test_rejections(prod):
    key = [("K", "INT64")]
    ok = abi.SinkHandle(prod, "KAFKA", key, "JSON", [("A", "INT64", 0, 3), ("B", "INT64", 0, 3), ("C", "DOUBLE", 1, 32767)])
    ok.close()
    # the value formats that carry no array (the reference's plan-time rejection)
    assert _create_error(prod, "KAFKA", key, "KAFKA", [("A", "INT64", 0, 3)]) == KHIP_E_INVALID
    assert _create_error(prod, "KAFKA", key, "DELIMITED", [("A", "INT64", 0, 3)]) == KHIP_E_INVALID
    assert _create_error(prod, "KAFKA", key, "DELIMITED", [("S", "INT64", 0), ("A", "DOUBLE", 1, 1)]) == KHIP_E_INVALID
    # WINDOWSTART / WINDOWEND are scalars
    for src in ("WS", "WE"):
        assert _create_error(prod, "KAFKA", key, "JSON", [("W", "INT64", src, 2)], window_kind="TUMBLING") == KHIP_E_INVALID
    # negative array bits
    for L in (-1, -32768):
        assert _create_error(prod, "KAFKA", key, "JSON", [("A", "INT64", 0, L)]) == KHIP_E_INVALID
    # an unknown base type under the bits
    assert _create_error(prod, "KAFKA", key, "JSON", [("A", "STRING", 0, 3)]) == KHIP_E_INVALID
    # one rows column read with different L, with different types, as an array and as a scalar
    assert _create_error(prod, "KAFKA", key, "JSON", [("A", "INT64", 0, 3), ("B", "INT64", 0, 4)]) == KHIP_E_INVALID
    assert _create_error(prod, "KAFKA", key, "JSON", [("A", "INT64", 0, 3), ("B", "DOUBLE", 0, 3)]) == KHIP_E_INVALID
    assert _create_error(prod, "KAFKA", key, "JSON", [("A", "INT64", 0, 3), ("B", "INT64", 0)]) == KHIP_E_INVALID
    assert _create_error(prod, "KAFKA", key, "JSON", [("B", "INT64", 0), ("A", "INT64", 0, 1)]) == KHIP_E_INVALID
    # (two scalar readers of one column stay legal, as before)
    abi.SinkHandle(prod, "KAFKA", key, "JSON", [("A", "INT64", 0), ("B", "INT64", 0)]).close()
    # key columns stay scalar: array bits on a key type are refused as an unknown key type is
    unknown = _create_error(prod, "KAFKA", [("K", 77)], "JSON", [("A", "INT64", 0)])
    assert _create_error(prod, "KAFKA", [("K", abi.TYPE["INT64"] | abi.SINK_ARRAY(3))], "JSON", [("A", "INT64", 0)]) == unknown
    assert unknown in (KHIP_E_INVALID, KHIP_E_UNSUPPORTED)


def test_encode_needs_the_null_bytes(prod):
    n = 10
    vals, nb = _array_column(np.random.default_rng(1), "INT64", n, 3)
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "JSON", [("S", "INT64", 0), ("A", "INT64", 1, 3)])
    rows = {"n": n, "key": np.arange(n), "ws": np.zeros(n, np.int64), "we": np.zeros(n, np.int64),
            "values": [np.arange(n), vals], "nulls": [None, None]}
    with pytest.raises(abi.KsqlHipError, match=r"\(-1\): .*null"):
        s.encode(rows)
    assert prod.dll.khip_last_error()
    with pytest.raises(ValueError):  # the boolean nulls of a snapshot are not the list's length
        s.encode(dict(rows, nulls=[None, nb.astype(bool)]))
    kb, vb = s.encode(dict(rows, nulls=[None, nb]))  # a scalar column's null array stays optional
    assert vb[3] == ar.encode_value([("S", "INT64"), ("A", "INT64", 3)], [3, ar.row_list(vals, nb, 3, "INT64")])
    s.close()


# ------------------------------------------------------------------ 6. scalar sinks unchanged

@pytest.mark.parametrize("vfmt", ["JSON", "DELIMITED", "KAFKA"])
def test_scalar_sink_after_an_array_sink(prod, vfmt):
    rng = np.random.default_rng(41)
    n = 3000
    arr = Table(LAYOUTS["small"], 300, seed=3)
    a = arr.sink(prod)  # an array handle on the same device, created and used first
    assert a.encode(arr.rows(), tombstone=arr.tomb)[1][0] == arr.expected(0)
    vc = [("D", "DOUBLE", 0), ("L", "INT64", 1), ("I", "INT32", 2)][:1 if vfmt == "KAFKA" else 3]
    d = _elements(rng, "DOUBLE", n)
    cols = [d, _elements(rng, "INT64", n), _elements(rng, "INT32", n)]
    nulls = [rng.random(n) < 0.1 for _ in cols]
    tomb = (rng.random(n) < 0.1).astype(np.uint8)
    keys = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], vfmt, vc)
    rows = {"n": n, "key": keys, "ws": np.zeros(n, np.int64), "we": np.zeros(n, np.int64), "values": cols, "nulls": nulls}
    host = s.encode(rows, tombstone=tomb)
    assert s.encode(rows, tombstone=tomb, device_out=True, align=6) == host
    for i in range(n):
        vals = [None if nulls[c][i] else _py(vc[c][1], cols[c][i]) for c in range(len(vc))]
        exp = sink_ref.encode_value(vfmt, [(c[0], c[1]) for c in vc], vals, tombstone=bool(tomb[i]))
        assert host[1][i] == exp, (i, host[1][i], exp)
        assert host[0][i] == struct.pack(">q", int(keys[i]))
    a.close()
    s.close()
