"""The AVRO value format of the sink (khip_sink_encode with value_format = KHIP_FMT_AVRO and
khip_sink_set_avro_schema_id; include/ksqldb_hip.h "AVRO values").

Every value is compared bit for bit with tests/avro_sink_ref.py (pinned to hand-written byte strings
by test_avro_sink_ref.py), every key with sink_ref:
1. row counts at the wave (64) and tile (256) edges, host and device rows and outputs, output
   alignments, window kinds and key formats;  2. the varint boundaries in every column type, NULLs,
   tombstones;  3. waves whose values pass the per-wave stage (SK_WBUF = 2048 bytes) beside waves that
   fit, 32 and 0 value columns;  4. ARRAY columns, rows across the tile stage's 32 KB rounds, a sink fed
   by a TOPK / LATEST_BY_OFFSET(col, 3, false) handle;  5. sizes, KHIP_E_BUFFER, guard bytes;  6. the
   schema id;  7. the device's own AVRO decoder reads the records back;  8. the QTT cases end to end.
"""
import ctypes as C
import json
import struct

import numpy as np
import pytest

import avro_ref
import avro_sink_ref as av
import qtt
import sink_array_ref as ar
import sink_ref
from ksql_amd import abi

pytestmark = pytest.mark.gpu

KHIP_E_INVALID, KHIP_E_BUFFER, KHIP_E_STATE = -1, abi.KHIP_E_BUFFER, -7
STAGE = abi.SINK_ARRAY_STAGE
WAVE_STAGE = 2048  # khip_sink.hip's SK_WBUF
NP = {"INT32": np.int32, "INT64": np.int64, "DOUBLE": np.float64}
SID = 0x01020304


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


# ------------------------------------------------------------------ rows

def boundaries(typ):
    """Where a zig-zag varint changes its length (+-2^(7k-1) and their neighbours), the type's
    extremes, 0 and +-1."""
    info = np.iinfo(NP[typ])
    out = {0, 1, -1, info.min, info.max, info.min + 1, info.max - 1}
    for k in range(1, 10):
        p = 1 << (7 * k - 1)
        out |= {p - 1, p, -p, -p - 1}
    return sorted(v for v in out if info.min <= v <= info.max)


DOUBLES = np.concatenate([
    np.array([0.0, -0.0, 1.0, -1.5, 0.1, 5e-324, 2.2250738585072009e-308, 1.7976931348623157e308, float("nan"), float("inf"),
              float("-inf")]).view(np.uint64),
    np.array([0x7FF8_0000_DEAD_BEEF, 0xFFF0_0000_0000_0001, 0x7FF0_0000_0000_0001, 0x0102_0304_0506_0708], np.uint64)])


def elements(rng, typ, shape):
    m = int(np.prod(shape))
    if typ == "DOUBLE":
        bits = rng.integers(0, 2**63, m, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, m).astype(np.uint64) << np.uint64(63))
        pick = rng.random(m) < 0.3
        bits[pick] = DOUBLES[rng.integers(0, len(DOUBLES), int(pick.sum()))]
        return bits.view(np.float64).reshape(shape)
    info = np.iinfo(NP[typ])
    v = rng.integers(info.min, info.max, m, dtype=np.int64, endpoint=True)
    # every varint length: magnitudes of every bit count
    short = rng.random(m) < 0.5
    v[short] >>= rng.integers(0, 64 if typ == "INT64" else 32, int(short.sum()))
    edge = rng.random(m) < 0.2
    v[edge] = rng.choice(np.array(boundaries(typ), np.int64), int(edge.sum()))
    return v.astype(NP[typ]).reshape(shape)


def array_column(rng, typ, n, L, lengths=None, null_rate=0.15):
    """(n, L) values and null bytes: list lengths 0..L, NULL elements (byte 2) inside the lists; the
    slots past the end hold values and bytes a reader must not look at."""
    vals = elements(rng, typ, (n, L))
    lens = rng.integers(0, L + 1, n) if lengths is None else np.asarray(lengths)
    nb = np.where(rng.random((n, L)) < null_rate, 2, 0).astype(np.uint8)
    past = np.arange(L)[None, :] >= lens[:, None]
    nb[past] = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), int(past.sum()))
    at_end = lens < L
    nb[np.nonzero(at_end)[0], lens[at_end]] = rng.choice(np.array([1, 1, 1, 3, 255], np.uint8), int(at_end.sum()))
    return vals, nb


def py(typ, x):
    return x if typ == "DOUBLE" else int(x)  # a DOUBLE stays a numpy float64: its bits are compared


class Table:
    """Seeded rows for value columns [(name, type, src[, L])] and their expected records."""

    def __init__(self, vcols, n, seed, window="NONE", schema_id=SID, null_rate=0.1, tomb_rate=0.1):
        rng = np.random.default_rng(seed)
        self.vcols, self.n, self.window, self.schema_id = vcols, n, window, schema_id
        self.keys = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
        self.ws = elements(rng, "INT64", n)
        self.we = elements(rng, "INT64", n)
        self.tomb = (rng.random(n) < tomb_rate).astype(np.uint8)
        nsrc = 1 + max([c[2] for c in vcols if not isinstance(c[2], str)] + [-1])
        self.values, self.nulls = [np.zeros(n, np.int64)] * nsrc, [None] * nsrc
        for c in vcols:
            if isinstance(c[2], str):
                continue
            if len(c) > 3:
                self.values[c[2]], self.nulls[c[2]] = array_column(rng, c[1], n, c[3])
            else:
                self.values[c[2]], self.nulls[c[2]] = elements(rng, c[1], n), rng.random(n) < null_rate

    def rows(self):
        return {"n": self.n, "key": self.keys, "ws": self.ws, "we": self.we, "values": self.values, "nulls": self.nulls}

    def row(self, i):
        vals = []
        for c in self.vcols:
            if c[2] == "WS":
                vals.append(int(self.ws[i]))
            elif c[2] == "WE":
                vals.append(int(self.we[i]))
            elif len(c) > 3:
                vals.append([None if x is None else py(c[1], x) for x in row_list(self.values[c[2]], self.nulls[c[2]], i)])
            else:
                vals.append(None if self.nulls[c[2]][i] else py(c[1], self.values[c[2]][i]))
        return vals

    def cols(self):
        return [(c[0], c[1]) + tuple(c[3:]) for c in self.vcols]

    def expected(self):
        keys = [struct.pack(">q", int(self.keys[i])) + sink_ref.window_suffix(self.window, int(self.ws[i]), int(self.we[i]))
                for i in range(self.n)]
        vals = [av.encode_value(self.cols(), self.row(i), self.schema_id, tombstone=bool(self.tomb[i])) for i in range(self.n)]
        return keys, vals

    def sink(self, prod):
        return abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "AVRO", self.vcols, window_kind=self.window,
                              avro_schema_id=self.schema_id)

    def check(self, prod, aligns=(0, 7, 13), device_rows=True):
        """Host rows to host outputs against the restatement; then the other memory kinds against that."""
        s = self.sink(prod)
        exp = self.expected()
        host = s.encode(self.rows(), tombstone=self.tomb)
        assert host[0] == exp[0]
        for i in range(self.n):
            assert host[1][i] == exp[1][i], (i, host[1][i], exp[1][i], self.row(i))
        for align in aligns:
            assert s.encode(self.rows(), tombstone=self.tomb, device_out=True, align=align) == host, align
        if device_rows:
            assert s.encode(self.rows(), tombstone=self.tomb, device_rows=True) == host
            assert s.encode(self.rows(), tombstone=self.tomb, device_out=True, align=9, device_rows=True) == host
        s.close()
        return host


def row_list(values, null_bytes, r):
    """Row r's list as numpy elements / None, by the rule of khip_sink_rows (sink_array_ref.row_list
    turns a DOUBLE into a Python float; this one keeps the element, whose bits are compared)."""
    out = []
    for v, nb in zip(values[r], null_bytes[r]):
        if nb == 2:
            out.append(None)
        elif nb == 0:
            out.append(v)
        else:
            break
    return out


SCALARS = [("I", "INT32", 0), ("L", "INT64", 1), ("D", "DOUBLE", 2)]


# ------------------------------------------------------------------ 1. shapes

@pytest.mark.parametrize("window", ["NONE", "TUMBLING", "SESSION"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_row_counts_memory_kinds_and_windows(prod, n, window):
    vcols = SCALARS + ([("WSTART", "INT64", "WS")] if window != "NONE" else []) + ([("WEND", "INT64", "WE")] if window == "SESSION" else [])
    host = Table(vcols, n, seed=n + len(window), window=window).check(prod)
    assert n < 255 or (len({len(v) for v in host[1] if v is not None}) > 15 and any(v is None for v in host[1]))


@pytest.mark.parametrize("kfmt", ["JSON", "DELIMITED"])
def test_json_and_delimited_keys(prod, kfmt):
    n = 300
    t = Table(SCALARS, n, seed=11, window="TUMBLING")
    keys = [("k%d,\"%d" % (i % 17, i)) * (1 + i % 3) for i in range(n)]
    s = abi.SinkHandle(prod, kfmt, [("K", "STRING")], "AVRO", SCALARS, window_kind="TUMBLING", avro_schema_id=5)
    t.schema_id = 5
    rows = dict(t.rows(), key=keys)
    exp = t.expected()[1]
    for kw in ({}, {"device_out": True, "align": 3}):
        kb, vb = s.encode(rows, tombstone=t.tomb, **kw)
        assert vb == exp
        for i in range(n):
            assert kb[i] == sink_ref.encode_key(kfmt, [("K", "STRING")], [keys[i]]) + sink_ref.window_suffix("TUMBLING", int(t.ws[i]), 0)
    s.close()


# ------------------------------------------------------------------ 2. values

def test_varint_boundaries_in_every_column_type(prod):
    b64, b32 = boundaries("INT64"), boundaries("INT32")
    n = len(b64)
    t = Table(SCALARS + [("WSTART", "INT64", "WS"), ("WEND", "INT64", "WE")], n, seed=1, window="SESSION", null_rate=0, tomb_rate=0)
    t.values[0] = np.array([b32[i % len(b32)] for i in range(n)], np.int32)
    t.values[1] = np.array(b64, np.int64)
    t.values[2] = np.resize(DOUBLES, n).view(np.float64)
    t.ws = np.array(b64[::-1], np.int64)
    t.we = np.roll(np.array(b64, np.int64), 7)
    host = t.check(prod)
    assert {len(av.optional("INT64", v)) for v in b64} == set(range(2, 12))
    assert {len(av.optional("INT32", v)) for v in b32} == set(range(2, 7))
    assert len({len(v) for v in host[1]}) > 10


def test_nulls_alone_together_and_tombstones(prod):
    """Each column NULL alone, every pair, all three (the value is still there: the header and three
    branch bytes), and tombstones over any of them (a null value)."""
    n = 8 * 40
    t = Table(SCALARS, n, seed=2, tomb_rate=0.2)
    for c in range(3):
        t.nulls[c] = (np.arange(n) >> c) & 1 == 1
    host = t.check(prod)
    all_null = [i for i in range(n) if i % 8 == 7 and not t.tomb[i]]
    assert all_null and all(host[1][i] == b"\x00" + struct.pack(">i", SID) + b"\x00\x00\x00" for i in all_null)
    assert all((host[1][i] is None) == bool(t.tomb[i]) for i in range(n)) and t.tomb.any()


# ------------------------------------------------------------------ 3. past the wave's stage; many and no columns

def test_waves_past_the_stage_beside_waves_that_fit(prod):
    """Five BIGINT columns of 10-byte varints: 5 + 5 x 11 = 60 bytes a row, 3840 a wave, past the
    2048-byte stage, so such a wave writes byte by byte; the tiles mix them with waves of short rows
    (staged), and a wave half of each is long too."""
    vcols = [("C%d" % c, "INT64", c) for c in range(5)]
    n = 3 * 256 + 100
    t = Table(vcols, n, seed=3, null_rate=0, tomb_rate=0.05)
    wave = np.arange(n) // 64
    long_row = (wave % 3 == 0) | ((wave % 3 == 1) & (np.arange(n) % 64 < 32) & (wave % 2 == 0))
    rng = np.random.default_rng(4)
    for c in range(5):
        big = rng.integers(2**62, 2**63 - 1, n) * rng.choice([1, -1], n)
        t.values[c] = np.where(long_row, big, rng.integers(-64, 64, n)).astype(np.int64)
    host = t.check(prod)
    lens = np.array([0 if v is None else len(v) for v in host[1]])
    assert set(lens[long_row & (t.tomb == 0)]) == {60} and set(lens[~long_row & (t.tomb == 0)]) == {15}
    sums = [int(lens[a:a + 64].sum()) for a in range(0, n, 64)]
    assert sum(s > WAVE_STAGE for s in sums) >= 4 and sum(0 < s <= WAVE_STAGE for s in sums) >= 4
    per_tile = [[s > WAVE_STAGE for s in sums[a:a + 4]] for a in range(0, len(sums), 4)]
    assert any(any(x) and not all(x) for x in per_tile)


def test_thirty_two_value_columns(prod):
    types = ["INT32", "INT64", "DOUBLE"]
    vcols = [("C%d" % c, types[c % 3], c) for c in range(30)]
    vcols = vcols[:7] + [("WSTART", "INT64", "WS")] + vcols[7:19] + [("WEND", "INT64", "WE")] + vcols[19:]
    assert len(vcols) == 32
    Table(vcols, 300, seed=5, window="SESSION").check(prod, aligns=(5,))


def test_no_value_columns(prod):
    n = 130
    t = Table([], n, seed=6, window="TUMBLING", schema_id=9)
    host = t.check(prod, aligns=(0, 3))
    assert [v for v in host[1] if v is not None] == [b"\x00\x00\x00\x00\x09"] * int((t.tomb == 0).sum())


# ------------------------------------------------------------------ 4. arrays

LAYOUTS = {
    # an array first, in the middle and last; scalars and the window bounds between them
    "mixed": [("A1", "INT32", 0, 1), ("S", "DOUBLE", 1), ("WSTART", "INT64", "WS"), ("A3", "DOUBLE", 2, 3),
              ("WEND", "INT64", "WE"), ("B3", "INT64", 3, 3)],
    # L = 29 of every type behind a scalar
    "wide": [("S", "INT64", 0), ("D29", "DOUBLE", 1, 29), ("I29", "INT32", 2, 29), ("L29", "INT64", 3, 29)],
    # the remaining (type, L) pairs of {INT32, INT64, DOUBLE} x {1, 3}: array columns only
    "small": [("a", "INT32", 0, 3), ("b", "INT64", 1, 1), ("c", "DOUBLE", 2, 1)],
}


def test_layouts_cover_every_type_and_length():
    got = {(c[1], c[3]) for cols in LAYOUTS.values() for c in cols if len(c) > 3}
    assert got == {(t, L) for t in NP for L in (1, 3, 29)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_array_columns(prod, n, layout):
    t = Table(LAYOUTS[layout], n, seed=n + len(layout), window="SESSION")
    host = t.check(prod, aligns=(0, 7, 13) if n < 1000 else (3,))
    if n >= 255:  # list lengths 0..L and NULL elements occurred
        c = next(c for c in LAYOUTS[layout] if len(c) > 3 and c[3] > 1)
        lists = [row_list(t.values[c[2]], t.nulls[c[2]], i) for i in range(n)]
        assert {len(x) for x in lists} == set(range(c[3] + 1)) and any(None in x for x in lists)
    assert n < 255 or len({len(v) for v in host[1] if v is not None}) > 20


def test_rows_across_the_rounds_of_the_tile_stage(prod):
    """L = 1000, eight full lists of 10-byte elements: 5 + 1 + 2 + 1000 x 11 + 1 bytes a row, so the
    tile's 88 KB leave in three rounds of 32 KB and rows lie across the rounds' edges (such a row is
    encoded once per round, each round keeping its part)."""
    n, L = 8, 1000
    t = Table([("A", "INT64", 0, L)], n, seed=7, tomb_rate=0)
    rng = np.random.default_rng(8)
    t.values[0] = rng.integers(2**62, 2**63 - 1, (n, L)) * rng.choice([1, -1], (n, L))
    t.nulls[0] = np.zeros((n, L), np.uint8)
    host = t.check(prod, aligns=(0, 11))
    lens = [len(v) for v in host[1]]
    assert lens == [5 + 1 + 2 + 11 * L + 1] * n
    end = np.cumsum(lens)
    assert sum(int((e - l) // STAGE != (e - 1) // STAGE) for e, l in zip(end, lens)) >= 2 and end[-1] > 2 * STAGE


def test_tiles_on_both_sides_of_the_tile_stage(prod):
    """Empty lists beside full BIGINT lists of L = 29 with NULL elements: tile 0 leaves in one round,
    the later tiles in several; a last partial tile alternates."""
    n = 3 * 256 + 100
    i = np.arange(n)
    full = np.where(i < 256, False, np.where(i < 512, i >= 384, np.where(i < 768, True, i % 2 == 0)))
    t = Table([("S", "INT32", 1), ("L", "INT64", 0, 29)], n, seed=9)
    rng = np.random.default_rng(10)
    vals, nb = array_column(rng, "INT64", n, 29, lengths=np.where(full, 29, 0), null_rate=0.05)
    big = rng.integers(-2**63, -2**62, (n, 29))
    t.values[0], t.nulls[0] = np.where(nb == 0, big, vals), nb
    host = t.check(prod, aligns=(5,))
    lens = np.array([0 if v is None else len(v) for v in host[1]])
    sums = [int(lens[a:a + 256].sum()) for a in range(0, n, 256)]
    assert 0 < sums[0] <= STAGE < sums[1] and 2 * STAGE < sums[2], sums


def test_sink_fed_by_a_topk_and_latest_by_offset_handle(prod):
    """TOPK(x, 3), LATEST_BY_OFFSET(x, 3, false) and COUNT(*) of one handle: each push's changes()
    go to the sink as they are (values and the library's null bytes)."""
    rng = np.random.default_rng(12)
    desc = abi.make_agg_desc(col_types=["INT64"], aggs=[("TOPK", 0, 3), ("LATEST_BY_OFFSET_NULLS", 0, 3), ("COUNT_STAR", -1)],
                             flags=abi.FLAG_CHANGELOG)
    assert abi.agg_result_len(desc) == [3, 3, 1]
    cols = [("T", "INT64", 3), ("L", "INT64", 3), ("C", "INT64")]
    s = abi.SinkHandle(prod, "KAFKA", [("ID", "INT64")], "AVRO", [("T", "INT64", 0, 3), ("L", "INT64", 1, 3), ("C", "INT64", 2)],
                       avro_schema_id=77)
    h = abi.AggHandle(prod, desc)
    seen, last = {}, {}
    for push in range(6):
        m = 50
        keys = rng.integers(0, 40, m)
        x = elements(rng, "INT64", m)
        valid = rng.random(m) > 0.3
        h.push(abi.HostBatch(np.full(m, push), keys=keys, cols=[x], col_valid=[valid]))
        for k, v, ok in zip(keys, x, valid):
            seen.setdefault(int(k), []).append(int(v) if ok else None)
        chg = h.changes()
        assert chg["n"] > 0
        for device_rows in (False, True):
            kb, vb = s.encode(chg, tombstone=chg["tombstone"], device_rows=device_rows)
            for r in range(chg["n"]):
                row = [ar.row_list(chg["values"][a], chg["null_bytes"][a], r, "INT64") for a in (0, 1)]
                row.append(None if chg["nulls"][2][r] else int(chg["values"][2][r]))
                assert vb[r] == av.encode_value(cols, row, 77, tombstone=bool(chg["tombstone"][r])), (push, r)
                assert kb[r] == struct.pack(">q", int(chg["key"][r]))
                last[int(chg["key"][r])] = vb[r]
    h.close()
    s.close()
    assert set(last) == set(seen)
    for k, xs in seen.items():  # the last record of every key, from the inputs alone
        top = sorted((v for v in xs if v is not None), reverse=True)[:3]
        assert last[k] == av.encode_value(cols, [top, xs[-3:], len(xs)], 77), (k, xs)
    assert any(None in xs[-3:] for xs in seen.values())


# ------------------------------------------------------------------ 5. sizes

@pytest.mark.parametrize("arrays", [False, True], ids=["scalars", "arrays"])
def test_buffer_one_byte_short_then_exact(prod, arrays):
    import torch
    n = 700
    t = Table(LAYOUTS["mixed"] if arrays else SCALARS, n, seed=13, window="SESSION")
    s = t.sink(prod)
    exp = t.expected()
    need = sum(len(v) for v in exp[1] if v is not None)
    kneed = 24 * n
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
    kbuf = torch.full((kneed + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    vbuf = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    out = abi.SinkOut()
    out.mem = abi.MEM_DEVICE
    out.key_offsets, out.key_bytes = koff.data_ptr(), kbuf.data_ptr() + 16
    out.value_offsets, out.value_bytes, out.value_null = voff.data_ptr(), vbuf.data_ptr() + 16, vnull.data_ptr()
    for kcap, vcap in ((kneed, need - 1), (kneed - 1, need)):
        out.key_capacity, out.value_capacity = kcap, vcap
        assert prod.sink_encode(s.h, C.byref(rows), C.byref(out)) == KHIP_E_BUFFER
        assert prod.dll.khip_last_error()
        assert (out.key_len, out.value_len) == (kneed, need)
        assert bool((vbuf == 0xAB).all()) and bool((kbuf == 0xAB).all())  # nothing written
    out.key_capacity, out.value_capacity = kneed, need
    prod.check(prod.sink_encode(s.h, C.byref(rows), C.byref(out)), "sink_encode")
    assert (out.key_len, out.value_len) == (kneed, need)
    kb, vb, ko, vo, vn = (x.cpu().numpy() for x in (kbuf, vbuf, koff, voff, vnull))
    for b, ln in ((kb, kneed), (vb, need)):
        assert (b[:16] == 0xAB).all() and (b[16 + ln:] == 0xAB).all()
    assert [None if vn[i] else vb[16 + vo[i]:16 + vo[i + 1]].tobytes() for i in range(n)] == exp[1]
    assert [kb[16 + ko[i]:16 + ko[i + 1]].tobytes() for i in range(n)] == exp[0]
    assert vo[n] == need and ko[n] == kneed
    s.close()


# ------------------------------------------------------------------ 6. the schema id

def test_schema_ids_and_setting_one_again(prod):
    t = Table(SCALARS, 100, seed=14)
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "AVRO", SCALARS)
    with pytest.raises(abi.KsqlHipError, match=r"\(-7\)"):  # KHIP_E_STATE: no id yet
        s.encode(t.rows(), tombstone=t.tomb)
    assert prod.dll.khip_last_error()
    for sid in (0, 1, 0x01020304, 2**31 - 1, 3):  # the next encode uses the new id
        s.set_avro_schema_id(sid)
        t.schema_id = sid
        for kw in ({}, {"device_out": True, "align": 1}):
            assert s.encode(t.rows(), tombstone=t.tomb, **kw) == t.expected(), sid
    assert prod.sink_set_avro_schema_id(s.h, -1) == KHIP_E_INVALID and prod.dll.khip_last_error()
    assert prod.sink_set_avro_schema_id(s.h, -2**31) == KHIP_E_INVALID
    assert s.encode(t.rows(), tombstone=t.tomb) == t.expected()  # a refused id changes nothing
    s.close()
    j = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "JSON", SCALARS)
    assert prod.sink_set_avro_schema_id(j.h, 1) == KHIP_E_INVALID and prod.dll.khip_last_error()
    with pytest.raises(abi.KsqlHipError, match=r"\(-1\)"):
        abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "JSON", SCALARS, avro_schema_id=1)
    j.close()


def test_rejections_and_names(prod):
    key = [("K", "INT64")]
    for kfmt, kc in (("KAFKA", key), ("JSON", [("A", "INT64"), ("B", "STRING")]), ("DELIMITED", [("A", "INT32"), ("B", "STRING")])):
        abi.SinkHandle(prod, kfmt, kc, "AVRO", [("A", "INT64", 0, 3), ("B", "INT64", 0, 3), ("C", "DOUBLE", 1, 32767)]).close()
    for bad in ([("W", "INT64", "WS", 2)], [("A", "INT64", 0, -1)], [("A", "STRING", 0)], [("A", "INT64", 0, 3), ("B", "INT64", 0, 4)],
                [("A", "INT64", 0, 3), ("B", "INT64", 0)]):
        with pytest.raises(abi.KsqlHipError, match=r"\(-1\)"):
            abi.SinkHandle(prod, "KAFKA", key, "AVRO", bad)
    with pytest.raises(abi.KsqlHipError, match=r"\(-4\)"):  # an AVRO key stays with the reference
        abi.SinkHandle(prod, "AVRO", key, "AVRO", [("A", "INT64", 0)])
    # the binary form carries no names: value_names may be NULL
    vt = (abi.i32 * 2)(abi.TYPE["INT64"], abi.TYPE["DOUBLE"])
    vs = (abi.i32 * 2)(0, 1)
    kt = (abi.i32 * 1)(abi.TYPE["INT64"])
    desc = abi.SinkDesc(abi.FMT["KAFKA"], 1, kt, None, abi.WINDOW["NONE"], abi.FMT["AVRO"], 2, vt, None, vs, 0, 0)
    h = C.c_void_p()
    prod.check(prod.sink_create(C.byref(desc), C.byref(h)), "sink_create")
    prod.check(prod.sink_destroy(h), "sink_destroy")
    # an ARRAY column still needs its null bytes
    s = abi.SinkHandle(prod, "KAFKA", key, "AVRO", [("A", "INT64", 0, 3)], avro_schema_id=1)
    rows = {"n": 4, "key": np.arange(4), "ws": np.zeros(4, np.int64), "we": np.zeros(4, np.int64),
            "values": [np.zeros((4, 3), np.int64)], "nulls": [None]}
    with pytest.raises(abi.KsqlHipError, match=r"\(-1\): .*null"):
        s.encode(rows)
    s.close()


# ------------------------------------------------------------------ 7. round trip on the device

@pytest.mark.parametrize("n", [1, 257, 3000])
def test_the_device_decoder_reads_the_records_back(prod, n):
    """khip_sink_encode's AVRO values through khip_serde_decode with the schema ksqlDB registers for
    these columns: the decoded columns and null bits are the rows, no record fails (a comparison that
    does not pass through the Python restatement)."""
    sid = 0x01020304
    t = Table(SCALARS, n, seed=15 + n, schema_id=sid)
    s = t.sink(prod)
    keys, vals = s.encode(t.rows(), tombstone=t.tomb, device_out=True, align=5)
    s.close()
    fields = [(c[0], c[1], c[2]) for c in SCALARS]
    sd = abi.SerdeHandle(prod, "AVRO", fields, key_type="INT64", avro_schema=avro_ref.ksql_writer_schema(fields), avro_schema_id=sid)
    d, nerr = sd.decode(np.arange(n, dtype=np.int64), keys, vals)
    got = sd.columns(d, [c[1] for c in SCALARS])
    sd.close()
    assert nerr == 0
    assert np.array_equal(got["key"], t.keys) and got["key_valid"].all()
    assert np.array_equal(got["row_valid"], t.tomb == 0)
    live = t.tomb == 0
    for c, (_, typ, src) in enumerate(SCALARS):
        present = live & ~t.nulls[src]
        assert np.array_equal(got["valid"][c][live], ~t.nulls[src][live]), c
        a, b = got["cols"][c][present], t.values[src][present]
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), c  # DOUBLE: the bits


# ------------------------------------------------------------------ 8. the QTT cases, end to end

QTT_CASES = qtt.load_cases("sink_avro")


def test_qtt_fixture_holds_the_cases():
    names = [c["name"] for c in QTT_CASES]
    assert len(names) == 12 and sum("(stream->table) - format [AVRO]" in x for x in names) == 3
    for agg in ("max", "min"):
        assert all("%s %s group by" % (agg, t) in names for t in ("integer", "long", "double"))
    assert all("sum " + t in names for t in ("int", "long", "double"))
    assert all(c["sink"]["value_format"] == "AVRO" and c["sink"]["key_format"] in ("KAFKA", "JSON") for c in QTT_CASES)


def _avro_spec(value, fields):
    """A QTT input value (JSON object) as the Avro record of the source's schema."""
    up = {k.upper(): x for k, x in value.items()}
    rec = {}
    for name, typ, _ in fields:
        x = up.get(name)
        rec[name] = None if x is None else (x if isinstance(x, str) else json.dumps(x)) if typ == "STRING" else \
            float(x) if typ == "DOUBLE" else int(x)
    return rec


def _result_type(case, a):
    ag = case["desc"]["aggs"][a]
    if ag["kind"] in ("COUNT", "COUNT_STAR"):
        return "INT64"
    return "DOUBLE" if ag["kind"] == "AVG" else case["desc"]["col_types"][ag["arg_col"]]


@pytest.mark.parametrize("case", QTT_CASES, ids=[c["name"] for c in QTT_CASES])
def test_qtt_records_to_avro_sink_records(prod, case):
    """One record per push; where the fixture carries the source's AVRO records they are decoded on
    the device first (raw AVRO records -> serde -> aggregate -> changes -> sink).  Keys are sink_ref's;
    values are the restatement's encoding of the row the device emitted and decode (avro_ref) to the
    reference's raw_value — integers exact, doubles within the QTT comparator's 1e-6; tombstones are
    null values."""
    sk, d, raw, sid = case["sink"], case["desc"], case["raw"], 41
    vcols = [(vc["name"], _result_type(case, vc["agg"]), vc["agg"]) if vc["src"] == "AGG" else (vc["name"], "INT64", vc["src"])
             for vc in sk["value_cols"]]
    group = d.get("group")
    kcols = [tuple(k) for k in (group["cols"] if group else sk["key_cols"])]
    s = abi.SinkHandle(prod, sk["key_format"], kcols, "AVRO", vcols, window_kind=d["window_kind"], avro_schema_id=sid)
    h = abi.AggHandle(prod, qtt.case_desc(case))
    sd = None
    if raw:
        assert raw["format"] == "AVRO" and not group
        fields = [(f["name"], f["type"], f["out"]) for f in raw["fields"]]
        writer = avro_ref.ksql_writer_schema(fields)
        sd = abi.SerdeHandle(prod, "AVRO", fields, key_type=raw["key_type"], avro_schema=writer)
    got = []
    for i in range(len(raw["records"] if raw else case["input"])):
        if raw:
            rec = raw["records"][i]
            k, v = rec["key"], rec["value"]
            kb = None if k is None else k.encode() if raw["key_type"] == "STRING" else \
                struct.pack(">q" if raw["key_type"] == "INT64" else ">i", int(k))
            vb = None if v is None else avro_ref.encode(writer, _avro_spec(v, fields))
            batch, _ = sd.decode(np.array([rec["ts"]], np.int64), [kb], [vb])
        else:
            batch = qtt.case_batch(case, i, i + 1)
            if group:  # the composite key, built on the device from the GROUP BY columns
                cols = [[v] if typ == "STRING" else (np.array([0 if v is None else v], np.int32 if typ == "INT32" else np.int64),
                                                      [v is not None]) for (_, typ), v in zip(kcols, case["input"][i]["gvals"])]
                batch = s.key(batch, cols)
        h.push(batch)
        chg = h.changes()
        if chg["n"]:
            keys, vals = s.encode(chg, tombstone=chg["tombstone"], key_serialized=bool(group))
            got += [(keys[r], vals[r], chg, r) for r in range(chg["n"])]
    h.close()
    s.close()
    if sd:
        sd.close()
    exp = case["outputs"]
    assert len(got) == len(exp), (len(got), len(exp))
    fields = [(nm, typ, j) for j, (nm, typ, _) in enumerate(vcols)]
    schema = avro_ref.ksql_writer_schema(fields)
    for i, ((kb, vb, chg, r), o) in enumerate(zip(got, exp)):
        inner = o["key"].encode() if group else sink_ref.encode_key(sk["key_format"], [tuple(sk["key_cols"][0])], [o["key"]])
        assert kb == inner + sink_ref.window_suffix(d["window_kind"], o["ws"], o["we"]), (i, kb)
        if o["tombstone"]:
            assert vb is None, (i, vb)
            continue
        row = [int(chg["ws"][r]) if src == "WS" else int(chg["we"][r]) if src == "WE" else
               None if chg["nulls"][src][r] else py(typ, chg["values"][src][r]) for (_, typ, src) in vcols]
        assert vb == av.encode_value([(v[0], v[1]) for v in vcols], row, sid), (i, vb, row)
        dec = avro_ref.decode_value(fields, schema, vb, sid)
        want = {k.upper(): x for k, x in o["raw_value"].items()}
        assert set(want) <= set(dec), (want, dec)
        for nm, x in want.items():
            g = dec[nm]
            if g is None or x is None:
                assert g is None and x is None, (i, nm, g, x)
            elif isinstance(g, float):
                assert abs(g - x) < 1e-6, (i, nm, g, x)
            else:
                assert type(x) is int and g == x, (i, nm, g, x)
