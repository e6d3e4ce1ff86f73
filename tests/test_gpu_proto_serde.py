"""khip_serde_decode for value_format = KHIP_FMT_PROTOBUF / KHIP_FMT_PROTOBUF_NOSR (include/
ksqldb_hip.h, "PROTOBUF values (deserialization)") against tests/proto_ref.py: the columns and
validity bit for bit, and n_errors.

1. every writer type into every column type that accepts it, sparse field numbers, fields out of
   order / duplicated / unknown / with the wrong wire type, unread fields, names by upper-casing,
   presence, over row counts at the wave and block edges, host and device input, both formats;
2. a refused pairing;  3. malformed records at the first, a middle and the last place of a batch
   whose bytes end with the allocation;  4. the framing;  5. null keys and values;  6. create errors;
7. the QTT raw records end to end.
"""
import struct

import numpy as np
import pytest

import proto_ref as pr
import qtt
from ksql_amd import abi

pytestmark = pytest.mark.gpu

KHIP_E_INVALID, KHIP_E_UNSUPPORTED = -1, -4
NP = {"INT32": np.int32, "INT64": np.int64, "DOUBLE": np.float64, "STRING": np.int64}
SID = 0x0A0B0C0D
BIG = pr.MAX_FIELD


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


# ------------------------------------------------------------------ schemas

INT32S = ("int32", "sint32", "sfixed32")
INTS = INT32S + ("uint32", "fixed32", "int64", "sint64", "sfixed64", "uint64", "fixed64")
NUMBERS = [1, 15, 16, 2047, 2048, BIG, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 32, 33, 100, 1000, 70000, 1 << 20, 1 << 28,
           BIG - 1, 4, 6, 8, 9, 10, 12, 14]


def numeric_schema():
    """INT ← the three 32-bit types, BIGINT ← all ten integer types, DOUBLE ← float / double: fifteen
    columns, names matched exactly or by upper-casing, presence on every other field; a bytes field
    that no column names, a string field whose column is not read (field_out = -1) and a column no
    writer field names."""
    writer, fields = [], []
    pairs = [(t, "INT32") for t in INT32S] + [(t, "INT64") for t in INTS] + [("float", "DOUBLE"), ("double", "DOUBLE")]
    for k, (pt, kt) in enumerate(pairs):
        col = "C%d_%s" % (k, pt.upper())
        writer.append((col if k % 3 else col.lower(), pt, NUMBERS[k], k % 2))
        fields.append((col, kt, k))
    writer.append(("blob", "bytes", NUMBERS[15], 0))
    writer.append(("UNREAD", "string", NUMBERS[16], 1))
    fields.append(("UNREAD", "STRING", -1))
    fields.append(("NOBODY", "INT64", 15))
    order = np.random.default_rng(1).permutation(len(writer))  # the writer's order is not the numbers'
    return [writer[i] for i in order], fields


def string_schema():
    """STRING ← every type but bytes."""
    writer, fields = [], []
    for k, pt in enumerate(t for t in pr.TYPES if t != "bytes"):
        writer.append(("s_%s" % pt, pt, NUMBERS[31 - k], (k + 1) % 2))
        fields.append(("S_%s" % pt.upper(), "STRING", k))
    return writer, fields


def value_of(rng, pt):
    r = int(rng.integers(0, 5))
    if pt in INT32S:
        return [0, -1, -2**31, 2**31 - 1, int(rng.integers(-2**31, 2**31))][r]
    if pt in ("uint32", "fixed32"):
        return [0, 1, 2**32 - 1, 2**31, int(rng.integers(0, 2**32))][r]
    if pt in ("uint64", "fixed64"):
        return [0, 1, 2**64 - 1, 2**63, int(rng.integers(0, 2**63))][r]
    if pt in ("int64", "sint64", "sfixed64"):
        return [0, -1, -2**63, 2**63 - 1, int(rng.integers(-2**63, 2**63 - 1))][r]
    if pt == "float":
        return np.array([0, 0x80000000, 0x7FC00001, 0x00000001, int(rng.integers(0, 2**32))], np.uint32).view(np.float32)[r]
    if pt == "double":
        return np.array([0, 1 << 63, 0x7FF80000DEADBEEF, 1, int(rng.integers(0, 2**63))], np.uint64).view(np.float64)[r]
    if pt == "bool":
        return bool(r & 1)
    if pt == "enum":
        return r
    if pt == "string":
        return ["", "a", "é中😀", "x" * int(rng.integers(0, 40)), "\x7f"][r]
    return bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8))


WRONG = {0: (1, b"\x11" * 8), 1: (5, b"\x22" * 4), 5: (2, b"\x03abc"), 2: (0, b"\x96\x01")}  # wire type → another one


def message(rng, writer):
    """A well-formed message: fields absent, once or several times, unknown fields of every wire type,
    known numbers with the wrong wire type, all shuffled."""
    parts = []
    for name, pt, num, _ in writer:
        r = rng.random()
        for _ in range(0 if r < 0.25 else 1 if r < 0.8 else 3):
            parts.append(pr.field(num, pt, value_of(rng, pt)))
        if rng.random() < 0.15:
            wt, payload = WRONG[pr.wire_type(pt)]
            parts.append(pr.tag(num, wt) + payload)
    known = {w[2] for w in writer}
    for wt, payload in ((0, pr.varint(int(rng.integers(0, 2**63)))), (1, b"\x01" * 8), (2, b"\x05hello"), (5, b"\x02" * 4)):
        if rng.random() < 0.3:
            num = int(rng.choice([21, 34, 999, 1 << 27, BIG - 2]))
            assert num not in known
            parts.append(pr.tag(num, wt) + payload)
    order = rng.permutation(len(parts))
    return b"".join(parts[i] for i in order)


def frame(rng, fmt, msg, sid=SID):
    return (pr.framing(sid, long_form=rng.random() < 0.3) if fmt == "PROTOBUF" else b"") + msg


# ------------------------------------------------------------------ decode and compare

def pack(items, pad=True):
    n = len(items)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([0 if x is None else len(x) for x in items])
    data = np.frombuffer(b"".join(b"" if x is None else x for x in items) + (b"\0" if pad else b""), np.uint8).copy()
    return offs, data, np.array([x is not None for x in items], bool)


def decode(prod, fmt, writer, fields, keys, vals, sid=SID, device=False):
    n = len(vals)
    sd = abi.SerdeHandle(prod, fmt, fields, key_type="INT64", proto_schema=writer, avro_schema_id=sid)
    ts = np.arange(n, dtype=np.int64)
    if device:
        import torch
        # the value bytes end with their allocation: a read past a record's end leaves the tensor
        koff, kb, kv = pack(keys)
        voff, vb, vv = pack(vals, pad=False)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        vbt = dev(vb) if len(vb) else torch.zeros(0, dtype=torch.uint8, device="cuda")
        d, nerr = sd.decode_device(dev(ts), dev(koff), dev(kb), dev(voff), vbt, key_valid=dev(abi.bitmap(kv)) if not kv.all() else None,
                                   value_valid=dev(abi.bitmap(vv)) if not vv.all() else None)
    else:
        d, nerr = sd.decode(ts, keys, vals)
    n_out = max(f[2] for f in fields) + 1
    types = ["INT64"] * n_out
    for _, t, o in fields:
        if o >= 0:
            types[o] = t
    got = sd.columns(d, types)
    sd.close()
    return got, nerr


def check(prod, fmt, writer, fields, keys, vals, sid=SID, device=False):
    got, nerr = decode(prod, fmt, writer, fields, keys, vals, sid, device)
    cols = [(f[0], f[1]) for f in fields]
    experr = 0
    for i, (k, v) in enumerate(zip(keys, vals)):
        row = None if v is None else pr.decode_value(writer, cols, v, fmt, sid)
        bad = v is not None and row is None
        experr += bad
        assert got["key_valid"][i] == (k is not None and not bad), (i, "key_valid")
        assert got["row_valid"][i] == (v is not None and not bad), (i, "row_valid", v.hex() if v else v)
        if k is not None and not bad:
            assert got["key"][i] == struct.unpack(">q", k)[0]
        for f, (name, typ, out) in enumerate(fields):
            if out < 0:
                continue
            want = None if row is None else row[f]
            assert got["valid"][out][i] == (want is not None), (i, name, want, v.hex() if v else v)
            if want is None:
                continue
            g = got["cols"][out][i]
            if typ == "STRING":
                assert g == 0, (i, name)
            elif typ == "DOUBLE":
                assert g.view(np.uint64) == np.float64(want).view(np.uint64), (i, name, g, want)
            else:
                assert g.dtype == NP[typ] and int(g) == want, (i, name, g, want)
    assert nerr == experr
    return experr


def keys_of(rng, n, null_rate=0.0):
    return [None if rng.random() < null_rate else struct.pack(">q", int(rng.integers(-2**63, 2**63 - 1))) for _ in range(n)]


# ------------------------------------------------------------------ 1. types, numbers, shapes

@pytest.mark.parametrize("fmt", ["PROTOBUF", "PROTOBUF_NOSR"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_numeric_columns_over_row_counts(prod, n, fmt):
    rng = np.random.default_rng(n)
    writer, fields = numeric_schema()
    vals = [frame(rng, fmt, message(rng, writer)) for _ in range(n)]
    keys = keys_of(rng, n)
    assert check(prod, fmt, writer, fields, keys, vals) == 0
    assert check(prod, fmt, writer, fields, keys, vals, device=True) == 0


def test_numeric_schema_covers_the_field_numbers_and_pairings():
    writer, fields = numeric_schema()
    assert {1, 15, 16, 2047, 2048, BIG} <= {w[2] for w in writer}
    cols = {f[0]: f[1] for f in fields}
    pairs = {(w[1], cols[w[0].upper()]) for w in writer if w[0].upper() in cols and w[1] != "string"}
    assert pairs == {(t, "INT32") for t in INT32S} | {(t, "INT64") for t in INTS} | {("float", "DOUBLE"), ("double", "DOUBLE")}
    assert any(w[0] != w[0].upper() for w in writer) and any(w[0] == w[0].upper() for w in writer)
    assert {w[3] for w in writer} == {0, 1}


@pytest.mark.parametrize("fmt", ["PROTOBUF", "PROTOBUF_NOSR"])
def test_string_columns_from_every_type(prod, fmt):
    rng = np.random.default_rng(3)
    writer, fields = string_schema()
    assert {w[1] for w in writer} == set(pr.TYPES) - {"bytes"}
    n = 300
    vals = [frame(rng, fmt, message(rng, writer)) for _ in range(n)]
    for device in (False, True):
        assert check(prod, fmt, writer, fields, keys_of(rng, n), vals, device=device) == 0


def test_absent_fields_and_the_empty_message(prod):
    """A zero-length NOSR value: every field without presence reads as its default, with presence as
    NULL, a column no field names as NULL; the same behind the PROTOBUF framing."""
    writer = [("A", "int32", 1, 0), ("B", "int64", 2, 1), ("C", "double", 3, 0), ("S", "string", 4, 0), ("T", "string", 5, 1)]
    fields = [("A", "INT32", 0), ("B", "INT64", 1), ("C", "DOUBLE", 2), ("S", "STRING", 3), ("T", "STRING", 4), ("X", "INT64", 5)]
    for fmt, empty in (("PROTOBUF_NOSR", b""), ("PROTOBUF", pr.framing(SID))):
        vals = [empty, frame(np.random.default_rng(0), fmt, pr.field(2, "int64", 0)), empty]
        for device in (False, True):
            got, nerr = decode(prod, fmt, writer, fields, keys_of(np.random.default_rng(1), 3), vals, device=device)
            assert nerr == 0 and got["row_valid"].all()
            assert [bool(got["valid"][c][0]) for c in range(6)] == [True, False, True, True, False, False]
            assert got["valid"][1][1] and got["cols"][1][1] == 0
            assert got["cols"][0][0] == 0 and got["cols"][2][0].view(np.uint64) == 0
            check(prod, fmt, writer, fields, keys_of(np.random.default_rng(1), 3), vals, device=device)


def test_two_writer_fields_for_one_column(prod):
    """`a` and `A` both land in column A (exact name, then upper-cased): the translator sets the columns
    in writer order, so the later writer field owns the column whatever the wire order."""
    fields = [("A", "INT64", 0)]
    for writer in ([("a", "int64", 1, 0), ("A", "int64", 2, 1)], [("A", "int64", 2, 1), ("a", "int64", 1, 0)]):
        vals = [pr.field(1, "int64", 5) + pr.field(2, "int64", 6), pr.field(2, "int64", 6) + pr.field(1, "int64", 5),
                pr.field(1, "int64", 5), pr.field(2, "int64", 6), b""]
        check(prod, "PROTOBUF_NOSR", writer, fields, keys_of(np.random.default_rng(2), 5), vals)


# ------------------------------------------------------------------ 2. a refused pairing

@pytest.mark.parametrize("pair", [("int64", "INT32"), ("double", "INT64"), ("bool", "INT64"), ("bytes", "STRING"), ("int32", "DOUBLE")])
def test_a_refused_pairing_fails_every_record(prod, pair):
    writer = [("A", pair[0], 1, 0), ("B", "int64", 2, 0)]
    fields = [("A", pair[1], 0), ("B", "INT64", 1)]
    vals = [b"", pr.field(2, "int64", 7), None, pr.field(2, "int64", 8)]
    assert check(prod, "PROTOBUF_NOSR", writer, fields, keys_of(np.random.default_rng(4), 4), vals) == 3


# ------------------------------------------------------------------ 3. malformed records

W3 = [("A", "int32", 1, 0), ("B", "int64", 2, 0), ("C", "double", 3, 0), ("S", "string", 4, 0), ("F", "float", 7, 0), ("O", "int64", 6, 1)]
F3 = [("A", "INT32", 0), ("B", "INT64", 1), ("C", "DOUBLE", 2), ("S", "STRING", 3), ("F", "DOUBLE", 4), ("O", "INT64", 5)]
GOOD = pr.field(1, "int32", 1)
MALFORMED = {
    "truncated varint": GOOD + bytes.fromhex("10ff"),
    "varint of 11 bytes": GOOD + bytes.fromhex("10" + "ff" * 10 + "01"),
    "truncated tag": GOOD + bytes.fromhex("88"),
    "tag of 11 bytes": GOOD + bytes.fromhex("ff" * 10 + "01"),
    "length past the end": GOOD + bytes.fromhex("2205 6162"),
    "length of 2^31": GOOD + bytes.fromhex("22 8080808008"),
    "length varint truncated": GOOD + bytes.fromhex("22 80"),
    "fixed64 past the end": GOOD + bytes.fromhex("19 00000000000000"),
    "fixed32 past the end": GOOD + bytes.fromhex("3d 000000"),
    "unknown fixed64 past the end": GOOD + bytes.fromhex("a106 0000"),
    "field number 0": GOOD + bytes.fromhex("0001"),
    "wire type 3": GOOD + bytes.fromhex("0b"),
    "wire type 4": GOOD + bytes.fromhex("0c"),
    "wire type 6": GOOD + bytes.fromhex("0e00"),
    "wire type 7": GOOD + bytes.fromhex("0f00"),
    "invalid UTF-8": GOOD + bytes.fromhex("2202c328"),
    "truncated UTF-8": GOOD + bytes.fromhex("2201e4"),
}


@pytest.mark.parametrize("fmt", ["PROTOBUF", "PROTOBUF_NOSR"])
@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_record_first_middle_and_last(prod, what, fmt):
    """The bad record fails alone: its neighbours decode, and (device input, the bytes ending with the
    allocation) nothing is read past the end of the value bytes."""
    rng = np.random.default_rng(len(what))
    n = 130
    good = [frame(rng, fmt, message(rng, W3)) for _ in range(n)]
    bad = frame(rng, fmt, MALFORMED[what])
    assert pr.decode_value(W3, [(f[0], f[1]) for f in F3], bad, fmt, SID) is None
    for place in (0, 70, n - 1):
        vals = list(good)
        vals[place] = bad
        assert check(prod, fmt, W3, F3, keys_of(rng, n), vals, device=True) == 1
    vals = list(good)
    vals[0] = vals[70] = vals[n - 1] = bad
    assert check(prod, fmt, W3, F3, keys_of(rng, n), vals) == 3


# ------------------------------------------------------------------ 4. the framing

def test_framing_index_forms_magic_and_schema_id(prod):
    msg = pr.field(1, "int32", 5) + pr.field(2, "int64", -7)
    head = lambda magic, sid, idx: bytes([magic]) + struct.pack(">i", sid) + idx
    vals = [head(0, SID, b"\x00") + msg,          # [0], short form
            head(0, SID, b"\x02\x00") + msg,      # [0], long form
            head(0, SID, b"\x02\x02") + msg,      # [1]: another message of the schema
            head(0, SID, b"\x04\x00\x00") + msg,  # [0, 0]: a nested message
            head(1, SID, b"\x00") + msg,          # wrong magic
            head(0, SID + 1, b"\x00") + msg,      # another schema id
            head(0, SID, b""),                    # five bytes
            head(0, SID, b"\x02"),                # the list cut short
            head(0, SID, b"\x00"),                # the framing alone: the empty message
            b"", b"\x00"]
    n = len(vals)
    for device in (False, True):
        assert check(prod, "PROTOBUF", W3, F3, keys_of(np.random.default_rng(5), n), vals, device=device) == 8
    # no expected id: any id passes
    assert check(prod, "PROTOBUF", W3, F3, keys_of(np.random.default_rng(5), n), vals, sid=-1) == 7
    # NOSR ignores avro_schema_id and has no framing: the bare message
    assert check(prod, "PROTOBUF_NOSR", W3, F3, keys_of(np.random.default_rng(5), 2), [msg, b""], sid=99) == 0


# ------------------------------------------------------------------ 5. null keys and values

@pytest.mark.parametrize("fmt", ["PROTOBUF", "PROTOBUF_NOSR"])
def test_null_keys_and_null_values(prod, fmt):
    rng = np.random.default_rng(6)
    n = 700
    vals = [None if rng.random() < 0.2 else frame(rng, fmt, message(rng, W3)) for _ in range(n)]
    keys = keys_of(rng, n, null_rate=0.2)
    for device in (False, True):
        assert check(prod, fmt, W3, F3, keys, vals, device=device) == 0
    assert any(k is None and v is None for k, v in zip(keys, vals))


# ------------------------------------------------------------------ 6. create errors

def _create(prod, value_format, fields, proto_schema, key_format="KAFKA"):
    try:
        abi.SerdeHandle(prod, value_format, fields, proto_schema=proto_schema, key_format=key_format).close()
        return 0
    except abi.KsqlHipError as e:
        return int(str(e).split("(")[1].split(")")[0])


def test_create_errors(prod):
    f = [("A", "INT64", 0)]
    assert _create(prod, "PROTOBUF", f, [("A", "int64", 1, 0)]) == 0
    assert _create(prod, "PROTOBUF", f, [("A", "int64", BIG, 1)]) == 0
    for bad in ([("A", "int64", 0, 0)], [("A", "int64", BIG + 1, 0)], [("A", "int64", 3, 0), ("B", "int32", 3, 1)],
                [("A", 0, 1, 0)], [("A", 18, 1, 0)], [("A", 31, 1, 0)]):
        assert _create(prod, "PROTOBUF_NOSR", f, bad) == KHIP_E_INVALID, bad
    for kind in ([("A", abi.PROTO_MESSAGE, 1, 0)], [("A", abi.PROTO_TYPE["int64"] | abi.PROTO_REPEATED, 1, 0)]):
        assert _create(prod, "PROTOBUF", f, kind) == KHIP_E_UNSUPPORTED
    for kf in ("PROTOBUF", "PROTOBUF_NOSR"):
        assert _create(prod, "PROTOBUF", f, [("A", "int64", 1, 0)], key_format=kf) == KHIP_E_UNSUPPORTED
    assert prod.dll.khip_abi_version() == 8


# ------------------------------------------------------------------ 7. the QTT raw records, end to end

RAW_CASES = [c for c in qtt.load_cases("proto") if c.get("raw")]


def test_fixture_has_raw_cases():
    assert RAW_CASES and all(c["raw"]["format"] in abi.PROTO_FORMATS and c["null_as_default"] for c in RAW_CASES)


@pytest.mark.parametrize("case", RAW_CASES, ids=[c["name"] for c in RAW_CASES])
def test_qtt_raw_records_end_to_end(prod, case):
    """The source's serialized records → khip_serde_decode → khip_agg_push (one record per push) → the
    reference's expected output sequence."""
    raw = case["raw"]
    fields = [(f["name"], f["type"], f["out"]) for f in raw["fields"]]
    ptype = {"INT32": "int32", "INT64": "int64", "DOUBLE": "double", "STRING": "string"}
    writer = [(f[0], ptype[f[1]], i + 1, 0) for i, f in enumerate(fields)]  # the schema ksqlDB derives from the columns
    sd = abi.SerdeHandle(prod, raw["format"], fields, key_type=raw["key_type"], proto_schema=writer,
                         avro_schema_id=-1 if raw["schema_id"] is None else raw["schema_id"])
    h = abi.AggHandle(prod, qtt.case_desc(case))
    rows = []
    for rec in raw["records"]:
        k = rec["key"]
        kb = None if k is None else k.encode() if raw["key_type"] == "STRING" else \
            struct.pack(">q" if raw["key_type"] == "INT64" else ">i", int(k))
        vb = None if rec["value_hex"] is None else bytes.fromhex(rec["value_hex"])
        d, nerr = sd.decode(np.array([rec["ts"]], np.int64), [kb], [vb])
        assert nerr == 0
        h.push(d)
        rows += qtt._rows_of(h.changes())
    snap = h.snapshot()
    h.close()
    sd.close()
    assert qtt.compare_outputs(case, rows) == []
    assert qtt.compare_agg(case, snap) == []
