"""Pins tests/proto_ref.py, the CPU restatement of the PROTOBUF / PROTOBUF_NOSR value formats:
fixed byte vectors made with a real protobuf implementation, a cross-check against google.protobuf
(dynamic proto3 messages from a DescriptorPool, no protoc) where it is importable, and the byte-exact
regeneration of tests/golden/qtt_proto.json.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import proto_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))

COLS = [("A", "INT32"), ("B", "INT64"), ("C", "DOUBLE"), ("D", "INT32", 3), ("E", "DOUBLE", 1), ("O", "INT64")]
# the source side of the same schema: the scalar fields (repeated source fields are out of scope)
WRITER = [("A", "int32", 1, 0), ("B", "int64", 2, 0), ("C", "double", 3, 0), ("O", "int64", 6, 1)]
KSQL = [("A", "INT32"), ("B", "INT64"), ("C", "DOUBLE"), ("O", "INT64")]


def hx(s):
    return bytes.fromhex(s.replace(" ", ""))


# ------------------------------------------------------------------ fixed vectors

def test_vector_every_kind_of_field():
    """A=-1, B=0, C=-0.0, D=[3,-2,0], E=[1.5], O=0 with O the only field with presence."""
    exp = hx("08ffffffffffffffffff01 190000000000000080 220c03feffffffffffffffff0100 2a08000000000000f83f 3000")
    plain = pr.encode_message(COLS[:5], [-1, 0, -0.0, [3, -2, 0], [1.5]], optional=False)
    opt = pr.encode_message(COLS, [None] * 3 + [[], []] + [0], optional=True)
    assert plain + opt == exp
    # the whole row in the optional representation also writes B = 0
    assert pr.encode_message(COLS, [-1, 0, -0.0, [3, -2, 0], [1.5], 0], optional=True) == exp[:11] + hx("1000") + exp[11:]


def test_vector_defaults_are_absent():
    assert pr.encode_message(COLS, [0, 300, 0.0, [], [], None]) == hx("10ac02")
    assert pr.encode_value(COLS, [0, 300, 0.0, [], [], None], "PROTOBUF_NOSR") == hx("10ac02")


def test_vector_framing():
    assert pr.framing(7) == hx("00 00000007 00")
    assert pr.encode_value(COLS, [0, 300, 0.0, [], [], None], "PROTOBUF", schema_id=7) == hx("00 00000007 00 10ac02")
    assert pr.encode_value(COLS, [0, 0, 0.0, [], [], None], "PROTOBUF", schema_id=7) == hx("00 00000007 00")
    assert pr.encode_value(COLS, [0, 0, 0.0, [], [], None], "PROTOBUF_NOSR") == b""
    assert pr.encode_value(COLS, [1, 2, 3.0, [], [], None], "PROTOBUF", schema_id=7, tombstone=True) is None


def test_vector_decode_last_wins_wrong_wire_type_unknown_and_presence():
    msg = hx("0801 1001 0802 1a03010203 3801 2005 2007")
    row = pr.decode_value(WRITER, KSQL, msg, "PROTOBUF_NOSR")
    assert row[0] == 2 and row[1] == 1 and row[3] is None
    assert row[2] == 0.0 and not np.signbit(row[2])
    for head in (hx("00 00000007 00"), hx("00 00000007 0200")):
        assert pr.decode_value(WRITER, KSQL, head + msg, "PROTOBUF", schema_id=7) == row
        assert pr.decode_value(WRITER, KSQL, head + msg, "PROTOBUF", schema_id=-1) == row
        assert pr.decode_value(WRITER, KSQL, head + msg, "PROTOBUF", schema_id=8) is None
    assert pr.decode_value(WRITER, KSQL, hx("00 00000007 0202") + msg, "PROTOBUF", schema_id=7) is None
    assert pr.decode_value(WRITER, KSQL, hx("00 00000007 0400 00") + msg, "PROTOBUF", schema_id=7) is None
    assert pr.decode_value(WRITER, KSQL, hx("01 00000007 00") + msg, "PROTOBUF", schema_id=7) is None
    assert pr.decode_value(WRITER, KSQL, hx("00 00000007"), "PROTOBUF", schema_id=7) is None
    assert pr.decode_value(WRITER, KSQL, b"", "PROTOBUF_NOSR") == [0, 0, np.float64(0.0), None]


def test_negative_int32_is_ten_bytes_and_tags_grow_at_sixteen():
    assert len(pr.field(1, "int32", -1)) == 11
    assert pr.tag(15, 0) == b"\x78" and pr.tag(16, 0) == b"\x80\x01"
    assert len(pr.tag(2047, 0)) == 2 and len(pr.tag(2048, 0)) == 3 and len(pr.tag(pr.MAX_FIELD, 0)) == 5


MALFORMED = {
    "truncated varint": hx("08ff"),
    "varint of 11 bytes": hx("08" + "ff" * 10 + "01"),
    "length past the end": hx("1a05 0102"),
    "fixed64 past the end": hx("19 00000000"),
    "fixed32 past the end": hx("3d 0000"),
    "field number 0": hx("0001"),
    "wire type 3": hx("0b"),
    "wire type 4": hx("0c"),
    "wire type 6": hx("0e"),
    "wire type 7": hx("0f00"),
    "truncated tag": hx("0801 88"),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_records_fail(what):
    assert pr.decode_value(WRITER, KSQL, MALFORMED[what], "PROTOBUF_NOSR") is None
    assert pr.decode_value(WRITER, KSQL, pr.framing(1) + MALFORMED[what], "PROTOBUF", 1) is None


def test_invalid_utf8_fails_only_in_a_string_field():
    w = [("S", "string", 1, 0), ("Y", "bytes", 2, 0)]
    k = [("S", "STRING")]
    assert pr.decode_value(w, k, hx("0a02c328"), "PROTOBUF_NOSR") is None
    assert pr.decode_value(w, k, hx("1202c328"), "PROTOBUF_NOSR") == [""]
    assert pr.decode_value(w, k, hx("1a02c328"), "PROTOBUF_NOSR") == [""]  # unknown field 3
    assert pr.decode_value(w, k, hx("0a02c3a9"), "PROTOBUF_NOSR") == ["é"]


def test_refused_pairing_fails_every_record():
    assert pr.decode_value([("A", "int64", 1, 0)], [("A", "INT32")], hx("0801"), "PROTOBUF_NOSR") is None
    assert pr.decode_value([("A", "bytes", 1, 0)], [("A", "STRING")], b"", "PROTOBUF_NOSR") is None
    assert pr.decode_value([("a", "uint32", 1, 0)], [("A", "INT64")], hx("08ffffffff0f"), "PROTOBUF_NOSR") == [0xFFFFFFFF]


# ------------------------------------------------------------------ against google.protobuf

def gp_class(fields, name):
    """A dynamic proto3 message class: fields [(name, proto type, number, presence[, repeated])]."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fp = descriptor_pb2.FileDescriptorProto(name=name + ".proto", package=name, syntax="proto3")
    en = fp.enum_type.add(name="E")
    for k in range(4):
        en.value.add(name="ENUM_%d" % k, number=k)
    m = fp.message_type.add(name="M")
    for f in fields:
        fd = m.field.add(name=f[0], number=f[2], type=getattr(F, "TYPE_" + f[1].upper()),
                         label=F.LABEL_REPEATED if len(f) > 4 and f[4] else F.LABEL_OPTIONAL)
        if f[1] == "enum":
            fd.type_name = "." + name + ".E"
        if f[3]:
            fd.proto3_optional = True
            fd.oneof_index = len(m.oneof_decl)
            m.oneof_decl.add(name="_" + f[0])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fp)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName(name + ".M"))


def gp_row(cls, writer, data):
    """What google.protobuf reads: per writer field its Connect value, None when a field with presence
    is absent; None for the record when parsing fails."""
    from google.protobuf.message import DecodeError
    m = cls()
    try:
        m.ParseFromString(bytes(data))
    except DecodeError:
        return None
    out = []
    for name, ptype, _, presence in writer:
        if presence and not m.HasField(name):
            out.append(None)
            continue
        v = getattr(m, name)
        if ptype == "enum":
            v = "ENUM_%d" % v
        elif ptype in ("float", "double"):
            v = np.float64(v)
        elif ptype in ("uint64", "fixed64"):
            v = v - (1 << 64) if v >> 63 else v
        out.append(v)
    return out


def ref_row(writer, data):
    try:
        got = pr.parse_message(writer, bytes(data))
    except pr._Bad:
        return None
    return [got[w] if w in got else (None if f[3] else pr.DEFAULT.get(f[1], 0)) for w, f in enumerate(writer)]


def same(a, b):
    if a is None or b is None:
        return a is b
    for x, y in zip(a, b):
        if isinstance(x, np.floating) or isinstance(y, np.floating):
            if x is None or y is None or np.float64(x).view(np.uint64) != np.float64(y).view(np.uint64):
                if not (x is not None and y is not None and np.isnan(x) and np.isnan(y)):
                    return False
        elif x != y:
            return False
    return len(a) == len(b)


def random_value(rng, ptype):
    r = int(rng.integers(0, 4))
    if ptype in ("int32", "sint32", "sfixed32"):
        return [0, -1, -2**31, int(rng.integers(-2**31, 2**31))][r]
    if ptype in ("uint32", "fixed32"):
        return [0, 1, 2**32 - 1, int(rng.integers(0, 2**32))][r]
    if ptype in ("int64", "sint64", "sfixed64"):
        return [0, -1, -2**63, int(rng.integers(-2**63, 2**63 - 1))][r]
    if ptype in ("uint64", "fixed64"):
        return [0, 1, 2**64 - 1, int(rng.integers(0, 2**63)) * 2 + 1][r]
    if ptype == "float":
        return [np.float32(0.0), np.float32(-0.0), np.float32(1.5), np.float32(rng.normal())][r]
    if ptype == "double":
        return [np.float64(0.0), np.float64(-0.0), np.float64(5e-324), np.float64(rng.normal())][r]
    if ptype == "bool":
        return bool(r & 1)
    if ptype == "enum":
        return r
    if ptype == "string":
        return ["", "a", "é中", "x" * int(rng.integers(0, 200))][r]
    return [b"", b"\xff\xfe", b"\0", bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))][r]


def test_sixteen_types_against_google_protobuf():
    pytest.importorskip("google.protobuf")
    rng = np.random.default_rng(5)
    numbers = [1, 15, 16, 2047, 2048, pr.MAX_FIELD] + list(range(2, 12))
    writer = [("f_%s" % t, t, numbers[k], k % 2) for k, t in enumerate(pr.TYPES)]
    cls = gp_class(writer, "t16")
    for trial in range(300):
        m = cls()
        mine = b""
        chosen = {}
        for name, ptype, num, presence in writer:
            if rng.random() < 0.7:
                v = random_value(rng, ptype)
                chosen[num] = (name, ptype, v)
                setattr(m, name, float(v) if ptype in ("float", "double") else v)
        theirs = m.SerializeToString(deterministic=True)
        for num in sorted(chosen):
            name, ptype, v = chosen[num]
            zero = pr.scalar(ptype, v) in (b"\0", b"\0" * 4, b"\0" * 8)
            has = dict((f[2], f[3]) for f in writer)[num]
            if has or not zero:
                mine += pr.field(num, ptype, v)
        assert mine == theirs, (trial, chosen)
        # each side reads the other's bytes alike, and shuffled / duplicated fields too
        assert same(gp_row(cls, writer, mine), ref_row(writer, theirs))
        parts = [pr.field(num, chosen[num][1], chosen[num][2]) for num in chosen] + \
                [pr.field(num, chosen[num][1], random_value(rng, chosen[num][1])) for num in list(chosen)[:3]] + \
                [pr.tag(99, 0) + pr.varint(5), pr.tag(98, 1) + b"\1" * 8, pr.tag(97, 2) + b"\x02ab", pr.tag(96, 5) + b"\2" * 4]
        rng.shuffle(parts)
        blob = b"".join(parts)
        assert same(gp_row(cls, writer, blob), ref_row(writer, blob)), (trial, blob.hex())


def test_sink_rows_against_google_protobuf():
    pytest.importorskip("google.protobuf")
    rng = np.random.default_rng(6)
    for optional in (False, True):
        fields = [("A", "int32", 1, optional), ("B", "int64", 2, optional), ("C", "double", 3, optional),
                  ("D", "int32", 4, 0, True), ("E", "double", 5, 0, True), ("O", "int64", 6, optional)]
        cls = gp_class(fields, "sink%d" % optional)
        for trial in range(300):
            row = [None if rng.random() < 0.2 else random_value(rng, "int32"),
                   None if rng.random() < 0.2 else random_value(rng, "int64"),
                   None if rng.random() < 0.2 else random_value(rng, "double"),
                   [random_value(rng, "int32") for _ in range(int(rng.integers(0, 4)))],
                   [random_value(rng, "double") for _ in range(int(rng.integers(0, 2)))],
                   None if rng.random() < 0.2 else random_value(rng, "int64")]
            m = cls()
            for f, v in zip(fields, row):
                if v is None:
                    continue
                if len(f) > 4:
                    getattr(m, f[0]).extend([float(x) if f[1] == "double" else x for x in v])
                elif optional or pr.scalar(f[1], v) not in (b"\0", b"\0" * 8):
                    setattr(m, f[0], float(v) if f[1] == "double" else v)
            assert pr.encode_message(COLS, row, optional) == m.SerializeToString(deterministic=True), (optional, row)
            # and back: NULL reads as the default without presence, as NULL with it
            back = gp_row(cls, [(n, t, k, int(optional)) for n, t, k, _ in WRITER], pr.encode_message(COLS, row, optional))
            want = [row[0], row[1], row[2], row[5]]
            if not optional:
                want = [0 if v is None else v for v in want[:2]] + [np.float64(0.0) if want[2] is None else want[2]] + \
                       [0 if want[3] is None else want[3]]
            assert same(back, want), (optional, row, back)


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_records_fail_in_google_protobuf_too(what):
    pytest.importorskip("google.protobuf")
    cls = gp_class(WRITER, "bad_" + "".join(c for c in what if c.isalnum()))
    assert gp_row(cls, WRITER, MALFORMED[what]) is None
    assert gp_row(cls, WRITER, hx("0801")) == [1, 0, np.float64(0.0), None]


def test_invalid_utf8_fails_in_google_protobuf_too():
    pytest.importorskip("google.protobuf")
    w = [("S", "string", 1, 0), ("Y", "bytes", 2, 0)]
    cls = gp_class(w, "utf8")
    assert gp_row(cls, w, hx("0a02c328")) is None
    assert gp_row(cls, w, hx("1202c328")) == ["", b"\xc3\x28"]


def test_a_null_list_element_has_no_form():
    with pytest.raises(ValueError):
        pr.encode_message(COLS, [1, 2, 3.0, [1, None], [], None])


# ------------------------------------------------------------------ the ABI, without a device

def test_library_exports_the_setter_and_abi_declares_it():
    import ctypes as C
    import re
    from ksql_amd import abi
    lib = abi.load_product()
    assert hasattr(lib.dll, "khip_sink_set_schema_id") and lib.dll.khip_abi_version() == 8
    assert abi.PRODUCT_ONLY["sink_set_schema_id"] == [C.c_void_p, abi.i32]
    assert abi.FMT["PROTOBUF"] == 5 and abi.FMT["PROTOBUF_NOSR"] == 6 and abi.PROTO_OPTIONAL == 0x100
    header = open(abi.REPO + "/include/ksqldb_hip.h").read()
    assert re.search(r"khip_status khip_sink_set_schema_id\(khip_sink\* s, int32_t schema_id\);", header)
    for name, code in abi.PROTO_TYPE.items():
        assert re.search(r"#define KHIP_PROTO_%s %d\b" % (name.upper(), code), header), name
    assert sorted(abi.PROTO_TYPE) == sorted(pr.TYPES) and sorted(abi.PROTO_TYPE.values()) == list(range(1, 17))
    assert "khip_sink_set_schema_id" in open(abi.REPO + "/INTEGRATION.md").read()


def test_argument_checks_cpu():
    """What the creates and khip_sink_set_schema_id refuse before touching a device."""
    from ksql_amd import abi
    lib = abi.load_product()
    assert lib.sink_set_schema_id(None, 1) == -1 and lib.dll.khip_last_error()
    key = [("A", "INT64")]
    for vf in abi.PROTO_FORMATS:
        for kf in abi.PROTO_FORMATS:  # a protobuf key stays with the reference, sink and serde
            with pytest.raises(abi.KsqlHipError, match=r"\(-4\)"):
                abi.SinkHandle(lib, kf, key, vf, [("X", "INT64", 0)])
            with pytest.raises(abi.KsqlHipError, match=r"\(-4\)"):
                abi.SerdeHandle(lib, vf, [("X", "INT64", 0)], key_format=kf, proto_schema=[("X", "int64", 1, 0)])
        for bad in ([("X", "int64", 0, 0)], [("X", "int64", 1 << 29, 0)], [("X", "int64", 2, 0), ("Y", "int64", 2, 0)], [("X", 0, 1, 0)]):
            with pytest.raises(abi.KsqlHipError, match=r"\(-1\)"):
                abi.SerdeHandle(lib, vf, [("X", "INT64", 0)], proto_schema=bad)
        with pytest.raises(abi.KsqlHipError, match=r"\(-4\)"):
            abi.SerdeHandle(lib, vf, [("X", "INT64", 0)], proto_schema=[("X", abi.PROTO_MESSAGE, 1, 0)])
        with pytest.raises(abi.KsqlHipError, match=r"\(-1\)"):
            abi.SinkHandle(lib, "KAFKA", key, vf, [("S", "STRING", 0)])
    for vf in ("KAFKA", "JSON", "DELIMITED", "AVRO"):  # the representation bit belongs to protobuf
        with pytest.raises(abi.KsqlHipError, match=r"\(-1\).*KHIP_PROTO_OPTIONAL"):
            abi.SinkHandle(lib, "KAFKA", key, vf, [("X", "INT64", 0)], proto_optional=True)


# ------------------------------------------------------------------ the fixture

def test_fixture_regenerates_byte_for_byte(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_fixtures as mf  # the generator's own idea of where the QTT cases are
    if not os.path.isdir(mf.QTT_DIR):
        pytest.skip("reference tree not present")
    out = tmp_path / "qtt_proto.json"
    subprocess.check_call([sys.executable, os.path.join(HERE, "golden", "make_proto_fixtures.py"), str(out)])
    with open(os.path.join(HERE, "golden", "qtt_proto.json"), "rb") as f:
        assert f.read() == out.read_bytes()
