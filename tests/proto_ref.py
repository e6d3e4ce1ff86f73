"""CPU restatement of the PROTOBUF / PROTOBUF_NOSR value formats (TEST INFRASTRUCTURE, like
avro_ref.py and avro_sink_ref.py: the checker of khip_serde_decode and khip_sink_encode for
KHIP_FMT_PROTOBUF and KHIP_FMT_PROTOBUF_NOSR).

The reference builds Confluent's ProtobufConverter (protobuf/ProtobufSerdeFactory.java:168-260) or,
with no registry, ProtobufNoSRConverter (protobuf/ProtobufNoSRConverter.java:56-157: Message.writeTo
and DynamicMessage.parseFrom); both read through ConnectDataTranslator.  Neither Confluent's classes
nor protobuf-java are vendored there, so what they do is restated here from the protobuf encoding
specification and Confluent's published wire format, and pinned by test_proto_ref.py: fixed byte
vectors made with a real protobuf implementation, and a cross-check against google.protobuf where
that is importable.

Framing (PROTOBUF): byte 0, the schema id as 4 bytes big-endian, the message-index list (zig-zag
varint count, then the indexes; [0] is the single byte 0), the message.  PROTOBUF_NOSR: the bare
message.

Writing.  Column i (from 0) is field i + 1; INT32 = int32, INT64 = int64, DOUBLE = double, an ARRAY
column a packed repeated field.  A column is (name, type) for a scalar and (name, type, L) for an
ARRAY of L slots; an ARRAY's value is a Python list, a scalar's a number or None.  A DOUBLE given as
a numpy float64 keeps its bits.  Default representation: a scalar is written when it is non-NULL and
its raw bits are not zero; `optional`: whenever it is non-NULL.  A NULL list element has no protobuf
form (ValueError).

Reading.  writer_schema: [(name, proto type, number, presence)], any of the sixteen scalar types;
columns: [(name, INT32 / INT64 / DOUBLE / STRING)].  DynamicMessage's rules: fields in any order,
the last occurrence wins, unknown numbers and known numbers with another wire type are skipped, a
string must be valid UTF-8; a malformed record is None.  Known divergence from protobuf-java: an
unknown proto2 group (wire type 3) fails the record here.
"""
import struct

import numpy as np

TYPES = ("int32", "sint32", "sfixed32", "uint32", "fixed32", "int64", "sint64", "sfixed64", "uint64", "fixed64",
         "float", "double", "bool", "string", "bytes", "enum")
WIRE = {"sfixed32": 5, "fixed32": 5, "float": 5, "sfixed64": 1, "fixed64": 1, "double": 1, "string": 2, "bytes": 2}
CONNECT = {"int32": "INT32", "sint32": "INT32", "sfixed32": "INT32", "float": "FLOAT32", "double": "FLOAT64",
           "bool": "BOOLEAN", "string": "STRING", "enum": "STRING", "bytes": "BYTES"}  # every other: INT64
# ConnectDataTranslator.validateSchema (:123-146): the Connect types a ksql column accepts
ACCEPTS = {"INT32": {"INT32"}, "INT64": {"INT32", "INT64"}, "DOUBLE": {"FLOAT32", "FLOAT64"},
           "STRING": {"INT32", "INT64", "FLOAT32", "FLOAT64", "BOOLEAN", "STRING"}}
MAX_FIELD = (1 << 29) - 1
M64 = (1 << 64) - 1


def wire_type(ptype):
    return WIRE.get(ptype, 0)


def connect_type(ptype):
    return CONNECT.get(ptype, "INT64")


def varint(u):
    """Base-128 varint of an unsigned value (a negative one as its 64-bit two's complement)."""
    u &= M64
    out = bytearray()
    while u >> 7:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def zigzag(v, bits=64):
    return ((v << 1) ^ (v >> (bits - 1))) & ((1 << bits) - 1)


def tag(number, wt):
    return varint(number << 3 | wt)


def _double(v):
    if isinstance(v, np.floating):
        return struct.pack("<Q", int(np.array(v, np.float64).view(np.uint64)))
    return struct.pack("<d", v)


def _float(v):
    if isinstance(v, np.floating):
        return struct.pack("<I", int(np.array(v, np.float32).view(np.uint32)))
    return struct.pack("<f", v)


def scalar(ptype, v):
    """The bytes of one value of a protobuf scalar type, without its tag."""
    if ptype in ("int32", "int64", "uint32", "uint64", "enum"):
        return varint(int(v))
    if ptype == "sint32":
        return varint(zigzag(int(v), 32))
    if ptype == "sint64":
        return varint(zigzag(int(v), 64))
    if ptype == "bool":
        return varint(1 if v else 0)
    if ptype in ("sfixed32", "fixed32"):
        return struct.pack("<I", int(v) & 0xFFFFFFFF)
    if ptype in ("sfixed64", "fixed64"):
        return struct.pack("<Q", int(v) & M64)
    if ptype == "float":
        return _float(v)
    if ptype == "double":
        return _double(v)
    b = v.encode("utf-8") if isinstance(v, str) else bytes(v)
    return varint(len(b)) + b


def field(number, ptype, v):
    """One field on the wire: its tag and value."""
    return tag(number, wire_type(ptype)) + scalar(ptype, v)


def framing(schema_id, long_form=False):
    return b"\x00" + struct.pack(">i", schema_id) + (b"\x02\x00" if long_form else b"\x00")


# ------------------------------------------------------------------ the sink's value

PTYPE = {"INT32": "int32", "INT64": "int64", "DOUBLE": "double"}


def _is_zero(typ, v):
    if typ == "DOUBLE":
        return _double(v) == b"\0" * 8
    return int(v) == 0


def encode_message(cols, row, optional=False):
    out = b""
    for i, (c, v) in enumerate(zip(cols, row)):
        pt = PTYPE[c[1]]
        if len(c) > 2:
            if any(x is None for x in v):
                raise ValueError("a NULL array element has no protobuf form")
            if v:
                payload = b"".join(scalar(pt, x) for x in v)
                out += tag(i + 1, 2) + varint(len(payload)) + payload
        elif v is not None and (optional or not _is_zero(c[1], v)):
            out += field(i + 1, pt, v)
    return out


def encode_value(cols, row, fmt, schema_id=None, optional=False, tombstone=False):
    """The record value of a row in fmt (PROTOBUF / PROTOBUF_NOSR); None for a tombstone."""
    if tombstone:
        return None
    head = framing(schema_id) if fmt == "PROTOBUF" else b""
    return head + encode_message(cols, row, optional)


# ------------------------------------------------------------------ the deserializer

class _Bad(Exception):
    pass


def _read_varint(b, j):
    v = 0
    for k in range(10):
        if j >= len(b):
            raise _Bad("truncated varint")
        x = b[j]
        j += 1
        v |= (x & 0x7F) << (7 * k)
        if not x & 0x80:
            return v & M64, j
    raise _Bad("varint longer than 10 bytes")


def _s32(u):
    u &= 0xFFFFFFFF
    return u - (1 << 32) if u >> 31 else u


def _s64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def _unzz(u, bits):
    u &= (1 << bits) - 1
    return (u >> 1) ^ -(u & 1)


def _value(ptype, raw):
    """raw: the varint / fixed value (unsigned) or the bytes of a length-delimited field → the Connect
    value: an int, a numpy float64, a bool, a str or bytes."""
    if ptype in ("int32", "sfixed32"):
        return _s32(raw)
    if ptype == "sint32":
        return _unzz(raw, 32)
    if ptype in ("uint32", "fixed32"):
        return raw & 0xFFFFFFFF
    if ptype == "sint64":
        return _unzz(raw, 64)
    if ptype in ("int64", "uint64", "sfixed64", "fixed64"):
        return _s64(raw)
    if ptype == "float":
        return np.float64(np.array(raw & 0xFFFFFFFF, np.uint32).view(np.float32))  # (double) f
    if ptype == "double":
        return np.array(raw, np.uint64).view(np.float64)[()]
    if ptype == "bool":
        return raw != 0
    if ptype == "enum":
        return "ENUM_%d" % _s32(raw)  # the symbol's name: only its presence is observable here
    if ptype == "string":
        return raw.decode("utf-8")
    return bytes(raw)


DEFAULT = {"float": np.float64(0.0), "double": np.float64(0.0), "bool": False, "string": "", "bytes": b"",
           "enum": "ENUM_0"}


def parse_message(writer_schema, b):
    """{writer field index: Connect value} of the fields that occurred; raises _Bad."""
    by_num = {num: w for w, (_, _, num, _) in enumerate(writer_schema)}
    got = {}
    j = 0
    while j < len(b):
        t, j = _read_varint(b, j)
        t &= 0xFFFFFFFF
        num, wt = t >> 3, t & 7
        if num == 0:
            raise _Bad("field number 0")
        if wt == 0:
            raw, j = _read_varint(b, j)
        elif wt == 1:
            if len(b) - j < 8:
                raise _Bad("fixed64 past the end")
            raw = struct.unpack_from("<Q", b, j)[0]
            j += 8
        elif wt == 5:
            if len(b) - j < 4:
                raise _Bad("fixed32 past the end")
            raw = struct.unpack_from("<I", b, j)[0]
            j += 4
        elif wt == 2:
            ln, j = _read_varint(b, j)
            ln = _s32(ln)
            if ln < 0 or ln > len(b) - j:
                raise _Bad("length past the end")
            raw = bytes(b[j:j + ln])
            j += ln
        else:
            raise _Bad("wire type %d" % wt)
        w = by_num.get(num)
        if w is None:
            continue
        ptype = writer_schema[w][1]
        if wire_type(ptype) != wt:
            continue
        try:
            got[w] = _value(ptype, raw)
        except UnicodeDecodeError:
            raise _Bad("invalid UTF-8 in a string field")
    return got


def upper(name):
    return name.upper()  # Java's toUpperCase for the names these tests use


def column_of(writer_name, columns):
    """ConnectDataTranslator.toKsqlStruct (:290-318): the column of the same name, else of the
    upper-cased name; or None."""
    names = [c[0] for c in columns]
    if writer_name in names:
        return names.index(writer_name)
    if upper(writer_name) in names:
        return names.index(upper(writer_name))
    return None


def compatible(writer_schema, columns):
    for name, ptype, _, _ in writer_schema:
        c = column_of(name, columns)
        if c is not None and connect_type(ptype) not in ACCEPTS[columns[c][1]]:
            return False
    return True


def strip_framing(b, schema_id=None):
    """The message bytes of a PROTOBUF value; raises _Bad."""
    if len(b) < 6 or b[0] != 0:
        raise _Bad("framing")
    if schema_id is not None and schema_id >= 0 and struct.unpack_from(">i", b, 1)[0] != schema_id:
        raise _Bad("schema id")
    cnt, j = _read_varint(b, 5)
    if cnt != 0:
        if cnt != 2:
            raise _Bad("message index list")
        idx, j = _read_varint(b, j)
        if idx != 0:
            raise _Bad("message index")
    return b[j:]


def decode_value(writer_schema, columns, data, fmt, schema_id=None):
    """The ksql row of a record value: a list with, per column, None (NULL), an int (INT32 / INT64), a
    numpy float64 (DOUBLE) or a str (STRING: String.valueOf of the value; the device keeps only its
    presence).  None when the record fails to deserialize."""
    data = bytes(data)
    try:
        if not compatible(writer_schema, columns):
            raise _Bad("a writer type its column does not accept")
        msg = strip_framing(data, schema_id) if fmt == "PROTOBUF" else data
        got = parse_message(writer_schema, msg)
    except _Bad:
        return None
    row = [None] * len(columns)
    for w, (name, ptype, _, presence) in enumerate(writer_schema):  # in writer order: the last one wins
        c = column_of(name, columns)
        if c is None:
            continue
        if w in got:
            v = got[w]
        elif presence:
            v = None
        else:
            v = DEFAULT.get(ptype, 0)
        kt = columns[c][1]
        if v is None:
            row[c] = None
        elif kt == "STRING":
            row[c] = v if isinstance(v, str) else str(v)
        elif kt == "DOUBLE":
            row[c] = np.float64(v)
        else:
            row[c] = int(v)
    return row
