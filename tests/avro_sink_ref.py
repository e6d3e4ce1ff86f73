"""CPU restatement of an AVRO sink value (TEST INFRASTRUCTURE, like sink_ref.py and
sink_array_ref.py: the checker of khip_sink_encode's KHIP_FMT_AVRO value format), built on
avro_ref's zig-zag and varint.

The reference serializes a sink row through KsqlAvroSerdeFactory.createConnectSerializer
(avro/KsqlAvroSerdeFactory.java:104-128): AvroDataTranslator over the schema of
AvroSchemas.getAvroCompatibleConnectSchema — every field optional, an array keeping its optional
element schema (avro/AvroSchemas.java:135-142) — then Confluent's AvroConverter /
KafkaAvroSerializer.  The record: byte 0, the schema id as 4 bytes big-endian, then per column the
union ["null", T]: the branch (0x00 = NULL, 0x02 = present) and the value — a zig-zag varint for
INT32 / INT64, the 8 raw IEEE bytes little-endian for DOUBLE, and for an ARRAY (never NULL itself)
one block: the long n, n items (each a branch and its value) and the end byte 0x00; the empty list
is the end byte alone.

A column is (name, type) for a scalar and (name, type, L) for an ARRAY of L slots; an ARRAY's value
is a Python list (None = a NULL element), a scalar's a number or None.  A DOUBLE given as a numpy
float64 keeps its bits (NaN payloads included).
"""
import struct

import numpy as np

from avro_ref import _varint, _zz

BITS = {"INT32": 32, "INT64": 64}


def _double(v):
    if isinstance(v, np.floating):
        return struct.pack("<Q", int(np.array(v, np.float64).view(np.uint64)))
    return struct.pack("<d", v)


def optional(typ, v):
    """The union ["null", T] of one value."""
    if v is None:
        return b"\x00"
    return b"\x02" + (_double(v) if typ == "DOUBLE" else _varint(_zz(int(v), BITS[typ])))


def array(typ, vals):
    """An optional ARRAY column holding the list vals."""
    if not vals:
        return b"\x02\x00"
    return b"\x02" + _varint(_zz(len(vals), 64)) + b"".join(optional(typ, v) for v in vals) + b"\x00"


def encode_value(cols, row, schema_id, tombstone=False):
    """The AVRO record value of a row; None for a tombstone."""
    if tombstone:
        return None
    out = b"\x00" + struct.pack(">i", schema_id)
    for c, v in zip(cols, row):
        out += array(c[1], v) if len(c) > 2 else optional(c[1], v)
    return out
