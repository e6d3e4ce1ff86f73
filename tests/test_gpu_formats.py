"""The format layer's options and paths beyond the comma and the BIGINT key: khip_serde_decode and
khip_sink_encode / khip_sink_key against their CPU restatements (tests/serde_ref.py, tests/sink_ref.py),
bit for bit, on the seeded inputs of tests/format_cases.py.

Decoder: DELIMITED under eight delimiters (three of them characters of printed numbers), every key
path (INT / BIGINT / STRING keys with nulls and wrong lengths, no key format), KAFKA values of each
type, the deferred-double pass (k_serde_fix: the fix list's growth and second decode, two deferred
fields in a record, a deferred field in a record that fails, a deferred field nobody reads), a handle
reused with shrinking batches.  Sink: DELIMITED values and keys under each delimiter, DOUBLE GROUP BY
columns in khip_sink_key, INT columns at their extremes, and the sink's bytes fed back into the decoder."""
import json
import os
import random
import struct

import numpy as np
import pytest

import format_cases as fc
import serde_ref
import sink_ref
from ksql_amd import abi

pytestmark = pytest.mark.gpu

DELIM_CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                          "delimited_delimiters.json")))["cases"]


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


def _out_types(fields):
    out = {c: t for _, t, c in fields if c >= 0}
    return [out[c] for c in range(len(out))]


def _serde(prod, fmt, fields, key="INT64", delim=","):
    if key.startswith("NONE"):
        return abi.SerdeHandle(prod, fmt, fields, key_format="NONE", delimiter=delim)
    return abi.SerdeHandle(prod, fmt, fields, key_type=key, delimiter=delim)


def _pack(items):
    n = len(items)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([0 if x is None else len(x) for x in items])
    data = np.frombuffer(b"".join(b"" if x is None else x for x in items) + b"\0", np.uint8).copy()
    return offs, data, np.array([x is not None for x in items], bool)


def _decode_device(sd, keys, vals):
    """The batch as device tensors (khip_serde_decode's KHIP_MEM_DEVICE input)."""
    import torch
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    n = len(vals)
    voff, vb, vv = _pack(vals)
    koff, kb, kv = _pack(keys) if keys is not None else (None, None, None)
    return sd.decode_device(dev(np.arange(n, dtype=np.int64)), dev(koff), dev(kb), dev(voff), dev(vb),
                            key_valid=None if kv is None else dev(abi.bitmap(kv)), value_valid=dev(abi.bitmap(vv)))


# ------------------------------------------------------------------ B.1 / B.2 / B.3 / B.6: the randomized cases

@pytest.mark.parametrize("case", fc.DECODE_CASES, ids=[c["id"] for c in fc.DECODE_CASES])
def test_decode_random_cases(prod, case):
    """Each seeded case (delimiters over the wide and the narrow schema; INT / BIGINT / STRING keys and
    no key format over DELIMITED, JSON and KAFKA values), batches of 1, 63, 64, 65, 257 and 3000 records
    on one handle; the 257-record batch goes in as a device batch.  A record whose key or value fails
    has neither key_valid nor row_valid, whatever the key type; STRING keys come back byte for byte."""
    refs = fc.case_reference(case)
    fc.check_shares(refs, case["fields"])  # from the reference alone, before the device is asked
    sd = _serde(prod, case["fmt"], case["fields"], case["key"], case["delim"])
    key_type = None if case["key"].startswith("NONE") else case["key"]
    for (keys, vals), (exp, experr) in zip(fc.case_batches(case), refs):
        n = len(vals)
        if case["key"] == "NONE-nokeys":
            keys = None
        if n == 257:
            d, nerr = _decode_device(sd, keys, vals)
        else:
            d, nerr = sd.decode(np.arange(n, dtype=np.int64), keys, vals)
        assert nerr == experr, (n, nerr, experr)
        got = sd.columns(d, _out_types(case["fields"]))
        fc.check_decoded(got, exp, case["fields"], key_type)
        if key_type is None:
            assert not got["key"].any()  # no key format: key 0 for every record
    sd.close()


@pytest.mark.parametrize("case", DELIM_CASES, ids=[c["name"][:60] for c in DELIM_CASES])
def test_decode_reference_delimiter_cases(prod, case):
    """The reference's own VALUE_DELIMITER cases ('-', '|', SPACE, TAB): its input records through the
    device, the numbers it expects out; the all-numeric case ("0-1") goes on through the sink with the
    output delimiter and gives the reference's expected output text."""
    fields = [(n, t, i) for i, (n, t) in enumerate(case["columns"])]
    vals = [v.encode() for v in case["inputs"]]
    keys = [struct.pack(">q", i) for i in range(len(vals))]
    sd = _serde(prod, "DELIMITED", fields, delim=case["delimiter_in"])
    d, nerr = sd.decode(np.arange(len(vals), dtype=np.int64), keys, vals)
    exp, experr = serde_ref.decode("DELIMITED", fields, "INT64", keys, vals, case["delimiter_in"])
    assert nerr == experr == 0
    got = sd.columns(d, [t for _, t in case["columns"]])
    fc.check_decoded(got, exp, fields)
    numeric = [(c, n, t) for c, (n, t) in enumerate(case["columns"]) if t != "STRING"]
    for i, text in enumerate(case["outputs"]):  # the reference's expected rows (a SELECT of every column)
        parts = text.split(case["delimiter_out"])
        for c, name, t in numeric:
            assert int(got["cols"][c][i]) == int(parts[c]), (i, name)
    sd.close()
    if len(numeric) == len(fields):  # the all-numeric case: the decoded columns through the sink
        s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], "DELIMITED", [(n, t, c) for c, n, t in numeric],
                           delimiter=case["delimiter_out"])
        n = len(vals)
        kb, vb = s.encode({"n": n, "key": np.arange(n, dtype=np.int64), "ws": np.zeros(n, np.int64),
                           "we": np.zeros(n, np.int64), "values": [got["cols"][c] for c, _, _ in numeric],
                           "nulls": [np.zeros(n, bool)] * len(numeric)})
        assert vb == [o.encode() for o in case["outputs"]]
        s.close()


def _kafka_case(prod, t, vals):
    fields = [("V", t, 0)]
    keys = [struct.pack(">q", i) for i in range(len(vals))]
    sd = _serde(prod, "KAFKA", fields)
    d, nerr = sd.decode(np.arange(len(vals), dtype=np.int64), keys, vals)
    exp, experr = serde_ref.decode("KAFKA", fields, "INT64", keys, vals)
    assert nerr == experr
    got = sd.columns(d, [t])
    fc.check_decoded(got, exp, fields)
    sd.close()
    return got, nerr


def test_kafka_int32_values(prod):
    good = [-(1 << 31), (1 << 31) - 1, -1, 0, 1, 0x01020304]
    vals = [struct.pack(">i", v) for v in good] + [b"", b"\x01\x02\x03", b"\x01" * 5, b"\x01" * 8, None]
    vals = vals * 7  # 77 records: more than a wave
    got, nerr = _kafka_case(prod, "INT32", vals)
    assert nerr == 4 * 7
    assert [int(x) for x in got["cols"][0][:6]] == good


def test_kafka_int64_values(prod):
    good = [-(1 << 63), (1 << 63) - 1, -1, 0, 0x0102030405060708]
    vals = [struct.pack(">q", v) for v in good] + [b"", b"\x01" * 4, b"\x01" * 7, b"\x01" * 9, None]
    vals = vals * 7
    got, nerr = _kafka_case(prod, "INT64", vals)
    assert nerr == 4 * 7
    assert [int(x) for x in got["cols"][0][:5]] == good


def test_kafka_double_values(prod):
    """The eight bytes big-endian are the double's bits, whatever they are: a signalling NaN keeps its
    payload (compared as bits here, beyond check_decoded's "NaN as NaN")."""
    patterns = [0x7FF0000000000001, 0xFFF4000000000123, 0x7FF8000000000000, 0x8000000000000000, 0x0000000000000001,
                0x000FFFFFFFFFFFFF, 0x8000000000000001, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000, 0x3FF8000000000000,
                0x0102030405060708]
    vals = [struct.pack(">Q", b) for b in patterns] + [b"\x01" * 4, b"\x01" * 7, b"\x01" * 9, None]
    vals = vals * 5
    got, nerr = _kafka_case(prod, "DOUBLE", vals)
    assert nerr == 3 * 5
    assert [int(x) for x in got["cols"][0].view(np.uint64)[:len(patterns)]] == patterns


def test_kafka_string_values(prod):
    """STRING columns carry validity only: any bytes, the empty string included, are non-NULL; a null
    value is a NULL row."""
    vals = [b"abc", b"", None, b"\xff\xfe", b"x" * 300] * 15
    got, nerr = _kafka_case(prod, "STRING", vals)
    assert nerr == 0
    assert list(got["valid"][0][:5]) == [True, True, False, True, True]
    assert list(got["row_valid"][:5]) == [True, True, False, True, True]


def test_failed_value_clears_the_key_for_every_key_type(prod):
    """A record whose value fails comes back with neither key_valid nor row_valid, whatever its key."""
    vals = [b"1,2", b"x,2", b"1", b"3,4"] * 20
    fields = [("A", "INT32", 0), ("B", "INT64", 1)]
    for key_type, key in (("INT32", struct.pack(">i", 7)), ("INT64", struct.pack(">q", 7)), ("STRING", b"seven")):
        sd = _serde(prod, "DELIMITED", fields, key=key_type)
        keys = [key] * len(vals)
        d, nerr = sd.decode(np.arange(len(vals), dtype=np.int64), keys, vals)
        exp, experr = serde_ref.decode("DELIMITED", fields, key_type, keys, vals)
        assert nerr == experr == 40
        got = sd.columns(d, ["INT32", "INT64"])
        fc.check_decoded(got, exp, fields, key_type)
        assert list(got["key_valid"][:4]) == list(got["row_valid"][:4]) == [True, False, False, True]
        sd.close()


# ------------------------------------------------------------------ B.4: deferred doubles

def _decode_check(sd, fmt, keys, vals, fields=fc.DEFER_FIELDS, out=fc.DEFER_OUT, device=False):
    n = len(vals)
    if device:
        d, nerr = _decode_device(sd, keys, vals)
    else:
        d, nerr = sd.decode(np.arange(n, dtype=np.int64), keys, vals)
    exp, experr = serde_ref.decode(fmt, fields, "INT64", keys, vals)
    assert nerr == experr, (n, nerr, experr)
    fc.check_decoded(sd.columns(d, out), exp, fields)
    return experr


@pytest.mark.parametrize("fmt", ["DELIMITED", "JSON"])
def test_deferred_doubles_grow_the_fix_list(prod, fmt):
    """1500 records with both DOUBLE columns next to a halfway point: 2700 deferred fields against a fix
    list of 1024 entries, so the decoder grows the list and decodes the batch again (the precondition,
    at least 1025 deferring fields, is tests/test_numparse.py's).  Then 10 records on the same handle,
    then 5000 records of which every 97th defers."""
    sd = _serde(prod, fmt, fc.DEFER_FIELDS)
    assert _decode_check(sd, fmt, *fc.grow_batch(fmt)) == 0
    assert _decode_check(sd, fmt, *fc.mixed_batch(fmt, 10)) == 2
    assert _decode_check(sd, fmt, *fc.sparse_batch(fmt)) == 0
    sd.close()


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("fmt", ["DELIMITED", "JSON"])
def test_deferred_doubles_mixed_records(prod, fmt, n):
    """In turn: both DOUBLE fields deferred; a deferred field and then an arity error (JSON: a boolean
    for the BIGINT column) in the same record; a halfway text in the column nobody reads, which neither
    defers nor fails; one deferred field; none.  n_errors counts records, the failed fifth."""
    sd = _serde(prod, fmt, fc.DEFER_FIELDS)
    keys, vals = fc.mixed_batch(fmt, n)
    assert _decode_check(sd, fmt, keys, vals) == (n + 3) // 5
    assert _decode_check(sd, fmt, keys, vals, device=True) == (n + 3) // 5
    sd.close()


# ------------------------------------------------------------------ B.5: a handle reused with shrinking batches

@pytest.mark.parametrize("fmt", ["DELIMITED", "JSON", "KAFKA"])
def test_shrinking_batches_on_one_handle(prod, fmt):
    """4000, then 65, then 1, then 0 records on one handle: each result in full (the validity bitmaps
    are written per wave; nothing of the larger batch may show through), and n = 0 gives no rows and
    no errors."""
    fields = [("V", "INT64", 0)] if fmt == "KAFKA" else fc.FIELDS
    rng = random.Random({"DELIMITED": 71, "JSON": 72, "KAFKA": 73}[fmt])
    batches = [fc.records(rng, fmt, fields, n, "INT64", ";") for n in (4000, 65, 1, 0)]
    refs = [serde_ref.decode(fmt, fields, "INT64", keys, vals, ";") for keys, vals in batches]
    fc.check_shares(refs, fields)
    assert refs[-1] == ([], 0)
    sd = _serde(prod, fmt, fields, delim=";")
    for (keys, vals), (exp, experr) in zip(batches, refs):
        n = len(vals)
        d, nerr = sd.decode(np.arange(n, dtype=np.int64), keys, vals)
        assert nerr == experr
        assert d.struct.n_rows == n
        fc.check_decoded(sd.columns(d, _out_types(fields)), exp, fields)
    sd.close()


# ------------------------------------------------------------------ C: the sink

def _rows(n, keys=None, values=(), nulls=()):
    return {"n": n, "key": keys if keys is not None else np.arange(n, dtype=np.int64), "ws": np.zeros(n, np.int64),
            "we": np.zeros(n, np.int64), "values": list(values), "nulls": list(nulls)}


SINK_DOUBLES = [1.0e10, -1.0e10, 1.5, -2.25, 100.0, 0.001, 1.0e-5, 1.0e7, -0.0, 0.0, 5e-324, 1e22, 1e23, float("nan"),
                float("inf"), float("-inf"), 1.7976931348623157e308, 123456.789]


def _random_bits(rng, n):
    """Doubles of random bit patterns, either sign (NaNs of any payload among them)."""
    b = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
    return b.view(np.float64)


def _sink_columns(seed, n):
    """INT / BIGINT / DOUBLE columns with NULLs: the special values first, then random ones."""
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    i64 = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    f64 = np.where(rng.random(n) < 0.5, rng.uniform(-1e6, 1e6, n), _random_bits(rng, n))
    k = min(n, len(SINK_DOUBLES))
    f64[:k] = SINK_DOUBLES[:k]
    i32[:min(n, 5)] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0, 100][:min(n, 5)]
    i64[:min(n, 5)] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0, 100][:min(n, 5)]
    nulls = [rng.random(n) < 0.15 for _ in range(3)]
    for m in nulls:
        m[:k:3] = False
    return [i32, i64, f64], nulls


def _py(cols, nulls, i):
    return [None if nulls[c][i] else (float(cols[c][i]) if cols[c].dtype == np.float64 else int(cols[c][i]))
            for c in range(len(cols))]


VCOLS = [("I", "INT32", 0), ("L", "INT64", 1), ("D", "DOUBLE", 2)]
VTYPES = [(n, t) for n, t, _ in VCOLS]
KEY_TEXTS = ["plain", "", " lead", "trail ", 'q"uote', "#hash", "a|b", "a;b", "a$b", "a\tb", "a b", "a-b", "a.b",
             "aEb", "a0b", "a,b", "-5", "1.0E10", "é"]


@pytest.mark.parametrize("dev_out", [False, True])
@pytest.mark.parametrize("delim", fc.SINK_DELIMS, ids=[fc.DELIM_IDS[d] for d in fc.SINK_DELIMS])
def test_sink_delimited_under_each_delimiter(prod, delim, dev_out):
    """DELIMITED values (INT, BIGINT, DOUBLE with NaN, the infinities, 1.0E10 and NULLs) and a DELIMITED
    STRING key whose text holds the delimiter, a quote or outer spaces: a field is quoted when it holds
    the delimiter, so "-5" under '-', every finite double under '.', "1.0E10" under 'E' and '0'."""
    n = 300
    cols, nulls = _sink_columns(ord(delim), n)
    keys = [KEY_TEXTS[i % len(KEY_TEXTS)] + ("" if i < len(KEY_TEXTS) else str(i)) for i in range(n)]
    tomb = (np.arange(n) % 11 == 10).astype(np.uint8)
    s = abi.SinkHandle(prod, "DELIMITED", [("K", "STRING")], "DELIMITED", VCOLS, delimiter=delim)
    kb, vb = s.encode(_rows(n, keys=keys, values=cols, nulls=nulls), tombstone=tomb, device_out=dev_out, align=3)
    for i in range(n):
        exp_k = sink_ref.encode_key("DELIMITED", [("K", "STRING")], [keys[i]], delim)
        assert kb[i] == exp_k, (i, kb[i], exp_k)
        exp_v = sink_ref.encode_value("DELIMITED", VTYPES, _py(cols, nulls, i), bool(tomb[i]), delim)
        assert vb[i] == exp_v, (i, vb[i], exp_v)
    s.close()


@pytest.mark.parametrize("delim", fc.SINK_DELIMS, ids=[fc.DELIM_IDS[d] for d in fc.SINK_DELIMS])
def test_sink_composite_delimited_keys_under_each_delimiter(prod, delim):
    """khip_sink_key, DELIMITED: two STRING columns around INT, BIGINT and DOUBLE ones."""
    n = 257
    cols, nulls = _sink_columns(1000 + ord(delim), n)
    s1 = [KEY_TEXTS[i % len(KEY_TEXTS)] for i in range(n)]
    s2 = [None if i % 29 == 28 else KEY_TEXTS[(i * 7 + 3) % len(KEY_TEXTS)] for i in range(n)]
    kc = [("S1", "STRING"), ("I", "INT32"), ("L", "INT64"), ("D", "DOUBLE"), ("S2", "STRING")]
    s = abi.SinkHandle(prod, "DELIMITED", kc, "JSON", [], delimiter=delim)
    hb = abi.HostBatch(np.arange(n, dtype=np.int64), keys=np.zeros(n, np.int64))
    got = s.key_bytes(s.key(hb, [s1] + [(cols[c], ~nulls[c]) for c in range(3)] + [s2]))
    for i in range(n):
        vals = [s1[i]] + _py(cols, nulls, i) + [s2[i]]
        exp = None if any(v is None for v in vals) else sink_ref.encode_key("DELIMITED", kc, vals, delim)
        assert got[i] == exp, (i, got[i], exp)
    s.close()


def _device_keys(keyed, n):
    """The keys of a keyed device batch: list of bytes / None."""
    b = keyed.struct
    offs = np.zeros(n + 1, np.int64)
    abi._hip_copy(offs, b.key_offsets, (n + 1) * 8)
    tot = int(offs[n])
    data = np.zeros(max(tot, 1), np.uint8)
    abi._hip_copy(data, b.key_bytes, tot)
    vbits = np.zeros((n + 7) // 8, np.uint8)
    abi._hip_copy(vbits, b.key_valid, len(vbits))
    valid = np.unpackbits(vbits, bitorder="little")[:n].astype(bool)
    return [bytes(data[offs[i]:offs[i + 1]]) if valid[i] else None for i in range(n)]


DOUBLE_KEYS = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 5e-324, 1e22, 1e23, 1.0, -1.5, 1e7, 0.001, 9.999e-4]
KEY_LAYOUTS = [("KAFKA", [("D", "DOUBLE")]), ("JSON", [("D", "DOUBLE")]), ("JSON", [("D", "DOUBLE"), ("I", "INT32")]),
               ("DELIMITED", [("I", "INT32"), ("D", "DOUBLE")])]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kfmt,kcols", KEY_LAYOUTS, ids=["KAFKA", "JSON", "JSON-composite", "DELIMITED-composite"])
def test_sink_key_double_columns(prod, kfmt, kcols, device):
    """DOUBLE GROUP BY columns: 8 bytes big-endian (KAFKA), Double.toString with the non-finite values
    quoted (JSON, alone and inside an object), the CSV field (DELIMITED); a NULL makes a null key."""
    import torch
    n = 257
    rng = np.random.default_rng(17)
    d = _random_bits(rng, n)
    d[:len(DOUBLE_KEYS)] = DOUBLE_KEYS
    dv = rng.random(n) > 0.1
    dv[:len(DOUBLE_KEYS)] = True
    dv[len(DOUBLE_KEYS)] = False
    i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    s = abi.SinkHandle(prod, kfmt, kcols, "JSON", [])
    ts = np.arange(n, dtype=np.int64)
    if device:
        keep = {k: torch.from_numpy(v).cuda() for k, v in dict(d=d, dv=abi.bitmap(dv), i=i32, ts=ts).items()}
        batch = abi.DeviceBatch(keep["ts"])
        by_type = {"DOUBLE": {"data": keep["d"].data_ptr(), "valid": keep["dv"].data_ptr()},
                   "INT32": {"data": keep["i"].data_ptr()}}
        keyed = s.key(batch, [by_type[t] for _, t in kcols])
        torch.cuda.synchronize()
        got = _device_keys(keyed, n)
    else:
        by_type = {"DOUBLE": (d, dv), "INT32": i32}
        got = s.key_bytes(s.key(abi.HostBatch(ts, keys=np.zeros(n, np.int64)), [by_type[t] for _, t in kcols]))
    for i in range(n):
        vals = [float(d[i]) if t == "DOUBLE" else int(i32[i]) for _, t in kcols]
        exp = sink_ref.encode_key(kfmt, kcols, vals) if dv[i] else None
        assert got[i] == exp, (i, d[i], got[i], exp)
    s.close()


@pytest.mark.parametrize("vfmt", ["KAFKA", "JSON", "DELIMITED"])
def test_sink_int32_value_extremes(prod, vfmt):
    v = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0, 1] * 13, np.int32)
    n = len(v)
    nulls = np.arange(n) % 7 == 6
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], vfmt, [("V", "INT32", 0)])
    for dev_out in (False, True):
        kb, vb = s.encode(_rows(n, values=[v], nulls=[nulls]), device_out=dev_out)
        for i in range(n):
            exp = sink_ref.encode_value(vfmt, [("V", "INT32")], [None if nulls[i] else int(v[i])])
            assert vb[i] == exp, (i, vb[i], exp)
    assert sink_ref.encode_value("KAFKA", [("V", "INT32")], [-(1 << 31)]) == b"\x80\0\0\0"
    s.close()


# ------------------------------------------------------------------ C.4: sink -> decoder

ROUND_TRIPS = [("KAFKA", ",", [c]) for c in VCOLS] + [("JSON", ",", VCOLS)] + \
    [("DELIMITED", d, VCOLS) for d in [","] + fc.SINK_DELIMS] + [("DELIMITED", ";", VCOLS[2:]), ("DELIMITED", "-", VCOLS[:1])]


@pytest.mark.parametrize("vfmt,delim,vcols", ROUND_TRIPS,
                         ids=["%s-%s-%s" % (f, fc.DELIM_IDS[d], "".join(c[0] for c in v)) for f, d, v in ROUND_TRIPS])
def test_round_trip_sink_to_decoder(prod, vfmt, delim, vcols):
    """Random typed columns with NULLs and tombstones through khip_sink_encode (bytes equal to sink_ref),
    those bytes through khip_serde_decode (result equal to serde_ref on them), and where the reference
    says the record decodes, the columns that went in: integers exact, doubles by bits, NaN as NaN.
    Which records do not decode (a tombstone; a single NULL DELIMITED column, an empty record) is the
    reference's verdict."""
    n = 1000
    all_cols, all_nulls = _sink_columns(7 + ord(delim) + len(vcols), n)
    src = [c[2] for c in vcols]
    names = [(c[0], c[1]) for c in vcols]
    cols, nulls = [all_cols[j] for j in src], [all_nulls[j] for j in src]
    tomb = (np.arange(n) % 13 == 12).astype(np.uint8)
    s = abi.SinkHandle(prod, "KAFKA", [("K", "INT64")], vfmt, [(c[0], c[1], j) for j, c in enumerate(vcols)],
                       delimiter=delim)
    kb, vb = s.encode(_rows(n, values=cols, nulls=nulls), tombstone=tomb)
    s.close()
    for i in range(n):
        exp = sink_ref.encode_value(vfmt, names, _py(cols, nulls, i), bool(tomb[i]), delim)
        assert vb[i] == exp, (i, vb[i], exp)
        assert kb[i] == struct.pack(">q", i)
    fields = [(c[0], c[1], j) for j, c in enumerate(vcols)]
    sd = _serde(prod, vfmt, fields, delim=delim)
    d, nerr = sd.decode(np.arange(n, dtype=np.int64), kb, vb)
    exp, experr = serde_ref.decode(vfmt, fields, "INT64", kb, vb, delim)
    assert nerr == experr
    got = sd.columns(d, [c[1] for c in vcols])
    fc.check_decoded(got, exp, fields)
    decodable = 0
    for i, (kv, key, rv, row) in enumerate(exp):
        if not rv or row is None:
            continue
        decodable += 1
        assert int(got["key"][i]) == i
        for j, (name, t, _) in enumerate(fields):
            if nulls[j][i]:
                assert not got["valid"][j][i], (i, name)
            elif t == "DOUBLE":
                assert got["valid"][j][i] and fc.same_double(float(got["cols"][j][i]), float(cols[j][i])), (i, name)
            else:
                assert got["valid"][j][i] and int(got["cols"][j][i]) == int(cols[j][i]), (i, name)
    assert decodable >= n // 2
    sd.close()
