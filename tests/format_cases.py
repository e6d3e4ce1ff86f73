"""Seeded inputs of the format-layer tests (khip_serde_decode, khip_sink_encode / khip_sink_key),
shared by the CPU tests of the references and the GPU tests so both see the same bytes.

The random record generators decide per record, not per field, whether a record is malformed, so
most rows reach the column comparison; check_shares() is the condition the tests assert from the
reference's result before they look at the device's.  No GPU, no library: plain Python."""
import decimal
import functools
import json
import math
import random
import struct

FIELDS = [("ID", "INT64", -1), ("V32", "INT32", 0), ("V64", "INT64", 1), ("D", "DOUBLE", 2), ("NAME", "STRING", 3),
          ("SKIPPED", "INT32", -1)]
NARROW = FIELDS[1:5]  # four fields: the decode kernel's register-array variant
OUT_TYPES = ["INT32", "INT64", "DOUBLE", "STRING"]

# '-', '.', 'E' (and '0' on the sink side) occur inside printed numbers, which must then be quoted
DELIMS = ["|", ";", "$", "\t", " ", "-", ".", "E"]
SINK_DELIMS = DELIMS + ["0"]
DELIM_IDS = {"|": "pipe", ";": "semicolon", "$": "dollar", "\t": "TAB", " ": "SPACE", "-": "minus", ".": "dot",
             "E": "E", "0": "zero", ",": "comma"}
# wave (64) and block (256) tails, and one batch of several blocks
SIZES = (1, 63, 64, 65, 257, 3000)


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def same_double(a, b):
    return bits_of(a) == bits_of(b) or (math.isnan(a) and math.isnan(b))


# ------------------------------------------------------------------ halfway decimals

_CTX = decimal.Context(prec=1300, traps=[decimal.Inexact])  # every operation below is exact or raises


def halfway_texts(x):
    """For a finite double x: the exact decimal expansion of the midpoint between |x| and the next
    double away from zero (2^1024 past the largest finite one), with x's sign; the same text with its
    last digit one up; and one down.  With more than 19 significant digits and a non-zero digit past
    the 19th, the 19-digit prefix and its successor lie either side of the midpoint and round to
    different doubles: Double.parseDouble needs the big-integer step (tests/test_numparse.py names the
    two texts of 1e23 for which this does not hold)."""
    ax = abs(x)
    nxt = from_bits(bits_of(ax) + 1)
    hi = _CTX.power(decimal.Decimal(2), 1024) if math.isinf(nxt) else decimal.Decimal(nxt)
    mid = _CTX.divide(_CTX.add(decimal.Decimal(ax), hi), decimal.Decimal(2))
    text = format(mid, "f")
    point = text.find(".")
    digits = text.replace(".", "")

    def moved(step):
        if point < 0:  # an integer: no leading zero (not a JSON number otherwise)
            return str(int(digits) + step)
        d = str(int(digits) + step).zfill(len(digits))  # a fraction ends in 5: no carry past the point
        return d[:point] + "." + d[point:]
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    return [sign + text, sign + moved(1), sign + moved(-1)]


HALFWAY_FIXED = [1.0, 0.1, 1e23, 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324, 0.0]


@functools.lru_cache(maxsize=None)
def halfway_pool(seed=41, n_random=150):
    """[(text, float(text))]: the fixed doubles, random bit patterns over the whole finite range, and
    the negative copies of all of them; three texts per double."""
    rng = random.Random(seed)
    xs = list(HALFWAY_FIXED)
    while len(xs) < len(HALFWAY_FIXED) + n_random:
        x = from_bits(rng.randrange(0, 0x7FF0000000000000))
        if all(tail_nonzero(t) for t in halfway_texts(x)):  # (not so for a double from 2^60 to 2^63: 19 digits)
            xs.append(x)
    out = []
    for x in xs + [-x for x in xs]:
        out += [(t, float(t)) for t in halfway_texts(x)]
    return out


def significant_digits(text):
    return len(text.lstrip("-").replace(".", "").lstrip("0"))


def tail_nonzero(text):
    """More than 19 significant digits, and a non-zero digit among those past the 19th: the parser cannot
    finish from the first 19 alone.  Of the pool's texts only the midpoint above 1e23 fails this: it is
    the decimal 1e23 itself, twenty-three zeros after a one."""
    return text.lstrip("-").replace(".", "").lstrip("0")[19:].strip("0") != ""


# ------------------------------------------------------------------ deferred-double batches

DEFER_FIELDS = [("A", "DOUBLE", 0), ("S", "DOUBLE", -1), ("B", "DOUBLE", 1), ("N", "INT64", 2)]
DEFER_OUT = ["DOUBLE", "DOUBLE", "INT64"]


def _plain_double(rng):
    return repr(rng.uniform(-1e6, 1e6))


def defer_record(rng, fmt, kind):
    """One record of DEFER_FIELDS.  kind: "both" (A and B halfway texts), "one" (A), "unread" (only
    the unread column S holds one: nothing defers, nothing fails), "fail" (A halfway, then the record
    fails: arity / a boolean for N), "plain" (no halfway text)."""
    pool = halfway_pool()
    hw = lambda: pool[rng.randrange(len(pool))][0]
    a = hw() if kind in ("both", "one", "fail") else _plain_double(rng)
    s = hw() if kind == "unread" else _plain_double(rng)
    b = hw() if kind == "both" else _plain_double(rng)
    n = str(rng.randrange(-10 ** 9, 10 ** 9))
    if fmt == "DELIMITED":
        parts = [a, s, b, n]
        parts = ['"%s"' % p if rng.random() < 0.2 else p for p in parts]
        if kind == "fail":
            parts = parts + ["extra"] if rng.random() < 0.5 else parts[:3]
        return ",".join(parts).encode()
    tok = lambda t: t if rng.random() < 0.5 else json.dumps(t)  # a number token, or the text as a string
    obj = ['"A": ' + tok(a), '"S": ' + tok(s), '"B": ' + tok(b), '"N": ' + ("true" if kind == "fail" else n)]
    return ("{" + ", ".join(obj) + "}").encode()


def defer_batch(seed, fmt, n, kinds):
    """n records; kinds: a function record index -> kind.  Returns (keys, values)."""
    rng = random.Random(seed)
    vals = [defer_record(rng, fmt, kinds(i)) for i in range(n)]
    keys = [struct.pack(">q", i) for i in range(n)]
    return keys, vals


GROW_N = 1500  # records of the batch that overflows the decoder's first 1024-entry fix list


def grow_batch(fmt):
    """About 1500 records, A and B both halfway texts in nine of ten: more than 1024 deferred fields."""
    return defer_batch(51, fmt, GROW_N, lambda i: "plain" if i % 10 == 9 else "both")


def grow_batch_deferring_texts(fmt):
    """The texts of the read DOUBLE fields (A, B) of grow_batch's records, as the kernel sees them."""
    _, vals = grow_batch(fmt)
    out = []
    for v in vals:
        if fmt == "DELIMITED":
            parts = [p.strip('"') for p in v.decode().split(",")]
            out += [parts[0], parts[2]]
        else:
            obj = json.loads(v.decode(), parse_float=str, parse_int=str)
            out += [obj["A"], obj["B"]]
    return out


def sparse_batch(fmt, n=5000):
    return defer_batch(52, fmt, n, lambda i: "one" if i % 97 == 0 else "plain")


def mixed_batch(fmt, n):
    kinds = ["both", "fail", "unread", "one", "plain"]
    return defer_batch(53 + n, fmt, n, lambda i: kinds[i % len(kinds)])


# ------------------------------------------------------------------ keys

def random_key(rng, key_type):
    """A record key: mostly well-formed, a few nulls and wrong lengths (8 bytes for an INT key, 4
    for a BIGINT key, 0 bytes for either: errors); STRING keys of any bytes, the empty key included."""
    r = rng.random()
    if r < 0.05:
        return None
    if key_type == "STRING":
        if r < 0.12:
            return b""
        return bytes(rng.randrange(256) for _ in range(rng.randrange(1, 24)))
    good = 4 if key_type == "INT32" else 8
    if r < 0.07:
        return b""
    if r < 0.09:
        return bytes(rng.randrange(256) for _ in range(12 - good))
    if r < 0.10:
        return bytes(rng.randrange(256) for _ in range(rng.choice([1, 3, 5, 7, 9])))
    if rng.random() < 0.1:
        v = rng.choice([-(1 << (8 * good - 1)), (1 << (8 * good - 1)) - 1, -1, 0])
    else:
        v = rng.randrange(-(1 << (8 * good - 1)), 1 << (8 * good - 1))
    return struct.pack(">i" if good == 4 else ">q", v)


# ------------------------------------------------------------------ DELIMITED records

NAMES = ["alice", "b,ob", 'q"uote', "x y", " lead", "trail ", "a|b;c$d", "1-2", "3.5E7", "tab\there", "é"]
GOOD_DOUBLES = ["NaN", "Infinity", "-Infinity", "1.0E10", "-2.5e-310", "1e400", "7d", " 1.5 ", "-0.0", ".5", "5."]
BAD_NUMBERS = {"INT32": [str(1 << 31), "-0x1", "+ 5", " 3", "1.0", "x", "99999999999999999999", "1e3"],
               "INT64": [str(1 << 63), " 3", "1.0", "x", "99999999999999999999", "--1"],
               "DOUBLE": ["abc", "1..2", "1e", "0x10", "Nan", "- 1", "1,5"]}


def good_number(rng, t):
    r = rng.random()
    if t == "DOUBLE":
        if r < 0.4:
            return repr(rng.uniform(-1e6, 1e6))
        if r < 0.55:  # more than 19 significant digits
            return str(rng.randrange(1, 10)) + "".join(str(rng.randrange(10)) for _ in range(rng.randrange(19, 30))) + \
                "e" + str(rng.randrange(-320, 300))
        if r < 0.75:
            return rng.choice(GOOD_DOUBLES)
        return "%d.%d" % (rng.randrange(-10 ** 6, 10 ** 6), rng.randrange(1000))
    bits = 32 if t == "INT32" else 64
    if r < 0.15:
        return rng.choice([str(-(1 << (bits - 1))), str((1 << (bits - 1)) - 1), "-1", "0", "-0", "+5", "007"])
    return str(rng.randrange(-(1 << (bits - 1)), 1 << (bits - 1)))


def csv_in(text, delim, rng, force=False):
    """An input field: quoted (with "" escapes) when it must be, or now and then when it need not."""
    must = force or any(x in text for x in (delim, '"', "\n", "\r"))
    return '"%s"' % text.replace('"', '""') if must or rng.random() < 0.1 else text


def delimited_record(rng, fields, delim, p_bad=0.12):
    """One DELIMITED value (bytes, or None for a null value).  A well-formed record has a NULL (empty
    field) in some columns, quoted fields holding the delimiter, quoted numbers, "" escapes, a ','
    inside an unquoted field when ',' is not the delimiter, and sometimes a line end (and ignored
    bytes after it).  With probability p_bad the whole record gets one defect."""
    if rng.random() < 0.04:
        return None
    parts = []
    for name, t, _ in fields:
        if rng.random() < 0.15:
            parts.append("")
        elif t == "STRING":
            parts.append(csv_in(rng.choice(NAMES), delim, rng))
        else:
            parts.append(csv_in(good_number(rng, t), delim, rng))
    if rng.random() < p_bad:
        k = rng.randrange(7)
        numeric = [i for i, (_, t, _) in enumerate(fields) if t != "STRING"]
        if k == 0:
            parts.append("extra")  # arity too long
        elif k == 1:
            parts = parts[:-1]  # arity too short (one field: the empty record)
        elif k == 2:
            i = rng.choice(numeric)
            parts[i] = csv_in(rng.choice(BAD_NUMBERS[fields[i][1]]), delim, rng)
        elif k == 3:
            parts[-1] = '"open'  # end of input inside quotes
        elif k == 4:
            parts[0] = '"a"b'  # a character after the closing quote
        elif k == 5:
            i = rng.choice(numeric)
            parts[i] = '"1""2"'  # an escaped quote inside a number
        else:
            return b""  # no fields in record
    line = delim.join(parts)
    r = rng.random()
    if r < 0.04:
        line += "\n"
    elif r < 0.08:
        line += "\r\n" + "ignored" + delim + "x"
    return line.encode()


# ------------------------------------------------------------------ JSON records

DECIMAL_TOKENS = ["3000000000.5", "-3000000000.5", "1e20", "9007199254740993.7", "-0.9", "4.2E1", "1e-5", "0.0",
                  "2147483648.0", "1E+19"]


def json_record(rng, fields, p_bad=0.12):
    if rng.random() < 0.04:
        return None
    obj = []
    for name, t, _ in fields:
        r = rng.random()
        if r < 0.08:
            continue  # missing: NULL
        key = name if rng.random() < 0.7 else name.lower()
        if r < 0.16:
            val = "null"
        elif t == "STRING":
            val = json.dumps(rng.choice(NAMES)) if rng.random() < 0.8 else rng.choice(["12", "true", "[1,2]"])
        else:
            k = rng.random()
            txt = good_number(rng, t)
            if k < 0.5:
                try:
                    json.loads(txt, parse_constant=lambda c: 1 / 0)
                    val = txt  # a JSON number token
                except (ValueError, ZeroDivisionError):
                    val = json.dumps(txt)
            elif k < 0.75:
                val = json.dumps(txt)  # the number as a string
            elif k < 0.9 and t != "DOUBLE":
                val = rng.choice(DECIMAL_TOKENS)  # BigDecimal into an integer column
            else:
                val = str(rng.randrange(-(1 << 70), 1 << 70))  # BigInteger token
        obj.append('"%s": %s' % (key, val))
    if rng.random() < 0.1 and obj:
        obj.append(obj[0])  # duplicate field: the last wins
    body = "{" + ", ".join(obj) + "}"
    if rng.random() < p_bad:
        k = rng.randrange(6)
        numeric = [(n, t) for n, t, _ in fields if t != "STRING"]
        name, t = rng.choice(numeric)
        if k == 0:
            body = body[:-1]  # truncated
        elif k == 1:
            body = body[:-1] + (", " if obj else "") + '"%s": true}' % name  # a boolean for a number
        elif k == 2:
            body = body[:-1] + (", " if obj else "") + '"%s": %s}' % (name, json.dumps(rng.choice(BAD_NUMBERS[t])))
        elif k == 3:
            body = body[:-1] + ",}" if obj else "[1]"  # trailing comma / not an object
        elif k == 4:
            body = body[:-1] + (", " if obj else "") + '"%s": {"a": [1]}}' % name  # an object for a number
        else:
            body = "x" + body
    if rng.random() < 0.05:
        body = "  " + body + "  trailing"
    return body.encode()


def kafka_record(rng, t, p_bad=0.12):
    """A KAFKA-format value of type t (INT32 / INT64 / DOUBLE): big-endian primitive bytes."""
    if rng.random() < 0.04:
        return None
    good = 4 if t == "INT32" else 8
    if rng.random() < p_bad:
        return bytes(rng.randrange(256) for _ in range(rng.choice([x for x in (0, 3, 4, 5, 7, 8, 9) if x != good])))
    return bytes(rng.randrange(256) for _ in range(good))


def records(rng, fmt, fields, n, key_type="INT64", delim=","):
    """(keys, values) of n random records; keys None-free lists of bytes / None."""
    keys, vals = [], []
    for _ in range(n):
        keys.append(random_key(rng, key_type) if key_type else b"")
        if fmt == "DELIMITED":
            vals.append(delimited_record(rng, fields, delim))
        elif fmt == "JSON":
            vals.append(json_record(rng, fields))
        else:
            vals.append(kafka_record(rng, fields[0][1]))
    return keys, vals


def check_shares(exps, fields):
    """The balance condition on a randomized case, from the reference's results alone (exps: the
    serde_ref.decode results of the case's batches, taken together): between 5 % and 25 % of the
    records fail, and every output column has NULL and non-NULL rows among the valid records."""
    rows = [r for exp, _ in exps for r in exp]
    failed = sum(nerr for _, nerr in exps)
    assert 0.05 * len(rows) <= failed <= 0.25 * len(rows), (failed, len(rows))
    for name, t, c in fields:
        if c < 0:
            continue
        # (a record with a key and a null value did not fail: every column of it is NULL; the one
        # field of a KAFKA value can be NULL in no other way)
        seen = {row is None or row[name] is None for kv, key, rv, row in rows if kv or rv}
        assert seen == {True, False}, (name, seen)


# ------------------------------------------------------------------ comparison with serde_ref

def key_list(got, n):
    """STRING keys of SerdeHandle.columns(): the records' key bytes."""
    o, b = got["key_offsets"], got["key_bytes"].tobytes()
    return [b[o[i]:o[i + 1]] for i in range(n)]


def check_decoded(got, exp, fields, key_type="INT64"):
    """SerdeHandle.columns() against serde_ref.decode's records, in full: key and row validity (a
    failed record has neither), the key's value or bytes, per column NULL and the value (integers
    exact, doubles by bits, NaN as NaN; STRING columns carry validity only)."""
    n = len(exp)
    assert len(got["key_valid"]) == len(got["row_valid"]) == n
    keys = key_list(got, n) if key_type == "STRING" else None
    for i, (kv, key, rv, row) in enumerate(exp):
        assert got["key_valid"][i] == kv, (i, kv)
        assert got["row_valid"][i] == rv, (i, rv)
        if kv and key_type == "STRING":
            assert keys[i] == key, (i, keys[i], key)
        elif kv and key_type is not None:
            assert int(got["key"][i]) == key, (i, got["key"][i], key)
        for name, t, c in fields:
            if c < 0:
                continue
            v = row[name] if rv and row is not None else None
            assert got["valid"][c][i] == (v is not None), (i, name, v)
            if v is None or t == "STRING":
                continue
            g = got["cols"][c][i]
            if t == "DOUBLE":
                assert same_double(float(g), v), (i, name, g, v)
            else:
                assert int(g) == v, (i, name, g, v)


# ------------------------------------------------------------------ the randomized decode cases

def _case(cid, fmt, fields, key, delim, seed):
    return {"id": cid, "fmt": fmt, "fields": fields, "key": key, "delim": delim, "seed": seed}


def _decode_cases():
    """key: INT32 / INT64 / STRING (key_format KAFKA), or NONE-keys / NONE-nokeys (key_format NONE,
    with the records' keys passed and ignored, or without key columns at all)."""
    out = []
    for k, d in enumerate(DELIMS):  # B.1: each delimiter, the wide and the narrow kernel variant
        out.append(_case("DELIMITED-%s-wide" % DELIM_IDS[d], "DELIMITED", FIELDS, "INT64", d, 100 + k))
        out.append(_case("DELIMITED-%s-narrow" % DELIM_IDS[d], "DELIMITED", NARROW, "INT64", d, 120 + k))
    keys = ["INT32", "INT64", "STRING", "NONE-keys", "NONE-nokeys"]
    for k, key in enumerate(keys):  # B.2: each key path, over each value format
        out.append(_case("DELIMITED-comma-key-%s" % key, "DELIMITED", FIELDS, key, ",", 140 + k))
        out.append(_case("JSON-key-%s" % key, "JSON", FIELDS if k % 2 else NARROW, key, ",", 150 + k))
    for k, t in enumerate(["INT32", "INT64", "DOUBLE"]):  # KAFKA values of each numeric type
        out.append(_case("KAFKA-%s-key-%s" % (t, keys[k]), "KAFKA", [("V", t, 0)], keys[k], ",", 160 + k))
    return out


DECODE_CASES = _decode_cases()


def ref_key_type(case):
    """The key type serde_ref.decode gets: without a key format every record has the same (empty) key."""
    return "STRING" if case["key"].startswith("NONE") else case["key"]


@functools.lru_cache(maxsize=None)
def _case_batches(cid):
    case = next(c for c in DECODE_CASES if c["id"] == cid)
    rng = random.Random(case["seed"])
    key = None if case["key"].startswith("NONE") else case["key"]
    return [records(rng, case["fmt"], case["fields"], n, key, case["delim"]) for n in SIZES]


def case_batches(case):
    """The case's batches [(keys, values)], one per size in SIZES (computed once per process)."""
    return _case_batches(case["id"])


@functools.lru_cache(maxsize=None)
def _case_reference(cid):
    import serde_ref
    case = next(c for c in DECODE_CASES if c["id"] == cid)
    return [serde_ref.decode(case["fmt"], case["fields"], ref_key_type(case), keys, vals, case["delim"])
            for keys, vals in _case_batches(cid)]


def case_reference(case):
    """serde_ref.decode of each batch of the case (computed once per process; read-only)."""
    return _case_reference(case["id"])
