"""Pure-Python restatement of the expression step (include/ksqldb_hip.h, "WHERE filters and computed
columns"): the semantics of the reference's generated Java for INT / BIGINT / DOUBLE arithmetic,
comparisons, boolean logic, null tests and numeric casts, evaluated row by row.

Python ints are wrapped to 32 / 64 bits; doubles are Python floats (IEEE binary64; math.fmod is C
fmod); every value is explicitly VALUE, NULL or ERROR (ERROR: the Java expression threw).  Test
infrastructure only; it shares nothing with ksql_amd/csrc/khip_expr.hpp.
"""
import math
import struct

import numpy as np

VALUE, NULL, ERROR = 0, 1, 2
INT32, INT64, DOUBLE, STRING, BOOL = 0, 1, 2, 3, 4
TYPE = {"INT32": INT32, "INT64": INT64, "DOUBLE": DOUBLE, "STRING": STRING}
NP = {INT32: np.int32, INT64: np.int64, DOUBLE: np.float64}

OPS = {1: "COL", 2: "CONST_I32", 3: "CONST_I64", 4: "CONST_F64",
       10: "ADD", 11: "SUB", 12: "MUL", 13: "DIV", 14: "MOD", 15: "NEG",
       20: "CAST_I32", 21: "CAST_I64", 22: "CAST_F64",
       30: "EQ", 31: "NE", 32: "LT", 33: "LE", 34: "GT", 35: "GE", 36: "DISTINCT",
       40: "AND", 41: "OR", 42: "NOT", 50: "IS_NULL", 51: "IS_NOT_NULL",
       60: "WHERE", 61: "OUT", 62: "KEY"}
ARITH = ("ADD", "SUB", "MUL", "DIV", "MOD")
CMP = ("EQ", "NE", "LT", "LE", "GT", "GE", "DISTINCT")
MAX_CODE, MAX_STACK, MAX_OUT, MAX_COLS = 64, 8, 32, 64


class Invalid(ValueError):
    """KHIP_E_INVALID at create."""


class Unsupported(ValueError):
    """KHIP_E_UNSUPPORTED at create."""


def wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def f64_bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", b & ((1 << 64) - 1)))[0]


def promote(a, b):
    return DOUBLE if DOUBLE in (a, b) else INT64 if INT64 in (a, b) else INT32


def numeric(t):
    return t in (INT32, INT64, DOUBLE)


# ------------------------------------------------------------------ Java scalar operations

def java_idiv(a, b, bits):
    """a / b on int (bits = 32) or long (64); None: ArithmeticException."""
    if b == 0:
        return None
    q = abs(a) // abs(b)
    return wrap(-q if (a < 0) != (b < 0) else q, bits)  # MIN / -1 wraps back to MIN


def java_imod(a, b, bits):
    if b == 0:
        return None
    r = abs(a) % abs(b)
    return wrap(-r if a < 0 else r, bits)  # the sign of the dividend; x % -1 = 0


def d2int(d, bits):
    """Java (int) d / (long) d."""
    if d != d:
        return 0
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if d >= hi:
        return hi
    if d <= lo:
        return lo
    return int(d)  # toward zero


def fdiv(a, b):
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    try:
        return a / b
    except OverflowError:  # (not raised for float / float; kept for safety)
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def fmod(a, b):
    try:
        return math.fmod(a, b)
    except ValueError:  # fmod(±inf, y), fmod(x, 0)
        return math.nan


def arith(op, t, a, b):
    """Both VALUE.  Returns the value, or None for an ArithmeticException."""
    if t == DOUBLE:
        if op == "ADD":
            return a + b
        if op == "SUB":
            return a - b
        if op == "MUL":
            return a * b
        if op == "DIV":
            return fdiv(a, b)
        return fmod(a, b)
    bits = 32 if t == INT32 else 64
    if op == "ADD":
        return wrap(a + b, bits)
    if op == "SUB":
        return wrap(a - b, bits)
    if op == "MUL":
        return wrap(a * b, bits)
    if op == "DIV":
        return java_idiv(a, b, bits)
    return java_imod(a, b, bits)


def compare(op, a, b):
    """The generated primitive comparison (after promotion)."""
    if op == "EQ":
        return (a <= b) and (a >= b)
    if op in ("NE", "DISTINCT"):
        return (a < b) or (a > b)
    return {"LT": a < b, "LE": a <= b, "GT": a > b, "GE": a >= b}[op]


def to_type(v, src, dst):
    """Numeric promotion / cast of a VALUE."""
    if src == dst:
        return v
    if dst == DOUBLE:
        return float(v)  # int / long -> double: round to nearest even
    if src == DOUBLE:
        return d2int(v, 32 if dst == INT32 else 64)
    return wrap(v, 32) if dst == INT32 else v


# ------------------------------------------------------------------ the program

def check(col_types, words):
    """Types a program: returns (steps, out_types, has_where, has_key); raises Invalid / Unsupported.
    steps: (name, operand, type info) per instruction."""
    col_types = [TYPE[t] if isinstance(t, str) else t for t in col_types]
    if len(col_types) > MAX_COLS:
        raise Unsupported("more than 64 input columns")
    if not words:
        raise Invalid("empty program")
    if len(words) > MAX_CODE:
        raise Unsupported("more than 64 instruction words")
    st, steps, outs = [], [], []
    has_where = has_key = any_sink = False
    i = 0

    def push(t):
        if len(st) == MAX_STACK:
            raise Unsupported("operand stack deeper than 8")
        st.append(t)
    while i < len(words):
        w = words[i]
        i += 1
        name = OPS.get(w & 0xFF)
        if name is None:
            raise Invalid("unknown opcode")
        if name == "COL":
            if len(st) == MAX_STACK:
                raise Unsupported("operand stack deeper than 8")
            c = w >> 32
            if not 0 <= c < len(col_types):
                raise Invalid("column index out of range")
            push(col_types[c])
            steps.append(("COL", c, col_types[c]))
        elif name.startswith("CONST_"):
            if len(st) == MAX_STACK:
                raise Unsupported("operand stack deeper than 8")
            if i >= len(words):
                raise Invalid("truncated constant")
            k = words[i]
            i += 1
            t = {"CONST_I32": INT32, "CONST_I64": INT64, "CONST_F64": DOUBLE}[name]
            v = wrap(k, 32) if t == INT32 else wrap(k, 64) if t == INT64 else bits_f64(k)
            push(t)
            steps.append(("CONST", v, t))
        elif name in ARITH or name in CMP or name in ("AND", "OR"):
            if len(st) < 2:
                raise Invalid("stack underflow")
            b, a = st.pop(), st.pop()
            if name in ("AND", "OR"):
                if a != BOOL or b != BOOL:
                    raise Invalid("type error")
                st.append(BOOL)
                steps.append((name, None, None))
            else:
                if not numeric(a) or not numeric(b):
                    raise Invalid("type error")
                t = promote(a, b)
                st.append(t if name in ARITH else BOOL)
                steps.append((name, (a, b), t))
        else:
            if not st:
                raise Invalid("stack underflow")
            a = st.pop()
            if name == "NEG":
                if not numeric(a):
                    raise Invalid("type error")
                st.append(a)
                steps.append(("NEG", None, a))
            elif name.startswith("CAST_"):
                if not numeric(a):
                    raise Invalid("type error")
                t = {"CAST_I32": INT32, "CAST_I64": INT64, "CAST_F64": DOUBLE}[name]
                st.append(t)
                steps.append(("CAST", a, t))
            elif name == "NOT":
                if a != BOOL:
                    raise Invalid("type error")
                st.append(BOOL)
                steps.append(("NOT", None, None))
            elif name in ("IS_NULL", "IS_NOT_NULL"):
                if a == BOOL:
                    raise Invalid("type error")
                st.append(BOOL)
                steps.append((name, None, None))
            elif name == "WHERE":
                if any_sink:
                    raise Invalid("WHERE must be the first sink")
                if a != BOOL:
                    raise Invalid("type error")
                has_where = True
                steps.append(("WHERE", None, None))
            elif name == "OUT":
                if not numeric(a):
                    raise Invalid("type error")
                if len(outs) == MAX_OUT:
                    raise Unsupported("more than 32 OUT columns")
                steps.append(("OUT", len(outs), a))
                outs.append(a)
            else:  # KEY
                if has_key:
                    raise Invalid("a second KEY")
                if a not in (INT32, INT64):
                    raise Invalid("type error")
                has_key = True
                steps.append(("KEY", None, a))
            if name in ("WHERE", "OUT", "KEY"):
                any_sink = True
        # a STRING may only sit directly under IS [NOT] NULL: every other consumer rejected it above
    if st:
        raise Invalid("values left on the stack")
    return steps, outs, has_where, has_key


def eval_row(steps, row):
    """row: per column (value, is_null).  Returns (keep, outs {index: (state, value)}, key (state, value) or
    None, n_errors).  OUT / KEY are evaluated for kept rows only, as the select follows the filter."""
    st = []
    outs, key, errors, keep = {}, None, 0, True
    for name, x, t in steps:
        if name == "COL":
            v, null = row[x]
            st.append((NULL, None) if null else (VALUE, v))
        elif name == "CONST":
            st.append((VALUE, x))
        elif name in ARITH:
            (sb, b), (sa, a) = st.pop(), st.pop()
            if sa != VALUE or sb != VALUE:  # a thrown operand, or the NullPointerException of unboxing
                st.append((ERROR, None))
            else:
                r = arith(name, t, to_type(a, x[0], t), to_type(b, x[1], t))
                st.append((ERROR, None) if r is None else (VALUE, r))
        elif name == "NEG":
            sa, a = st.pop()
            if sa != VALUE:
                st.append((ERROR, None))
            else:
                st.append((VALUE, -a if t == DOUBLE else wrap(-a, 32 if t == INT32 else 64)))
        elif name == "CAST":
            sa, a = st.pop()
            st.append((sa, to_type(a, x, t) if sa == VALUE else None))
        elif name in CMP:
            (sb, b), (sa, a) = st.pop(), st.pop()
            if name == "DISTINCT":
                # both sides are evaluated on every path of the generated ternary
                if sa == ERROR or sb == ERROR:
                    st.append((ERROR, None))
                elif sa == NULL or sb == NULL:
                    st.append((VALUE, (sa == NULL) != (sb == NULL)))
                else:
                    st.append((VALUE, compare(name, to_type(a, x[0], t), to_type(b, x[1], t))))
            elif sa == ERROR:
                st.append((ERROR, None))
            elif sa == NULL:
                st.append((VALUE, False))  # the right side is not evaluated: its ERROR is lost
            elif sb == ERROR:
                st.append((ERROR, None))
            elif sb == NULL:
                st.append((VALUE, False))
            else:
                st.append((VALUE, compare(name, to_type(a, x[0], t), to_type(b, x[1], t))))
        elif name in ("AND", "OR"):
            (sb, b), (sa, a) = st.pop(), st.pop()
            if sa == ERROR:
                st.append((ERROR, None))
            elif name == "AND":
                st.append((VALUE, False) if not a else (ERROR, None) if sb == ERROR else (VALUE, bool(b)))
            else:
                st.append((VALUE, True) if a else (ERROR, None) if sb == ERROR else (VALUE, bool(b)))
        elif name == "NOT":
            sa, a = st.pop()
            st.append((sa, (not a) if sa == VALUE else None))
        elif name in ("IS_NULL", "IS_NOT_NULL"):
            sa, a = st.pop()
            st.append((ERROR, None) if sa == ERROR else (VALUE, (sa == NULL) == (name == "IS_NULL")))
        elif name == "WHERE":
            sa, a = st.pop()
            if sa == ERROR:
                errors += 1
            keep = sa == VALUE and bool(a)
            if not keep:
                return False, {}, None, errors
        elif name == "OUT":
            sa, a = st.pop()
            errors += sa == ERROR
            outs[x] = (sa, a)
        else:  # KEY
            sa, a = st.pop()
            errors += sa == ERROR
            key = (sa, a)
    return keep, outs, key, errors


def _valid(bm, n):
    return np.ones(n, bool) if bm is None else np.asarray(bm, bool)


def apply(col_types, words, batch):
    """batch: dict with ts (int64 array) and optionally key (int64 array) or utf8_keys (list of bytes),
    key_valid / row_valid (bool arrays or None), cols (list of arrays), valid (list of bool arrays or
    None), partition, stream_time.  Returns the output batch as Expr.columns() shapes it, every bitmap
    a bool array, plus n_errors."""
    types = [TYPE[t] if isinstance(t, str) else t for t in col_types]
    steps, out_types, has_where, has_key = check(types, words)
    ts = np.asarray(batch["ts"], np.int64)
    n = len(ts)
    cols = batch.get("cols", [])
    valid = list(batch.get("valid", [])) + [None] * (len(cols) - len(batch.get("valid", [])))
    cvalid = [_valid(v, n) for v in valid]
    row_valid, key_valid = _valid(batch.get("row_valid"), n), _valid(batch.get("key_valid"), n)
    pycols = []
    for c, t in enumerate(types):
        if c >= len(cols) or cols[c] is None or t == STRING:
            pycols.append([0] * n)
        elif t == DOUBLE:
            pycols.append([float(v) for v in np.asarray(cols[c], np.float64)])
        else:
            pycols.append([int(v) for v in cols[c]])
    kept, o_cols, o_valid = [], [[] for _ in out_types], [[] for _ in out_types]
    o_key, o_key_valid, n_errors = [], [], 0
    for r in range(n):
        if not row_valid[r]:
            if has_where:
                continue  # a null value never reaches the predicate
            kept.append(r)
            for c in range(len(out_types)):
                o_cols[c].append(0)
                o_valid[c].append(False)
            o_key.append(0)
            o_key_valid.append(False)
            continue
        row = [(pycols[c][r], not (c < len(cvalid) and cvalid[c][r]) if c < len(cols) else True)
               for c in range(len(types))]
        keep, outs, key, errs = eval_row(steps, row)
        n_errors += errs
        if not keep:
            continue
        kept.append(r)
        for c in range(len(out_types)):
            s, v = outs[c]
            o_cols[c].append(v if s == VALUE else 0)
            o_valid[c].append(s == VALUE)
        if has_key:
            o_key.append(key[1] if key[0] == VALUE else 0)
            o_key_valid.append(key[0] == VALUE)
    kept = np.asarray(kept, np.int64)
    res = {"n": len(kept), "ts": ts[kept], "row_valid": row_valid[kept], "n_errors": n_errors,
           "cols": [np.asarray(o_cols[c], NP[t]) for c, t in enumerate(out_types)],
           "valid": [np.asarray(o_valid[c], bool) for c in range(len(out_types))],
           "out_types": out_types, "key": None, "key_offsets": None, "key_bytes": None, "rows": kept}
    for f, dt in (("partition", np.int32), ("stream_time", np.int64)):
        res[f] = None if batch.get(f) is None else np.asarray(batch[f], dt)[kept]
    if has_key:
        res["key"] = np.asarray(o_key, np.int64)
        res["key_valid"] = np.asarray(o_key_valid, bool)
    else:
        res["key_valid"] = key_valid[kept]
        if batch.get("utf8_keys") is not None:
            ks = [b"" if k is None else bytes(k) for k in batch["utf8_keys"]]
            ks = [ks[r] for r in kept]
            res["key_offsets"] = np.concatenate([[0], np.cumsum([len(k) for k in ks])]).astype(np.int64)
            res["key_bytes"] = np.frombuffer(b"".join(ks), np.uint8).copy()
        elif batch.get("key") is not None:
            res["key"] = np.asarray(batch["key"], np.int64)[kept]
    return res
