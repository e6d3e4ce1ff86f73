// khip_sink.hip — serialization of columnar rows into Kafka record bytes (gfx950).
//
// The output side of GenericKeySerDe / GenericRowSerDe (include/ksqldb_hip.h "serialization"):
// an aggregate's changelog rows become sink records — the inner key in the key format, Kafka
// Streams' windowed key suffix, the value in the value format or a null value for a tombstone —
// and several GROUP BY columns become the serialized composite key the aggregate groups by.
//
// Two passes over tiles of 256 rows, one thread per row: k_sink_measure runs the very
// encoder the write pass runs, with a counting writer, so a row's length and its bytes can never
// disagree, and sums each tile's lengths; one block scans the tile sums; k_sink_write scans its
// tile's lengths in the block, adds the tile's carry and writes each record at its offset, and
// the offsets.  A KAFKA INT32 / BIGINT key has a fixed width (no key lengths; a BIGINT key and its
// window suffix leave as 8-byte words), and a JSON column's '{' / ',' + escaped name + ':' is built
// once on the host.  The three kernels are templates over the value encoder ("the value encoders"
// below): TextEnc for JSON / DELIMITED / KAFKA values, AvroEnc for AVRO values (the Confluent wire
// format of ksqlDB's own schema: scalars and ARRAY columns, keys as above; the lengths in closed
// form) and PbEnc for PROTOBUF / PROTOBUF_NOSR values.  A sink with an ARRAY value column
// (KHIP_SINK_ARRAY) runs its own instantiations, k_sink_measure<Enc, true> and
// k_sink_write_arr<Enc>; a scalar sink's kernels carry none of it.  Doubles print
// through the Schubfach shortest-decimal algorithm (R. Giulietti 2020; java.lang.Double.toString
// since JDK 19) with the 126-bit powers of ten of tools/gen_dtoa.py, so every digit is computed
// exactly with 64-bit integer arithmetic.  Byte parity of DOUBLE text therefore assumes the
// reference runs on JDK 19 or later: JDK <= 18's FloatingDecimal prints longer digit strings for
// some values (tests/sink_ref.py lists them); on such a JVM the values still parse to the same
// double, but the bytes differ (DESIGN.md §(c), unpinned).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "khip_util.hpp"

namespace khip {

constexpr int SK_MAX = KHIP_SINK_MAX_COLS;
constexpr int SK_NAME = 64;
constexpr int SK_PRE = 72;  // a JSON column's text before its value, escaped name included
// The write pass's outputs leave as nontemporal stores: k_sink_write 717 / 719 us per 22M rows
// against 750 / 751 (profiles/r05/ab/sink_two_pass.txt).
#ifndef KHIP_SINK_NT
#define KHIP_SINK_NT 1
#endif
template <class T>
__device__ __forceinline__ void sk_st(T* p, T v) {
  if (KHIP_SINK_NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

constexpr int SK_SCAN_T = 1024;
constexpr int SK_SCAN_I = 8;  // items per thread per scan block

__device__ const uint64_t kDtoaG[617][2] = {
#include "khip_dtoa.inc"
};

struct SinkParams {
  int32_t key_format, n_key, window_kind, value_format, n_val, delim;
  int32_t ktype[SK_MAX], vtype[SK_MAX], vsrc[SK_MAX];
  int32_t kname_len[SK_MAX], vname_len[SK_MAX];
  uint8_t kname[SK_MAX][SK_NAME], vname[SK_MAX][SK_NAME];
  // JSON object columns: '{' (first) or ',', the escaped quoted name and ':' — built once on the
  // host by the device's own escaper (put_json_str); length -1 when longer than SK_PRE
  int32_t kpre_len[SK_MAX], vpre_len[SK_MAX];
  alignas(8) uint8_t kpre[SK_MAX][SK_PRE];
  alignas(8) uint8_t vpre[SK_MAX][SK_PRE];
  // ARRAY value columns (JSON and AVRO values): the slots per row, KHIP_SINK_ARRAY's L; 0 = the scalar
  // column (vtype is the element type either way)
  int32_t varr[SK_MAX];
};

// ------------------------------------------------------------------ writers

struct CountW {
  int64_t n = 0;
  __device__ __forceinline__ void put(uint8_t) { n++; }
};
struct MemW {
  uint8_t* p;
  __device__ __forceinline__ void put(uint8_t c) { *p++ = c; }
  __device__ __forceinline__ static MemW at(uint32_t* stage, int64_t off) { return MemW{(uint8_t*)stage + off}; }
};
struct HostW {  // host: a JSON column prefix (SinkParams::kpre / vpre)
  uint8_t* p;
  int n, cap;
  void put(uint8_t c) {
    if (n < cap) p[n] = c;
    n++;
  }
};
constexpr int SK_ABUF = 32768;  // k_sink_write_arr's stage: a tile's value bytes per round
// WinW keeps the bytes that fall into a window of SK_ABUF bytes of LDS; rel: the next byte's place in
// it, negative while a row that began in the window before is still outside.  b is an LDS
// address-space pointer, so that the stores are DS instructions.  Through a generic pointer they
// are FLAT stores, and the hardware picks a FLAT access's aperture from the base register without
// the instruction's offset field: consecutive puts compile to one base and offsets :1, :2, ..., and
// with rel < 0 at the first of them and the stage at LDS offset 0 that base lies below the LDS
// aperture (a memory aperture violation, although every stored byte is inside the window).
typedef __attribute__((address_space(3))) uint8_t sk_lds_u8;
struct WinW {
  sk_lds_u8* b;
  int64_t rel;
  __device__ __forceinline__ void put(uint8_t c) {
    if ((uint64_t)rel < (uint64_t)SK_ABUF) b[rel] = c;
    rel++;
  }
};
struct BufW {  // a field's text, for the CSV quoting decision
  uint8_t b[40];
  int n = 0;
  __device__ __forceinline__ void put(uint8_t c) { b[n++] = c; }
};

// ------------------------------------------------------------------ numbers

// Long.toString.  The digits collect in a 24-byte shift register (d2:d1:d0, each new digit in at
// the bottom, so the most significant ends in byte 0): registers, where a digit array indexed by a
// variable would live in scratch memory.
template <class W>
__device__ __forceinline__ void put_i64(W& w, int64_t v) {
  uint64_t u = v < 0 ? 0ULL - (uint64_t)v : (uint64_t)v;
  uint64_t d0 = 0, d1 = 0, d2 = 0;
  int n = 0;
  auto push = [&](uint64_t dig) {
    d2 = (d2 << 8) | (d1 >> 56);
    d1 = (d1 << 8) | (d0 >> 56);
    d0 = (d0 << 8) | ('0' + dig);
    n++;
  };
  while (u >> 32) {
    push(u % 10);
    u /= 10;
  }
  uint32_t x = (uint32_t)u;
  do {
    push(x % 10);
    x /= 10;
  } while (x);
  if (v < 0) w.put('-');
  for (; n; n--) {
    w.put((uint8_t)d0);
    d0 = (d0 >> 8) | (d1 << 56);
    d1 = (d1 >> 8) | (d2 << 56);
    d2 >>= 8;
  }
}

__device__ __forceinline__ int flog10pow2(int q) { return (int)(((int64_t)q * 661971961083LL) >> 41); }
__device__ __forceinline__ int flog10tqpow2(int q) { return (int)(((int64_t)q * 661971961083LL - 274743187321LL) >> 41); }
__device__ __forceinline__ int flog2pow10(int e) { return (int)(((int64_t)e * 913124641741LL) >> 38); }

constexpr uint64_t MASK63 = 0x7FFFFFFFFFFFFFFFULL;

// round to odd of the product g * cp (Schubfach's rop)
__device__ __forceinline__ uint64_t sk_rop(uint64_t g1, uint64_t g0, uint64_t cp) {
  const uint64_t x1 = __umul64hi(g0, cp);
  const uint64_t y0 = g1 * cp;
  const uint64_t y1 = __umul64hi(g1, cp);
  const uint64_t z = (y0 >> 1) + x1;
  const uint64_t vbp = y1 + (z >> 63);
  return vbp | (((z & MASK63) + MASK63) >> 63);
}

// c 2^q → the shortest decimal f 10^e in its rounding interval (closest; even on ties)
__device__ void sk_to_decimal(int q, uint64_t c, int dk, uint64_t* fo, int* eo) {
  const uint64_t out = c & 1;
  const uint64_t cb = c << 2, cbr = cb + 2;
  uint64_t cbl;
  int k;
  if (c != (1ULL << 52) || q == -1074) {
    cbl = cb - 2;
    k = flog10pow2(q);
  } else {
    cbl = cb - 1;
    k = flog10tqpow2(q);
  }
  const int h = q + flog2pow10(-k) + 2;
  const uint64_t g1 = kDtoaG[k + 324][0], g0 = kDtoaG[k + 324][1];
  const uint64_t vb = sk_rop(g1, g0, cb << h);
  const uint64_t vbl = sk_rop(g1, g0, cbl << h);
  const uint64_t vbr = sk_rop(g1, g0, cbr << h);
  const uint64_t s = vb >> 2;
  if (s >= 100) {
    const uint64_t sp10 = 10 * __umul64hi(s, 115292150460684698ULL << 4);
    const uint64_t tp10 = sp10 + 10;
    const bool upin = vbl + out <= sp10 << 2;
    const bool wpin = (tp10 << 2) + out <= vbr;
    if (upin != wpin) {
      *fo = upin ? sp10 : tp10;
      *eo = k;
      return;
    }
  }
  const uint64_t t = s + 1;
  const bool uin = vbl + out <= s << 2;
  const bool win = (t << 2) + out <= vbr;
  if (uin != win) {
    *fo = uin ? s : t;
    *eo = k + dk;
    return;
  }
  const int64_t cmp = (int64_t)(vb - ((s + t) << 1));
  *fo = cmp < 0 || (cmp == 0 && (s & 1) == 0) ? s : t;
  *eo = k + dk;
}

// Double.toString of a finite double
template <class W>
__device__ void put_f64(W& w, double v) {
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  const uint64_t t = bits & ((1ULL << 52) - 1);
  const int bq = (int)((bits >> 52) & 0x7FF);
  if (bits >> 63) w.put('-');
  uint64_t f;
  int e;
  if (bq != 0) {
    const int mq = 1075 - bq;
    const uint64_t c = (1ULL << 52) | t;
    if (mq > 0 && mq < 53 && ((c >> mq) << mq) == c) {
      f = c >> mq;
      e = 0;
    } else {
      sk_to_decimal(-mq, c, 0, &f, &e);
    }
  } else if (t != 0) {
    if (t < 3) sk_to_decimal(-1074, 10 * t, -1, &f, &e);
    else sk_to_decimal(-1074, t, 0, &f, &e);
  } else {
    w.put('0');
    w.put('.');
    w.put('0');
    return;
  }
  // digits of f, then Java's layout (DoubleToDecimal.toChars): plain for 1e-3 <= |v| < 1e7,
  // computerized scientific notation otherwise; at least one digit after the point
  uint8_t d[20];
  int L = 0;
  {
    uint8_t r[20];
    uint64_t u = f;
    do {
      r[L++] = (uint8_t)('0' + u % 10);
      u /= 10;
    } while (u);
    for (int i = 0; i < L; i++) d[i] = r[L - 1 - i];
  }
  const int e10 = e + L;  // |v| = 0.d 10^e10
  int nd = L;
  while (nd > 1 && d[nd - 1] == '0') nd--;
  if (e10 > 0 && e10 <= 7) {
    for (int i = 0; i < e10; i++) w.put(i < nd ? d[i] : (uint8_t)'0');
    w.put('.');
    if (nd > e10) {
      for (int i = e10; i < nd; i++) w.put(d[i]);
    } else {
      w.put('0');
    }
  } else if (e10 > -3 && e10 <= 0) {
    w.put('0');
    w.put('.');
    for (int i = 0; i < -e10; i++) w.put('0');
    for (int i = 0; i < nd; i++) w.put(d[i]);
  } else {
    w.put(d[0]);
    w.put('.');
    if (nd > 1) {
      for (int i = 1; i < nd; i++) w.put(d[i]);
    } else {
      w.put('0');
    }
    w.put('E');
    put_i64(w, (int64_t)(e10 - 1));
  }
}

// Double.toString of any double (NaN, Infinity, -Infinity)
template <class W>
__device__ void put_f64_any(W& w, double v) {
  if (v != v) {
    w.put('N'); w.put('a'); w.put('N');
  } else if (v == __builtin_inf() || v == -__builtin_inf()) {
    if (v < 0) w.put('-');
    const char* s = "Infinity";
    for (int i = 0; i < 8; i++) w.put((uint8_t)s[i]);
  } else {
    put_f64(w, v);
  }
}

// ------------------------------------------------------------------ values

struct Val {
  int64_t i;  // INT32 / INT64 (sign-extended); DOUBLE: the bits
  const uint8_t* s;
  int64_t len;  // STRING
  bool null;
};

// f(byte) over s[0..len), the bytes loaded eight at a time: on gfx950 a load issued behind a store
// waits for the store (one vmcnt counts both), so a byte-by-byte copy would wait a memory round
// trip per byte.
template <class F>
__host__ __device__ __forceinline__ void for_bytes(const uint8_t* s, int64_t len, F&& f) {
  for (int64_t j = 0; j < len; j += 8) {
    uint64_t x = 0;
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (j + b < len) x |= (uint64_t)s[j + b] << (8 * b);
    const int m = len - j < 8 ? (int)(len - j) : 8;
    for (int b = 0; b < m; b++) f((uint8_t)(x >> (8 * b)));
  }
}

template <class W>
__device__ void put_be(W& w, uint64_t v, int nbytes) {
  for (int b = nbytes - 1; b >= 0; b--) w.put((uint8_t)(v >> (8 * b)));
}

// Jackson's string escaping: quote, backslash, the short escapes, \u00XX for other control bytes
template <class W>
__host__ __device__ void put_json_str(W& w, const uint8_t* s, int64_t len) {
  w.put('"');
  for_bytes(s, len, [&](uint8_t c) {
    if (c == '"' || c == '\\') {
      w.put('\\');
      w.put(c);
    } else if (c < 0x20) {
      w.put('\\');
      switch (c) {
        case 0x08: w.put('b'); break;
        case 0x09: w.put('t'); break;
        case 0x0A: w.put('n'); break;
        case 0x0C: w.put('f'); break;
        case 0x0D: w.put('r'); break;
        default: {
          const char* hx = "0123456789ABCDEF";
          w.put('u'); w.put('0'); w.put('0');
          w.put((uint8_t)hx[c >> 4]);
          w.put((uint8_t)hx[c & 15]);
        }
      }
    } else {
      w.put(c);
    }
  });
  w.put('"');
}

template <class W>
__device__ void put_json_val(W& w, int type, const Val& v) {
  if (v.null) {
    w.put('n'); w.put('u'); w.put('l'); w.put('l');
    return;
  }
  if (type == KHIP_TYPE_DOUBLE) {
    const double d = __longlong_as_double(v.i);
    if (d != d || d == __builtin_inf() || d == -__builtin_inf()) {  // QUOTE_NON_NUMERIC_NUMBERS
      w.put('"');
      put_f64_any(w, d);
      w.put('"');
    } else {
      put_f64(w, d);
    }
  } else if (type == KHIP_TYPE_STRING) {
    put_json_str(w, v.s, v.len);
  } else {
    put_i64(w, v.i);
  }
}

// commons-csv 1.4 CSVFormat.printAndQuote, QuoteMode.MINIMAL (KsqlDelimitedSerializer's CSVPrinter)
template <class W>
__device__ void put_csv_text(W& w, const uint8_t* s, int64_t len, bool first, uint8_t delim) {
  bool quote = false;
  if (len <= 0) {
    quote = first;
  } else {
    const uint8_t c = s[0];
    if (first && (c < 0x20 || (c > 0x21 && c < 0x23) || (c > 0x2B && c < 0x2D) || c > 0x7E)) {
      quote = true;
    } else if (c <= '#') {
      quote = true;
    } else {
      for (int64_t i = 0; i < len && !quote; i++) {
        const uint8_t x = s[i];
        quote = x == '\n' || x == '\r' || x == '"' || x == delim;
      }
      if (!quote) quote = s[len - 1] <= ' ';
    }
  }
  if (quote) w.put('"');
  for_bytes(s, len, [&](uint8_t c) {
    if (quote && c == '"') w.put('"');
    w.put(c);
  });
  if (quote) w.put('"');
}

template <class W>
__device__ void put_csv_val(W& w, int type, const Val& v, bool first, uint8_t delim) {
  if (v.null) return;  // CSVPrinter.print(null) with no null string: nothing, unquoted
  if (type == KHIP_TYPE_STRING) {
    put_csv_text(w, v.s, v.len, first, delim);
    return;
  }
  BufW b;
  if (type == KHIP_TYPE_DOUBLE) put_f64_any(b, __longlong_as_double(v.i));
  else put_i64(b, v.i);
  put_csv_text(w, b.b, b.n, first, delim);
}

// KAFKA format primitive bytes (kafka/KafkaSerdeFactory.java:42-46)
template <class W>
__device__ void put_kafka_val(W& w, int type, const Val& v) {
  if (type == KHIP_TYPE_INT32) put_be(w, (uint64_t)(uint32_t)v.i, 4);
  else if (type == KHIP_TYPE_STRING)
    for_bytes(v.s, v.len, [&](uint8_t c) { w.put(c); });
  else put_be(w, (uint64_t)v.i, 8);
}

// the inner key (never null: a null GROUP BY value drops the row upstream)
// A column prefix: 8-byte words from the parameters, put byte by byte from registers.
template <class W>
__device__ __forceinline__ void put_pre(W& w, const uint8_t* pre, int len) {
  for (int j = 0; j < len; j += 8) {
    const uint64_t x = *(const uint64_t*)(pre + j);
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (j + b < len) w.put((uint8_t)(x >> (8 * b)));
  }
}

template <class W, class F>
__device__ void put_key(W& w, const SinkParams& q, F&& kval) {
  if (q.key_format == KHIP_FMT_KAFKA) {
    put_kafka_val(w, q.ktype[0], kval(0));
  } else if (q.key_format == KHIP_FMT_JSON) {
    if (q.n_key == 1) {
      put_json_val(w, q.ktype[0], kval(0));
    } else {
      for (int i = 0; i < q.n_key; i++) {
        if (q.kpre_len[i] >= 0) {
          put_pre(w, q.kpre[i], q.kpre_len[i]);
        } else {
          w.put(i ? ',' : '{');
          put_json_str(w, q.kname[i], q.kname_len[i]);
          w.put(':');
        }
        put_json_val(w, q.ktype[i], kval(i));
      }
      w.put('}');
    }
  } else {
    for (int i = 0; i < q.n_key; i++) {
      if (i) w.put((uint8_t)q.delim);
      put_csv_val(w, q.ktype[i], kval(i), i == 0, (uint8_t)q.delim);
    }
  }
}

// ARR: the instantiation for sinks with an ARRAY column; velem(c, e, v) fetches element e of the
// row's list in column c and answers false at the list's end (the one rule of row_elem).  Without
// ARR velem is never called and the code is the scalar encoder's.
template <bool ARR, class W, class F, class G>
__device__ __forceinline__ void put_value(W& w, const SinkParams& q, F&& vval, G&& velem) {
  if (q.value_format == KHIP_FMT_KAFKA) {
    put_kafka_val(w, q.vtype[0], vval(0));
  } else if (q.value_format == KHIP_FMT_JSON) {
    if (q.n_val == 0) w.put('{');
    for (int i = 0; i < q.n_val; i++) {
      if (q.vpre_len[i] >= 0) {
        put_pre(w, q.vpre[i], q.vpre_len[i]);
      } else {
        w.put(i ? ',' : '{');
        put_json_str(w, q.vname[i], q.vname_len[i]);
        w.put(':');
      }
      if (ARR && q.varr[i] > 0) {
        w.put('[');
        Val v;
        for (int e = 0; velem(i, e, v); e++) {
          if (e) w.put(',');
          put_json_val(w, q.vtype[i], v);
        }
        w.put(']');
        continue;
      }
      put_json_val(w, q.vtype[i], vval(i));
    }
    w.put('}');
  } else {
    for (int i = 0; i < q.n_val; i++) {
      if (i) w.put((uint8_t)q.delim);
      put_csv_val(w, q.vtype[i], vval(i), i == 0, (uint8_t)q.delim);
    }
  }
}

// ------------------------------------------------------------------ AVRO values
//
// The Confluent wire format of the record ksqlDB's own schema describes (include/ksqldb_hip.h,
// "AVRO values"): byte 0, the schema id big-endian, then per column the union ["null", T] — branch
// 0 for NULL, branch 1 (the byte 0x02) and the value.  An AVRO sink runs the kernels' AvroEnc
// instantiations: put_value and the other formats' instantiations carry none of this.

__device__ __forceinline__ uint64_t avro_zz(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
// bytes of the varint of u: seven bits a byte
__device__ __forceinline__ int avro_varint_len(uint64_t u) { return (63 - __clzll((long long)(u | 1))) / 7 + 1; }

template <class W>
__device__ __forceinline__ void put_avro_varint(W& w, uint64_t u) {
  while (u >> 7) {
    w.put((uint8_t)(u | 0x80));
    u >>= 7;
  }
  w.put((uint8_t)u);
}

// An optional INT32 / INT64 (v.i sign-extended: an int's zig-zag is the long's) or DOUBLE (the raw
// bits, little-endian).
template <class W>
__device__ __forceinline__ void put_avro_val(W& w, int type, const Val& v) {
  if (v.null) {
    w.put(0);
    return;
  }
  w.put(2);
  if (type == KHIP_TYPE_DOUBLE) {
#pragma unroll
    for (int b = 0; b < 8; b++) w.put((uint8_t)((uint64_t)v.i >> (8 * b)));
  } else {
    put_avro_varint(w, avro_zz(v.i));
  }
}
__device__ __forceinline__ int avro_val_len(int type, const Val& v) {
  return v.null ? 1 : type == KHIP_TYPE_DOUBLE ? 9 : 1 + avro_varint_len(avro_zz(v.i));
}

// vcount(c): the length of the row's list in ARRAY column c; velem as for put_value.  A list is one
// block (its length, its items, the end byte 0); the empty list is the end byte alone.
template <bool ARR, class W, class F, class C, class G>
__device__ __forceinline__ void put_avro_value(W& w, const SinkParams& q, int32_t schema_id, F&& vval, C&& vcount,
                                               G&& velem) {
  w.put(0);
  put_be(w, (uint64_t)(uint32_t)schema_id, 4);
  for (int i = 0; i < q.n_val; i++) {
    if (ARR && q.varr[i] > 0) {
      w.put(2);
      const int cnt = vcount(i);
      if (cnt) put_avro_varint(w, (uint64_t)cnt << 1);
      Val v;
      for (int e = 0; e < cnt && velem(i, e, v); e++) put_avro_val(w, q.vtype[i], v);
      w.put(0);
      continue;
    }
    put_avro_val(w, q.vtype[i], vval(i));
  }
}

// ------------------------------------------------------------------ rows → records

struct RowsDev {
  int32_t key_serialized;
  const int64_t* key_i64;
  const int64_t* key_off;
  const uint8_t* key_bytes;
  const int64_t* ws;
  const int64_t* we;
  const uint8_t* tomb;
  const void* col[SK_MAX];
  const uint8_t* cnull[SK_MAX];
};

__device__ __forceinline__ Val row_key_val(const SinkParams& q, const RowsDev& r, int64_t i) {
  Val v{0, nullptr, 0, false};
  if (q.ktype[0] == KHIP_TYPE_STRING) {
    v.s = r.key_bytes + r.key_off[i];
    v.len = r.key_off[i + 1] - r.key_off[i];
  } else {
    v.i = q.ktype[0] == KHIP_TYPE_INT32 ? (int64_t)(int32_t)r.key_i64[i] : r.key_i64[i];
  }
  return v;
}

__device__ __forceinline__ Val row_value_val(const SinkParams& q, const RowsDev& r, int64_t i, int c) {
  Val v{0, nullptr, 0, false};
  const int src = q.vsrc[c];
  if (src == KHIP_SINK_SRC_WS) {
    v.i = r.ws[i];
  } else if (src == KHIP_SINK_SRC_WE) {
    v.i = r.we[i];
  } else {
    v.null = r.cnull[src] && r.cnull[src][i];
    if (q.vtype[c] == KHIP_TYPE_INT32) v.i = ((const int32_t*)r.col[src])[i];
    else v.i = ((const int64_t*)r.col[src])[i];  // INT64, DOUBLE bits
  }
  return v;
}

// Element e of row i's list in ARRAY column c (L slots per row, khip_snapshot's layout): the list is
// the row's leading slots whose null byte is 0 (an element) or 2 (a NULL element); any other byte,
// or slot L, ends it.  The measure pass and the write pass both read the length here.
__device__ __forceinline__ bool row_elem(const SinkParams& q, const RowsDev& r, int64_t i, int c, int e, Val& v) {
  const int L = q.varr[c], src = q.vsrc[c];
  if (e >= L) return false;
  const int64_t at = i * L + e;
  const uint8_t nb = r.cnull[src][at];
  if (nb != 0 && nb != 2) return false;
  v = Val{0, nullptr, 0, nb == 2};
  if (q.vtype[c] == KHIP_TYPE_INT32) v.i = ((const int32_t*)r.col[src])[at];
  else v.i = ((const int64_t*)r.col[src])[at];
  return true;
}

// The row's window bounds, loaded before any of its bytes are stored.
struct RowWin {
  int64_t ws, we;
};
__device__ __forceinline__ RowWin row_win(const SinkParams& q, const RowsDev& r, int64_t i) {
  RowWin x{0, 0};
  if (q.window_kind != KHIP_WINDOW_NONE) x.ws = r.ws[i];
  if (q.window_kind == KHIP_WINDOW_SESSION) x.we = r.we[i];
  return x;
}

template <class W>
__device__ __forceinline__ void encode_key_row(W& w, const SinkParams& q, const RowsDev& r, int64_t i) {
  const RowWin win = row_win(q, r, i);
  if (r.key_serialized) {
    const int64_t b0 = r.key_off[i], b1 = r.key_off[i + 1];
    for_bytes(r.key_bytes + b0, b1 - b0, [&](uint8_t c) { w.put(c); });
  } else {
    const Val kv = row_key_val(q, r, i);
    put_key(w, q, [&](int) { return kv; });
  }
  if (q.window_kind == KHIP_WINDOW_TUMBLING || q.window_kind == KHIP_WINDOW_HOPPING) {
    put_be(w, (uint64_t)win.ws, 8);
  } else if (q.window_kind == KHIP_WINDOW_SESSION) {
    put_be(w, (uint64_t)win.we, 8);
    put_be(w, (uint64_t)win.ws, 8);
  }
}

// a value that is a null record: a tombstone, or a KAFKA-format value whose one column is NULL
__device__ __forceinline__ bool value_is_null(const SinkParams& q, const RowsDev& r, int64_t i) {
  if (r.tomb && r.tomb[i]) return true;
  return q.value_format == KHIP_FMT_KAFKA && row_value_val(q, r, i, 0).null;
}

// Tiles of SK_TILE = 256 rows, one block of 256 threads, one row per thread (eight rows per
// thread in rounds, measured earlier, kept the write pass's row state live across rounds: 171
// VGPRs).
constexpr int SK_TILE = 256;
// k_sink_write at 4 waves per SIMD (<= 128 VGPRs; the spills are in the DOUBLE printer): 782-802
// us per 22M rows against 840 at 5 and 890 uncapped (138 VGPRs), profiles/r05/ab/sink_two_pass.txt
#ifndef KHIP_SINK_MINB
#define KHIP_SINK_MINB 4
#endif
#define KHIP_SINK_WRITE_LB __launch_bounds__(256, KHIP_SINK_MINB)

// Sums of (a, b) over the block; every thread gets them.
__device__ __forceinline__ void sk_block_sum2(int64_t& a, int64_t& b, int64_t (*ws)[4]) {
  for (int off = 32; off; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    ws[0][wave] = a;
    ws[1][wave] = b;
  }
  __syncthreads();
  a = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
  b = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
  __syncthreads();
}

// Exclusive scans of (a, b) over the block; the block totals in ta, tb.
__device__ __forceinline__ void sk_block_scan2(int64_t& a, int64_t& b, int64_t& ta, int64_t& tb, int64_t (*ws)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t ia = a, ib = b;
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t ya = __shfl_up(ia, off, 64), yb = __shfl_up(ib, off, 64);
    if (lane >= off) {
      ia += ya;
      ib += yb;
    }
  }
  if (lane == 63) {
    ws[0][wave] = ia;
    ws[1][wave] = ib;
  }
  __syncthreads();
  int64_t pa = 0, pb = 0;
  ta = tb = 0;
  for (int w = 0; w < 4; w++) {
    pa += w < wave ? ws[0][w] : 0;
    pb += w < wave ? ws[1][w] : 0;
    ta += ws[0][w];
    tb += ws[1][w];
  }
  __syncthreads();
  a = pa + ia - a;
  b = pb + ib - b;
}

// A fixed-width KAFKA BIGINT key and its window suffix as big-endian 8-byte words (kb + 8-aligned),
// every load before the first store.
__device__ __forceinline__ void put_key_words(const SinkParams& q, const RowsDev& r, int64_t i, uint64_t* o) {
  const RowWin win = row_win(q, r, i);
  const uint64_t k = __builtin_bswap64((uint64_t)r.key_i64[i]);
  if (q.window_kind == KHIP_WINDOW_TUMBLING || q.window_kind == KHIP_WINDOW_HOPPING) {
    if (((uintptr_t)o & 15) == 0) {
      if (KHIP_SINK_NT) {
        __builtin_nontemporal_store(k, o);
        __builtin_nontemporal_store(__builtin_bswap64((uint64_t)win.ws), o + 1);
      } else {
        *(ulonglong2*)o = make_ulonglong2(k, __builtin_bswap64((uint64_t)win.ws));
      }
    } else {
      o[0] = k;
      o[1] = __builtin_bswap64((uint64_t)win.ws);
    }
  } else if (q.window_kind == KHIP_WINDOW_SESSION) {
    o[0] = k;
    o[1] = __builtin_bswap64((uint64_t)win.we);
    o[2] = __builtin_bswap64((uint64_t)win.ws);
  } else {
    o[0] = k;
  }
}

// A wave's value bytes, staged contiguously in LDS (lds[0..L)), to dst[0..L): 16-byte aligned
// chunks, one per lane and round — whole 16-byte stores inside, bytes at the two edge chunks
// (shared with the neighbouring waves).  lds has 16 readable bytes past L.
// sk_range_copy<NT>: the same by NT threads, this one being thread t (k_sink_write_arr: the block).
template <int NT>
__device__ __forceinline__ void sk_range_copy(const uint8_t* lds, int L, uint8_t* __restrict__ dst, int t);
__device__ __forceinline__ void sk_wave_copy(const uint8_t* lds, int L, uint8_t* __restrict__ dst) {
  sk_range_copy<64>(lds, L, dst, threadIdx.x & 63);
}
template <int NT>
__device__ __forceinline__ void sk_range_copy(const uint8_t* lds, int L, uint8_t* __restrict__ dst, int t) {
  const int A = (int)((uintptr_t)dst & 15);
  const int nch = (A + L + 15) >> 4;
  const uint32_t* l32 = (const uint32_t*)lds;
  for (int c = t; c < nch; c += NT) {
    const int o = 16 * c - A;
    uint8_t* g = dst + o;
    if (o >= 0 && o + 16 <= L) {
      const int ao = o >> 2, sh = o & 3;
      const uint32_t w0 = l32[ao], w1 = l32[ao + 1], w2 = l32[ao + 2], w3 = l32[ao + 3], w4 = l32[ao + 4];
      uint4 v;
      v.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
      v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
      v.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
      v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
      if (KHIP_SINK_NT) {
        __builtin_nontemporal_store(v.x, (uint32_t*)g);
        __builtin_nontemporal_store(v.y, (uint32_t*)g + 1);
        __builtin_nontemporal_store(v.z, (uint32_t*)g + 2);
        __builtin_nontemporal_store(v.w, (uint32_t*)g + 3);
      } else {
        *(uint4*)g = v;
      }
    } else {
      for (int b = 0; b < 16; b++)
        if (o + b >= 0 && o + b < L) g[b] = lds[o + b];
    }
  }
}

constexpr int SK_WBUF = 2048;  // staged value bytes per wave: 64 rows of 32

// ------------------------------------------------------------------ AVRO values of rows
//
// put_avro_value's inputs from the rows, and a value's length in closed form: the measure pass of
// an AVRO sink runs no byte writer.

// the length of row i's list in ARRAY column c: row_elem's rule, the null bytes alone
__device__ __forceinline__ int row_list_len(const SinkParams& q, const RowsDev& r, int64_t i, int c) {
  const int L = q.varr[c];
  const uint8_t* nb = r.cnull[q.vsrc[c]] + i * L;
  int e = 0;
  while (e < L && (nb[e] == 0 || nb[e] == 2)) e++;
  return e;
}

// the bytes put_avro_value writes for row i
template <bool ARR>
__device__ __forceinline__ int64_t avro_value_len(const SinkParams& q, const RowsDev& r, int64_t i) {
  int64_t len = 5;
  for (int c = 0; c < q.n_val; c++) {
    if (ARR && q.varr[c] > 0) {
      Val v;
      int e = 0;
      for (; row_elem(q, r, i, c, e, v); e++) len += avro_val_len(q.vtype[c], v);
      len += e ? 2 + avro_varint_len((uint64_t)e << 1) : 2;
      continue;
    }
    len += avro_val_len(q.vtype[c], row_value_val(q, r, i, c));
  }
  return len;
}

struct LdsW {  // MemW into LDS: DS stores, not FLAT ones
  sk_lds_u8* p;
  __device__ __forceinline__ void put(uint8_t c) { *p++ = c; }
  __device__ __forceinline__ static LdsW at(uint32_t* stage, int64_t off) { return LdsW{(sk_lds_u8*)stage + off}; }
};

// ------------------------------------------------------------------ PROTOBUF values
//
// PROTOBUF / PROTOBUF_NOSR values (include/ksqldb_hip.h, "PROTOBUF values (sink)").  schema_id < 0 is
// the NOSR form (no framing); opt the `optional` representation.  A packed list's length prefix
// depends on its payload, so the measure pass sizes the payload first; the write pass sizes it
// again from the same elements.  A NULL element (null byte 2) has no protobuf form: the measure
// pass raises *bad and the host answers KHIP_E_UNSUPPORTED before anything is written.

// the varint of a sign-extended int32 / int64: 1..10 bytes
__device__ __forceinline__ int pb_val_len(int type, const Val& v) {
  return type == KHIP_TYPE_DOUBLE ? 8 : avro_varint_len((uint64_t)v.i);
}
__device__ __forceinline__ int pb_tag_len(int c) { return c + 1 < 16 ? 1 : 2; }  // field c + 1 <= 32
// a scalar is on the wire: non-NULL, and not the all-zero default unless the field has presence
__device__ __forceinline__ bool pb_present(const Val& v, int opt) { return !v.null && (opt || v.i != 0); }

template <class W>
__device__ __forceinline__ void put_pb_scalar(W& w, int type, const Val& v) {
  if (type == KHIP_TYPE_DOUBLE) {
#pragma unroll
    for (int b = 0; b < 8; b++) w.put((uint8_t)((uint64_t)v.i >> (8 * b)));
  } else {
    put_avro_varint(w, (uint64_t)v.i);
  }
}

// the payload bytes of row i's list in ARRAY column c; *cnt its length, *bad set on a NULL element
__device__ __forceinline__ int64_t pb_list_payload(const SinkParams& q, const RowsDev& r, int64_t i, int c, int* cnt,
                                                   bool* bad) {
  int64_t len = 0;
  Val v;
  int e = 0;
  for (; row_elem(q, r, i, c, e, v); e++) {
    if (v.null) *bad = true;
    len += pb_val_len(q.vtype[c], v);
  }
  *cnt = e;
  return len;
}

template <bool ARR>
__device__ __forceinline__ int64_t pb_value_len(const SinkParams& q, const RowsDev& r, int64_t i, int32_t schema_id,
                                                int opt, bool* bad) {
  int64_t len = schema_id >= 0 ? 6 : 0;
  for (int c = 0; c < q.n_val; c++) {
    if (ARR && q.varr[c] > 0) {
      int cnt;
      const int64_t pl = pb_list_payload(q, r, i, c, &cnt, bad);
      if (cnt) len += pb_tag_len(c) + avro_varint_len((uint64_t)pl) + pl;
      continue;
    }
    const Val v = row_value_val(q, r, i, c);
    if (pb_present(v, opt)) len += pb_tag_len(c) + pb_val_len(q.vtype[c], v);
  }
  return len;
}

// vpayload(c, &cnt): the payload bytes and length of the row's list in ARRAY column c
template <bool ARR, class W, class F, class P, class G>
__device__ __forceinline__ void put_pb_value(W& w, const SinkParams& q, int32_t schema_id, int opt, F&& vval,
                                             P&& vpayload, G&& velem) {
  if (schema_id >= 0) {
    w.put(0);
    put_be(w, (uint64_t)(uint32_t)schema_id, 4);
    w.put(0);  // the message-index list [0]
  }
  for (int i = 0; i < q.n_val; i++) {
    const uint32_t fld = (uint32_t)(i + 1) << 3;
    if (ARR && q.varr[i] > 0) {
      int cnt = 0;
      const int64_t pl = vpayload(i, &cnt);
      if (!cnt) continue;
      put_avro_varint(w, fld | 2);
      put_avro_varint(w, (uint64_t)pl);
      Val v;
      for (int e = 0; e < cnt && velem(i, e, v); e++) put_pb_scalar(w, q.vtype[i], v);
      continue;
    }
    const Val v = vval(i);
    if (!pb_present(v, opt)) continue;
    put_avro_varint(w, fld | (q.vtype[i] == KHIP_TYPE_DOUBLE ? 1u : 0u));
    put_pb_scalar(w, q.vtype[i], v);
  }
}

// ------------------------------------------------------------------ the value encoders
//
// One policy per format family; the three kernels below are templates over it.  A policy says
//   value_len<ARR>(m, q, r, i, &bad)  the bytes of row i's value (PROTOBUF: *bad on a NULL list element);
//   put<ARR>(w, q, r, i, vval)        the value through the writer w, vval(c) being scalar column c (the
//                                     list callbacks of the format are built here, from the rows);
//   StageW                            the writer of k_sink_write's LDS stage;
//   empty_ok                          a value that is not null may have no bytes;
//   parent_shape                      TextEnc only: two places where the text kernels' statements stand
//                                     in another order than the other formats', for no reason of the
//                                     format: the measure kernel's row sits in a loop of one round, and
//                                     k_sink_write tests the null value and loads the first columns
//                                     inside `if (in)`.  They stay because the compiler makes other
//                                     code without them (92 VGPRs for 95 and another descriptor in the
//                                     measure kernel; sink_json measured 0.9 % slower without both).
// The policy is a kernel argument of the write kernels, and its Measure one of the measure kernel:
// the measure kernels of the text and AVRO formats take no argument, PROTOBUF's takes three, and
// the kernels' argument bytes are to stay as they were, so Measure is a type of its own.

// A kernel argument of no bytes.  An empty struct takes one byte of the kernel's arguments and moves
// the hidden arguments behind it; a zero-length array member (a GNU extension that hipcc accepts)
// makes sizeof 0, and the launch then copies nothing for it.  Should a compiler refuse the member or
// give it a size, the static_assert below fails the build; nothing else depends on it.
struct NoArgs {
  int32_t none[0];
  __device__ __forceinline__ void raise() const {}
};

struct TextEnc : NoArgs {  // JSON / DELIMITED / KAFKA: put_value; the length is a counting run of it
  using Measure = NoArgs;
  using StageW = MemW;
  static constexpr bool empty_ok = false;
  static constexpr bool parent_shape = true;
  Measure measure(int32_t*) const { return {}; }
  template <bool ARR, class W, class F>
  __device__ __forceinline__ static void put(W& w, const SinkParams& q, const RowsDev& r, int64_t i, F&& vval) {
    put_value<ARR>(w, q, vval, [&](int c, int e, Val& v) { return row_elem(q, r, i, c, e, v); });
  }
  template <bool ARR>
  __device__ __forceinline__ static int64_t value_len(const Measure&, const SinkParams& q, const RowsDev& r, int64_t i,
                                                      bool*) {
    CountW w;
    put<ARR>(w, q, r, i, [&](int c) { return row_value_val(q, r, i, c); });
    return w.n;
  }
};
static_assert(sizeof(TextEnc) == 0, "no kernel argument bytes");

struct AvroEnc {
  int32_t schema_id;
  using Measure = NoArgs;
  using StageW = LdsW;
  static constexpr bool parent_shape = false;
  static constexpr bool empty_ok = false;
  Measure measure(int32_t*) const { return {}; }
  template <bool ARR, class W, class F>
  __device__ __forceinline__ void put(W& w, const SinkParams& q, const RowsDev& r, int64_t i, F&& vval) const {
    put_avro_value<ARR>(w, q, schema_id, vval, [&](int c) { return row_list_len(q, r, i, c); },
                        [&](int c, int e, Val& v) { return row_elem(q, r, i, c, e, v); });
  }
  template <bool ARR>
  __device__ __forceinline__ static int64_t value_len(const Measure&, const SinkParams& q, const RowsDev& r, int64_t i,
                                                      bool*) {
    return avro_value_len<ARR>(q, r, i);
  }
};

struct PbEnc {
  int32_t schema_id;  // < 0: PROTOBUF_NOSR
  int opt;
  struct Measure {
    int32_t schema_id;
    int opt;
    int32_t* bad;
    __device__ __forceinline__ void raise() const { atomicOr(bad, 1); }
  };
  using StageW = LdsW;
  static constexpr bool parent_shape = false;
  static constexpr bool empty_ok = true;  // NOSR: no framing, every column absent
  Measure measure(int32_t* bad) const { return {schema_id, opt, bad}; }
  template <bool ARR, class W, class F>
  __device__ __forceinline__ void put(W& w, const SinkParams& q, const RowsDev& r, int64_t i, F&& vval) const {
    put_pb_value<ARR>(w, q, schema_id, opt, vval,
                      [&](int c, int* cnt) {
                        bool bad = false;
                        return pb_list_payload(q, r, i, c, cnt, &bad);
                      },
                      [&](int c, int e, Val& v) { return row_elem(q, r, i, c, e, v); });
  }
  template <bool ARR>
  __device__ __forceinline__ static int64_t value_len(const Measure& m, const SinkParams& q, const RowsDev& r, int64_t i,
                                                      bool* bad) {
    return pb_value_len<ARR>(q, r, i, m.schema_id, m.opt, bad);
  }
};

// ------------------------------------------------------------------ the sink's kernels
//
// Three templates over the value encoder Enc.  ARR: the instantiation for sinks with an ARRAY
// column (k_sink_measure<Enc, true> and k_sink_write_arr<Enc>); a scalar sink's kernels
// (k_sink_measure<Enc, false>, k_sink_write<Enc>) carry none of it.

// Pass 1: each row's key / value length at klen / vlen[i + 1] (keys skipped when every key is kfix
// bytes), each tile's sums at tsum[1 + tile] (keys) and tsum[nT + 2 + tile] (values).
template <class Enc, bool ARR>
__global__ __launch_bounds__(256) void k_sink_measure(const SinkParams* __restrict__ qp, RowsDev r, int64_t n, int kfix,
                                                      int64_t nT, int64_t* __restrict__ klen, int64_t* __restrict__ vlen,
                                                      int64_t* __restrict__ tsum, typename Enc::Measure m) {
  __shared__ int64_t ws[2][4];
  const SinkParams& q = *qp;
  const int64_t i = (int64_t)blockIdx.x * SK_TILE + threadIdx.x;
  int64_t sk = 0, sv = 0;
  bool bad = false;
  auto row = [&] {
    if (!kfix) {
      CountW kw;
      encode_key_row(kw, q, r, i);
      klen[i + 1] = kw.n;
      sk += kw.n;
    }
    if (!value_is_null(q, r, i)) sv = Enc::template value_len<ARR>(m, q, r, i, &bad);
    vlen[i + 1] = sv;
  };
  if constexpr (Enc::parent_shape) {
#pragma unroll 1
    for (int u = 0; u < 1; u++) {
      if (i >= n) break;
      row();
    }
  } else if (i < n) {
    row();
  }
  if (ARR && bad) m.raise();
  sk_block_sum2(sk, sv, ws);
  if (threadIdx.x == 0) {
    tsum[1 + blockIdx.x] = sk;
    tsum[nT + 2 + blockIdx.x] = sv;
  }
}

// Pass 2 (after sk_scan made tsum the tiles' offsets).  Its rules, for both write kernels:
//   - every load of a row comes before its first global store (on gfx950 a load behind a store
//     waits for the store): the lengths in the offsets prologue, the first value columns in
//     SkFirst4, and the key's in put_key_words / encode_key_row before they store;
//   - the barriers (sk_block_scan2's, the stages') are uniform over the block: past-n threads run
//     them with lengths of 0;
//   - each row's end offsets go over its own length slots (koff / voff[i + 1]: only this thread
//     reads them, so no other tile's lengths are overwritten before they are read).
// The offsets prologue and the outputs at the end stand in both kernels as plain statements, not
// in helpers: moved into a function (a struct's constructor, a function with out-parameters, one
// taking the last stores as a callable, one for the key alone) they are allocated other registers throughout, the
// ARRAY writers of the text formats spill two more VGPRs, and those legs measured 2 to 4 % slower
// (profiles/sink_templates/README.md).

// The row's first four scalar value columns, loaded at once by load(); vval(c) for the encoders.
template <bool ARR>
struct SkFirst4 {
  const SinkParams& q;
  const RowsDev& r;
  const int64_t i;
  Val v0{0, nullptr, 0, true}, v1 = v0, v2 = v0, v3 = v0;
  __device__ __forceinline__ SkFirst4(const SinkParams& q_, const RowsDev& r_, int64_t i_) : q(q_), r(r_), i(i_) {}
  __device__ __forceinline__ void load() {
    if (q.n_val > 0 && !(ARR && q.varr[0])) v0 = row_value_val(q, r, i, 0);
    if (q.n_val > 1 && !(ARR && q.varr[1])) v1 = row_value_val(q, r, i, 1);
    if (q.n_val > 2 && !(ARR && q.varr[2])) v2 = row_value_val(q, r, i, 2);
    if (q.n_val > 3 && !(ARR && q.varr[3])) v3 = row_value_val(q, r, i, 3);
  }
  __device__ __forceinline__ Val operator()(int c) const {
    return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : c == 3 ? v3 : row_value_val(q, r, i, c);
  }
};

// Pass 2 of a scalar sink.  A wave whose 64 values take at most SK_WBUF bytes (one contiguous
// range of the output) encodes them into LDS at their places in that range and copies the range
// out in 16-byte stores (sk_wave_copy); a longer wave writes each value at its offset byte by byte.
template <class Enc>
__global__ KHIP_SINK_WRITE_LB void k_sink_write(const SinkParams* __restrict__ qp, RowsDev r, int64_t n, int kfix,
                                                int kwords, int64_t nT, const int64_t* __restrict__ tsum,
                                                int64_t* __restrict__ koff, uint8_t* __restrict__ kb,
                                                int64_t* __restrict__ voff, uint8_t* __restrict__ vb,
                                                uint8_t* __restrict__ vnull, Enc enc) {
  __shared__ int64_t ws[2][4];
  __shared__ uint32_t vst[4][SK_WBUF / 4 + 4];
  const SinkParams& q = *qp;
  const int wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * SK_TILE + threadIdx.x;
  const bool in = i < n;
  const int64_t kl = !in ? 0 : kfix ? kfix : koff[i + 1];
  const int64_t vl = in ? voff[i + 1] : 0;
  int64_t ko = kl, vo = vl, tk, tv;
  sk_block_scan2(ko, vo, tk, tv, ws);
  ko += kfix ? (int64_t)blockIdx.x * SK_TILE * kfix : tsum[blockIdx.x];
  vo += tsum[nT + 1 + blockIdx.x];
  const int64_t wbase = __shfl(vo, 0, 64), wlen = __shfl(vo + vl, 63, 64) - wbase;  // past-n lanes: vl 0
  const bool staged = wlen <= SK_WBUF;
  SkFirst4<false> vval(q, r, i);
  bool isnull = true;
  if constexpr (Enc::parent_shape) {
    if (in) {
      isnull = value_is_null(q, r, i);
      if (!isnull) vval.load();
    }
  } else {
    isnull = in ? value_is_null(q, r, i) : true;
    if (!isnull) vval.load();
  }
  if ((!Enc::parent_shape || in) && staged && !isnull && (!Enc::empty_ok || vl > 0)) {
    auto vw = Enc::StageW::at(vst[wave], vo - wbase);
    enc.template put<false>(vw, q, r, i, vval);
  }
  __syncthreads();
  if (staged && wlen > 0) sk_wave_copy((const uint8_t*)vst[wave], (int)wlen, vb + wbase);
  if (in) {
    if (kwords) {  // the key as kfix / 8 words
      put_key_words(q, r, i, (uint64_t*)(kb + ko));
    } else {
      MemW kw{kb + ko};
      encode_key_row(kw, q, r, i);
    }
    sk_st(vnull + i, (uint8_t)(isnull ? 1 : 0));
    if (!staged && !isnull && (!Enc::empty_ok || vl > 0)) {
      MemW vw{vb + vo};
      enc.template put<false>(vw, q, r, i, vval);
    }
    sk_st(koff + i + 1, ko + kl);
    sk_st(voff + i + 1, vo + vl);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    koff[0] = 0;
    voff[0] = 0;
  }
}

// Pass 2 of a sink with an ARRAY column: k_sink_write's offsets, keys and outputs, with another way
// for the values out.  A row with lists is long (64 rows pass SK_WBUF at 32 bytes each), so the
// stage is the tile's: the tile's values are one contiguous range of tv bytes, and the block goes
// over it in rounds of SK_ABUF bytes.  In a round every row that overlaps the round's window
// encodes itself through WinW, which keeps the bytes inside the window (a row across a window's
// edge encodes twice, each window taking its part), and the 256 threads copy the window out in
// 16-byte stores.  A round's element loads come while only LDS is written; the next round's wait
// once for the round's stores.  Rounds are uniform over the block (tv is), so the barriers are
// too.  32 KB of LDS: four blocks per CU, the four waves per SIMD the register cap gives.
template <class Enc>
__global__ KHIP_SINK_WRITE_LB void k_sink_write_arr(const SinkParams* __restrict__ qp, RowsDev r, int64_t n, int kfix,
                                                    int kwords, int64_t nT, const int64_t* __restrict__ tsum,
                                                    int64_t* __restrict__ koff, uint8_t* __restrict__ kb,
                                                    int64_t* __restrict__ voff, uint8_t* __restrict__ vb,
                                                    uint8_t* __restrict__ vnull, Enc enc) {
  __shared__ int64_t ws[2][4];
  __shared__ uint32_t ast[SK_ABUF / 4 + 4];
  const SinkParams& q = *qp;
  const int64_t i = (int64_t)blockIdx.x * SK_TILE + threadIdx.x;
  const bool in = i < n;
  const int64_t kl = !in ? 0 : kfix ? kfix : koff[i + 1];
  const int64_t vl = in ? voff[i + 1] : 0;
  int64_t ko = kl, vo = vl, tk, tv;
  sk_block_scan2(ko, vo, tk, tv, ws);
  ko += kfix ? (int64_t)blockIdx.x * SK_TILE * kfix : tsum[blockIdx.x];
  const int64_t tbase = tsum[nT + 1 + blockIdx.x];  // the tile's first value byte; vo: the row's, within the tile
  const bool isnull = in ? value_is_null(q, r, i) : true;
  SkFirst4<true> vval(q, r, i);
  if (!isnull) vval.load();
  const uint8_t* als = (const uint8_t*)ast;
  for (int64_t lo = 0; lo < tv; lo += SK_ABUF) {
    if (!isnull && vo < lo + SK_ABUF && vo + vl > lo) {
      WinW vw{(sk_lds_u8*)ast, vo - lo};
      enc.template put<true>(vw, q, r, i, vval);
    }
    __syncthreads();
    sk_range_copy<256>(als, (int)(tv - lo < SK_ABUF ? tv - lo : SK_ABUF), vb + tbase + lo, threadIdx.x);
    __syncthreads();
  }
  if (in) {
    if (kwords) {  // the key as kfix / 8 words
      put_key_words(q, r, i, (uint64_t*)(kb + ko));
    } else {
      MemW kw{kb + ko};
      encode_key_row(kw, q, r, i);
    }
    sk_st(vnull + i, (uint8_t)(isnull ? 1 : 0));
    sk_st(koff + i + 1, ko + kl);
    sk_st(voff + i + 1, tbase + vo + vl);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    koff[0] = 0;
    voff[0] = 0;
  }
}

// ------------------------------------------------------------------ GROUP BY columns → key bytes

struct KeySrcDev {
  const void* data[SK_MAX];
  const int64_t* off[SK_MAX];
  const uint8_t* bytes[SK_MAX];
  const uint8_t* valid[SK_MAX];
};

__device__ __forceinline__ Val src_key_val(const SinkParams& q, const KeySrcDev& k, int64_t i, int c) {
  Val v{0, nullptr, 0, false};
  v.null = !bit_get(k.valid[c], i);
  if (q.ktype[c] == KHIP_TYPE_STRING) {
    v.s = k.bytes[c] + k.off[c][i];
    v.len = k.off[c][i + 1] - k.off[c][i];
  } else if (q.ktype[c] == KHIP_TYPE_INT32) {
    v.i = ((const int32_t*)k.data[c])[i];
  } else {
    v.i = ((const int64_t*)k.data[c])[i];
  }
  return v;
}

__device__ __forceinline__ bool src_key_null(const SinkParams& q, const KeySrcDev& k, int64_t i) {
  for (int c = 0; c < q.n_key; c++)
    if (src_key_val(q, k, i, c).null) return true;
  return false;
}

__global__ __launch_bounds__(256) void k_key_measure(const SinkParams* __restrict__ qp, KeySrcDev k, int64_t n,
                                                     int64_t* __restrict__ klen, uint8_t* __restrict__ kvalid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const SinkParams& q = *qp;
  const bool ok = i < n && !src_key_null(q, k, i);
  const uint64_t b = __ballot(ok);
  if (i < n) {
    CountW w;
    if (ok) put_key(w, q, [&](int c) { return src_key_val(q, k, i, c); });
    klen[i + 1] = w.n;
  }
  // each wave writes its 64 rows' validity bits (8 bytes; the buffer is padded to whole waves)
  if ((threadIdx.x & 63) == 0 && i < n) *(uint64_t*)(kvalid + (i >> 3)) = b;
}

__global__ __launch_bounds__(256) void k_key_write(const SinkParams* __restrict__ qp, KeySrcDev k, int64_t n,
                                                   const int64_t* __restrict__ koff, uint8_t* __restrict__ kb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const SinkParams& q = *qp;
  if (koff[i + 1] == koff[i]) return;
  MemW w{kb + koff[i]};
  put_key(w, q, [&](int c) { return src_key_val(q, k, i, c); });
}

// ------------------------------------------------------------------ scan (lengths → offsets)

// v[1..n] lengths → v[0..n] exclusive offsets from 0, in place.  Block b scans items
// [b*S, (b+1)*S) of v[1..]: pass 1 block sums, pass 2 one block over the sums, pass 3 in-block
// scan plus the block's carry.
__device__ __forceinline__ int64_t sk_block_scan(int64_t x, int64_t* wsum, int64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t incl = x;
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t y = __shfl_up(incl, off, 64);
    if (lane >= off) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int64_t before = 0, tot = 0;
  for (int k = 0; k < SK_SCAN_T / 64; k++) {
    before += k < wave ? wsum[k] : 0;
    tot += wsum[k];
  }
  __syncthreads();
  *total = tot;
  return before + incl - x;  // exclusive
}

__global__ __launch_bounds__(SK_SCAN_T) void k_sk_scan1(const int64_t* __restrict__ v, int64_t n,
                                                        int64_t* __restrict__ bsum) {
  __shared__ int64_t wsum[SK_SCAN_T / 64];
  const int64_t base = (int64_t)blockIdx.x * SK_SCAN_T * SK_SCAN_I + (int64_t)threadIdx.x * SK_SCAN_I;
  int64_t s = 0;
  for (int u = 0; u < SK_SCAN_I; u++) s += base + u < n ? v[1 + base + u] : 0;
  int64_t tot;
  sk_block_scan(s, wsum, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SK_SCAN_T) void k_sk_scan2(int64_t* __restrict__ bsum, int64_t nb) {
  __shared__ int64_t wsum[SK_SCAN_T / 64];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += SK_SCAN_T) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t x = b < nb ? bsum[b] : 0;
    int64_t tot;
    const int64_t ex = sk_block_scan(x, wsum, &tot);
    if (b < nb) bsum[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(SK_SCAN_T) void k_sk_scan3(int64_t* __restrict__ v, int64_t n,
                                                        const int64_t* __restrict__ bsum) {
  __shared__ int64_t wsum[SK_SCAN_T / 64];
  const int64_t base = (int64_t)blockIdx.x * SK_SCAN_T * SK_SCAN_I + (int64_t)threadIdx.x * SK_SCAN_I;
  int64_t x[SK_SCAN_I], s = 0;
  for (int u = 0; u < SK_SCAN_I; u++) {
    x[u] = base + u < n ? v[1 + base + u] : 0;
    s += x[u];
  }
  int64_t tot;
  int64_t run = bsum[blockIdx.x] + sk_block_scan(s, wsum, &tot);
  for (int u = 0; u < SK_SCAN_I; u++) {
    run += x[u];
    if (base + u < n) v[1 + base + u] = run;  // inclusive at i + 1 = exclusive at i + 1
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) v[0] = 0;
}

}  // namespace khip

using namespace khip;

struct khip_sink {
  khip_sink_desc desc{};
  SinkParams q{};
  int device = 0;
  bool has_arr = false;        // some value column is an ARRAY: k_sink_measure<Enc, true> / k_sink_write_arr<Enc>
  int32_t schema_id = -1;      // AVRO / PROTOBUF values: the schema id of the records' header; -1 = not set yet
  bool pb = false;             // PROTOBUF / PROTOBUF_NOSR values: PbEnc
  int pb_opt = 0;              // KHIP_PROTO_OPTIONAL: scalars have presence
  DevBuf pb_bad;               // the measure pass's flag: some list holds a NULL element
  int32_t src_len[SK_MAX] = {};  // per rows column: its ARRAY length L, 0 = scalar
  hipStream_t stream = nullptr;
  DevBuf dq, bsum, bsum2, tsum, koff, kbytes, kvalid, voff, vbytes, vnull;
  DevBuf st_key, st_koff, st_kbytes, st_ws, st_we, st_tomb, st_col[SK_MAX], st_null[SK_MAX], st_cv[SK_MAX];
  std::vector<int64_t> h_koff;  // khip_sink_key of a host batch: the keys, in host memory
  std::vector<uint8_t> h_kbytes, h_kvalid;
};

namespace {

khip_status sk_stage(khip_sink* s, DevBuf& b, const void* src, size_t bytes, const void** dst) {
  if (!src) {
    *dst = nullptr;
    return KHIP_OK;
  }
  KHIP_TRY(b.ensure(std::max<size_t>(bytes, 8)));
  if (bytes) KHIP_TRY_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s->stream));
  *dst = b.p;
  return KHIP_OK;
}

// in place: off[1..n] lengths → off[0..n] offsets; returns the total (synchronises the stream)
// v[1..n] lengths → v[0..n] offsets, in place, on the stream (ws: the block sums); *total ← v[n]
// (a host copy: complete once the stream is synchronised, here when sync).
khip_status sk_scan(khip_sink* s, DevBuf& ws, int64_t* off, int64_t n, int64_t* total, bool sync = true) {
  const int64_t per = (int64_t)SK_SCAN_T * SK_SCAN_I;
  const int64_t nb = std::max<int64_t>(1, ceil_div(n, per));
  KHIP_TRY(ws.ensure((size_t)(nb + 1) * 8));
  int64_t* bs = ws.as<int64_t>();
  hipLaunchKernelGGL(k_sk_scan1, dim3(nb), dim3(SK_SCAN_T), 0, s->stream, off, n, bs);
  hipLaunchKernelGGL(k_sk_scan2, dim3(1), dim3(SK_SCAN_T), 0, s->stream, bs, nb);
  hipLaunchKernelGGL(k_sk_scan3, dim3(nb), dim3(SK_SCAN_T), 0, s->stream, off, n, bs);
  KHIP_TRY_HIP(hipGetLastError());
  KHIP_TRY_HIP(hipMemcpyAsync(total, bs + nb, 8, hipMemcpyDeviceToHost, s->stream));
  if (sync) KHIP_TRY_HIP(hipStreamSynchronize(s->stream));
  return KHIP_OK;
}

bool sk_type_ok(int t, bool str) {
  return t == KHIP_TYPE_INT32 || t == KHIP_TYPE_INT64 || t == KHIP_TYPE_DOUBLE || (str && t == KHIP_TYPE_STRING);
}

khip_status sk_set_schema_id(khip_sink* s, int32_t schema_id, std::initializer_list<int> formats, const char* whose) {
  clear_error();
  if (!s) return fail(KHIP_E_INVALID, "null argument");
  if (std::find(formats.begin(), formats.end(), s->q.value_format) == formats.end()) return fail(KHIP_E_INVALID, whose);
  if (schema_id < 0) return fail(KHIP_E_INVALID, "negative schema id");
  s->schema_id = schema_id;
  return KHIP_OK;
}

// f(enc) with the sink's value encoder: the one place that picks it
template <class F>
void sk_with_enc(const khip_sink* s, F&& f) {
  if (s->pb) f(PbEnc{s->q.value_format == KHIP_FMT_PROTOBUF ? s->schema_id : -1, s->pb_opt});  // NOSR: no framing
  else if (s->q.value_format == KHIP_FMT_AVRO) f(AvroEnc{s->schema_id});
  else f(TextEnc{});
}

// ---- khip_sink_encode's stages, in their order; SinkCall is what one hands to the next

struct SinkCall {
  int64_t n = 0, nT = 0;  // rows, tiles
  bool str_key = false, dev_out = false;
  int ncol = 0;       // rows columns up to the last one read
  int ctype[SK_MAX];
  bool used[SK_MAX];  // columns some value column reads: only those are staged or passed on
  RowsDev r{};
  int kfix = 0;       // every key this many bytes: a KAFKA INT32 / BIGINT key and its window suffix
  int64_t *koff = nullptr, *voff = nullptr;  // the offsets: the device outputs, else the handle's buffers
  int64_t ktot = 0, vtot = 0;
  uint8_t *kb = nullptr, *vb = nullptr, *vn = nullptr;  // likewise the bytes and the null flags
};

khip_status enc_check_args(khip_sink* s, const khip_sink_rows* rows, khip_sink_out* out, SinkCall& c) {
  const SinkParams& q = s->q;
  if (q.value_format == KHIP_FMT_AVRO && s->schema_id < 0)
    return fail(KHIP_E_STATE, "AVRO values need khip_sink_set_avro_schema_id first");
  if (q.value_format == KHIP_FMT_PROTOBUF && s->schema_id < 0)
    return fail(KHIP_E_STATE, "PROTOBUF values need khip_sink_set_schema_id first");
  const int64_t n = c.n = rows->n_rows;
  if (n < 0 || !out->key_offsets || !out->value_offsets || !out->value_null) return fail(KHIP_E_INVALID, "rows / outputs");
  const bool windowed = q.window_kind != KHIP_WINDOW_NONE;
  if (n && windowed && !rows->window_start) return fail(KHIP_E_INVALID, "a windowed key needs window_start");
  if (n && q.window_kind == KHIP_WINDOW_SESSION && !rows->window_end) return fail(KHIP_E_INVALID, "a session key needs window_end");
  c.str_key = rows->key_serialized || q.ktype[0] == KHIP_TYPE_STRING;
  if (!rows->key_serialized && (q.n_key != 1 || q.ktype[0] == KHIP_TYPE_DOUBLE))
    return fail(KHIP_E_INVALID, "row keys: one INT32/INT64/STRING key column, or serialized keys");
  if (n && (c.str_key ? !(rows->key_offsets && rows->key_bytes) : !rows->key_i64))
    return fail(KHIP_E_INVALID, "row key arrays");
  for (int k = 0; k < SK_MAX; k++) {
    c.ctype[k] = KHIP_TYPE_INT64;
    c.used[k] = false;
  }
  for (int k = 0; k < q.n_val; k++) {
    const int src = q.vsrc[k];
    if (src == KHIP_SINK_SRC_WS && n && !rows->window_start) return fail(KHIP_E_INVALID, "WINDOWSTART source");
    if (src == KHIP_SINK_SRC_WE && n && !rows->window_end) return fail(KHIP_E_INVALID, "WINDOWEND source");
    if (src >= 0) {
      if (n && (!rows->col_data || !rows->col_data[src])) return fail(KHIP_E_INVALID, "value source column");
      if (n && q.varr[k] && (!rows->col_null || !rows->col_null[src]))
        return fail(KHIP_E_INVALID, "an ARRAY value column needs col_null (the list's length lives in its null bytes)");
      c.ncol = std::max(c.ncol, src + 1);
      c.ctype[src] = q.vtype[k];
      c.used[src] = true;
    }
  }
  return KHIP_OK;
}

// c.r: the rows as the kernels read them; host rows are copied to the handle's staging buffers
khip_status enc_stage_rows(khip_sink* s, const khip_sink_rows* rows, SinkCall& c) {
  const int64_t n = c.n;
  RowsDev& r = c.r;
  r.key_serialized = rows->key_serialized;
  r.key_i64 = rows->key_i64;
  r.key_off = rows->key_offsets;
  r.key_bytes = rows->key_bytes;
  r.ws = rows->window_start;
  r.we = rows->window_end;
  r.tomb = rows->tombstone;
  for (int k = 0; k < c.ncol; k++) {
    r.col[k] = c.used[k] && rows->col_data ? rows->col_data[k] : nullptr;
    r.cnull[k] = c.used[k] && rows->col_null ? rows->col_null[k] : nullptr;
  }
  if (rows->mem == KHIP_MEM_HOST && n) {
    const void* p;
    if (c.str_key) {
      KHIP_TRY(sk_stage(s, s->st_koff, rows->key_offsets, (size_t)(n + 1) * 8, &p));
      r.key_off = (const int64_t*)p;
      KHIP_TRY(sk_stage(s, s->st_kbytes, rows->key_bytes, (size_t)rows->key_offsets[n], &p));
      r.key_bytes = (const uint8_t*)p;
    } else {
      KHIP_TRY(sk_stage(s, s->st_key, rows->key_i64, (size_t)n * 8, &p));
      r.key_i64 = (const int64_t*)p;
    }
    KHIP_TRY(sk_stage(s, s->st_ws, rows->window_start, (size_t)n * 8, &p));
    r.ws = (const int64_t*)p;
    KHIP_TRY(sk_stage(s, s->st_we, rows->window_end, (size_t)n * 8, &p));
    r.we = (const int64_t*)p;
    KHIP_TRY(sk_stage(s, s->st_tomb, rows->tombstone, (size_t)n, &p));
    r.tomb = (const uint8_t*)p;
    for (int k = 0; k < c.ncol; k++) {
      if (!c.used[k] || !rows->col_data[k]) continue;
      const size_t ne = (size_t)n * (size_t)std::max(s->src_len[k], 1);  // ARRAY: n x L elements and null bytes
      KHIP_TRY(sk_stage(s, s->st_col[k], rows->col_data[k], ne * (c.ctype[k] == KHIP_TYPE_INT32 ? 4 : 8), &p));
      r.col[k] = p;
      KHIP_TRY(sk_stage(s, s->st_null[k], rows->col_null ? rows->col_null[k] : nullptr, ne, &p));
      r.cnull[k] = (const uint8_t*)p;
    }
  } else if (rows->mem != KHIP_MEM_HOST && rows->mem != KHIP_MEM_DEVICE) {
    return fail(KHIP_E_INVALID, "rows mem");
  }
  return KHIP_OK;
}

// Pass 1 and the scans: the lengths at c.koff / c.voff become offsets, c.ktot / c.vtot the totals.
khip_status enc_measure(khip_sink* s, const khip_sink_rows* rows, khip_sink_out* out, SinkCall& c) {
  const SinkParams& q = s->q;
  const int64_t n = c.n;
  if (out->mem != KHIP_MEM_HOST && out->mem != KHIP_MEM_DEVICE) return fail(KHIP_E_INVALID, "output mem");
  c.dev_out = out->mem == KHIP_MEM_DEVICE;
  if (c.dev_out) {
    c.koff = out->key_offsets;
    c.voff = out->value_offsets;
  } else {
    KHIP_TRY(s->koff.ensure((size_t)(n + 1) * 8));
    KHIP_TRY(s->voff.ensure((size_t)(n + 1) * 8));
    c.koff = s->koff.as<int64_t>();
    c.voff = s->voff.as<int64_t>();
  }
  c.nT = ceil_div(n, SK_TILE);
  if (!rows->key_serialized && q.key_format == KHIP_FMT_KAFKA && q.ktype[0] != KHIP_TYPE_STRING)
    c.kfix = (q.ktype[0] == KHIP_TYPE_INT64 ? 8 : 4) +
             (q.window_kind == KHIP_WINDOW_SESSION ? 16 : q.window_kind != KHIP_WINDOW_NONE ? 8 : 0);
  if (!n) {
    const int64_t z = 0;
    if (c.dev_out) {
      KHIP_TRY_HIP(hipMemcpyAsync(c.koff, &z, 8, hipMemcpyHostToDevice, s->stream));
      KHIP_TRY_HIP(hipMemcpyAsync(c.voff, &z, 8, hipMemcpyHostToDevice, s->stream));
      KHIP_TRY_HIP(hipStreamSynchronize(s->stream));
    }
    return KHIP_OK;
  }
  KHIP_TRY(s->tsum.ensure((size_t)(2 * (c.nT + 1)) * 8));
  int64_t* ts = s->tsum.as<int64_t>();
  const bool may_be_bad = s->pb && s->has_arr;  // a NULL list element: PbEnc raises the flag
  if (s->pb) KHIP_TRY(s->pb_bad.ensure(8));
  if (may_be_bad) KHIP_TRY_HIP(hipMemsetAsync(s->pb_bad.p, 0, 8, s->stream));
  sk_with_enc(s, [&](auto enc) {
    using Enc = decltype(enc);
    hipLaunchKernelGGL((s->has_arr ? k_sink_measure<Enc, true> : k_sink_measure<Enc, false>), dim3((unsigned)c.nT),
                       dim3(256), 0, s->stream, s->dq.as<SinkParams>(), c.r, n, c.kfix, c.nT, c.koff, c.voff, ts,
                       enc.measure(s->pb_bad.as<int32_t>()));
  });
  KHIP_TRY_HIP(hipGetLastError());
  int64_t tk = 0, tv = 0;
  int32_t bad = 0;
  if (may_be_bad) KHIP_TRY_HIP(hipMemcpyAsync(&bad, s->pb_bad.p, 4, hipMemcpyDeviceToHost, s->stream));
  if (!c.kfix) KHIP_TRY(sk_scan(s, s->bsum, ts, c.nT, &tk, false));
  KHIP_TRY(sk_scan(s, s->bsum2, ts + c.nT + 1, c.nT, &tv, true));
  if (bad)
    return fail(KHIP_E_UNSUPPORTED, "a NULL array element has no PROTOBUF form (the query stays with the reference)");
  c.ktot = c.kfix ? (int64_t)c.kfix * n : tk;
  c.vtot = tv;
  return KHIP_OK;
}

// the totals to the caller; c.kb / c.vb / c.vn: where pass 2 writes
khip_status enc_out_buffers(khip_sink* s, khip_sink_out* out, SinkCall& c) {
  out->key_len = c.ktot;
  out->value_len = c.vtot;
  if (c.ktot > out->key_capacity || c.vtot > out->value_capacity) return fail(KHIP_E_BUFFER, "sink output capacity too small");
  if (c.n && (c.ktot && !out->key_bytes)) return fail(KHIP_E_INVALID, "key_bytes");
  if (c.n && (c.vtot && !out->value_bytes)) return fail(KHIP_E_INVALID, "value_bytes");
  c.kb = out->key_bytes;
  c.vb = out->value_bytes;
  c.vn = out->value_null;
  if (!c.dev_out) {
    KHIP_TRY(s->kbytes.ensure((size_t)std::max<int64_t>(c.ktot, 8)));
    KHIP_TRY(s->vbytes.ensure((size_t)std::max<int64_t>(c.vtot, 8)));
    KHIP_TRY(s->vnull.ensure((size_t)std::max<int64_t>(c.n, 8)));
    c.kb = s->kbytes.as<uint8_t>();
    c.vb = s->vbytes.as<uint8_t>();
    c.vn = s->vnull.as<uint8_t>();
  }
  return KHIP_OK;
}

// Pass 2
khip_status enc_write(khip_sink* s, const SinkCall& c) {
  if (!c.n) return KHIP_OK;
  const int kwords = c.kfix && s->q.ktype[0] == KHIP_TYPE_INT64 && ((uintptr_t)c.kb & 7) == 0 ? c.kfix / 8 : 0;
  sk_with_enc(s, [&](auto enc) {
    using Enc = decltype(enc);
    hipLaunchKernelGGL((s->has_arr ? k_sink_write_arr<Enc> : k_sink_write<Enc>), dim3((unsigned)c.nT), dim3(256), 0,
                       s->stream, s->dq.as<SinkParams>(), c.r, c.n, c.kfix, kwords, c.nT, s->tsum.as<int64_t>(), c.koff,
                       c.kb, c.voff, c.vb, c.vn, enc);
  });
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

// host outputs: the handle's buffers to the caller's; the call ends synchronised either way
khip_status enc_copy_out(khip_sink* s, khip_sink_out* out, const SinkCall& c) {
  if (!c.dev_out) {
    const int64_t n = c.n;
    KHIP_TRY_HIP(hipMemcpyAsync(out->key_offsets, c.koff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s->stream));
    KHIP_TRY_HIP(hipMemcpyAsync(out->value_offsets, c.voff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s->stream));
    if (n) KHIP_TRY_HIP(hipMemcpyAsync(out->value_null, c.vn, (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (c.ktot) KHIP_TRY_HIP(hipMemcpyAsync(out->key_bytes, c.kb, (size_t)c.ktot, hipMemcpyDeviceToHost, s->stream));
    if (c.vtot) KHIP_TRY_HIP(hipMemcpyAsync(out->value_bytes, c.vb, (size_t)c.vtot, hipMemcpyDeviceToHost, s->stream));
  }
  KHIP_TRY_HIP(hipStreamSynchronize(s->stream));
  return KHIP_OK;
}

}  // namespace

extern "C" {

khip_status khip_sink_create(const khip_sink_desc* d, khip_sink** out) {
  clear_error();
  if (!d || !out) return fail(KHIP_E_INVALID, "null argument");
  const int kf = d->key_format;
  int vf = d->value_format;
  const bool pb_opt = vf > 0 && (vf & KHIP_PROTO_OPTIONAL);
  if (pb_opt) vf &= ~KHIP_PROTO_OPTIONAL;
  const bool pb = vf == KHIP_FMT_PROTOBUF || vf == KHIP_FMT_PROTOBUF_NOSR;
  if (kf != KHIP_FMT_KAFKA && kf != KHIP_FMT_JSON && kf != KHIP_FMT_DELIMITED)
    return fail(KHIP_E_UNSUPPORTED, "sink key format (KAFKA, JSON, DELIMITED)");
  if (vf != KHIP_FMT_KAFKA && vf != KHIP_FMT_JSON && vf != KHIP_FMT_DELIMITED && vf != KHIP_FMT_AVRO && !pb)
    return fail(KHIP_E_UNSUPPORTED, "sink value format (KAFKA, JSON, DELIMITED, AVRO, PROTOBUF, PROTOBUF_NOSR)");
  if (pb_opt && !pb) return fail(KHIP_E_INVALID, "KHIP_PROTO_OPTIONAL belongs to the PROTOBUF value formats");
  if (d->n_key_cols < 1 || d->n_key_cols > SK_MAX || !d->key_types) return fail(KHIP_E_INVALID, "1..32 key columns");
  if (kf == KHIP_FMT_KAFKA && d->n_key_cols != 1)
    return fail(KHIP_E_UNSUPPORTED, "the KAFKA key format carries one column");
  if (d->n_value_cols < 0 || d->n_value_cols > SK_MAX || (d->n_value_cols && (!d->value_types || !d->value_src)))
    return fail(KHIP_E_INVALID, "0..32 value columns with types and sources");
  if (vf == KHIP_FMT_KAFKA && d->n_value_cols != 1) return fail(KHIP_E_UNSUPPORTED, "the KAFKA value format carries one column");
  if (d->window_kind < KHIP_WINDOW_NONE || d->window_kind > KHIP_WINDOW_SESSION) return fail(KHIP_E_INVALID, "window kind");
  khip_sink* s = new khip_sink();
  s->desc = *d;
  s->pb = pb;
  s->pb_opt = pb_opt ? 1 : 0;
  SinkParams& q = s->q;
  q.key_format = kf;
  q.value_format = vf;
  q.n_key = d->n_key_cols;
  q.n_val = d->n_value_cols;
  q.window_kind = d->window_kind;
  q.delim = d->delimiter ? d->delimiter : ',';
  auto name = [&](const char* const* names, int i, uint8_t* dst, int32_t* len) -> bool {
    const char* nm = names ? names[i] : nullptr;
    const size_t L = nm ? strlen(nm) : 0;
    if (!nm || L > SK_NAME) return false;
    memcpy(dst, nm, L);
    *len = (int32_t)L;
    return true;
  };
  for (int i = 0; i < q.n_key; i++) {
    q.ktype[i] = d->key_types[i];
    if (!sk_type_ok(q.ktype[i], true)) {
      delete s;
      return fail(KHIP_E_UNSUPPORTED, "key column type");
    }
    if (kf == KHIP_FMT_JSON && q.n_key > 1 && !name(d->key_names, i, q.kname[i], &q.kname_len[i])) {
      delete s;
      return fail(KHIP_E_INVALID, "JSON key column names (<= 64 bytes) required");
    }
  }
  int src_type[SK_MAX];
  for (int c = 0; c < SK_MAX; c++) src_type[c] = -1;
  for (int i = 0; i < q.n_val; i++) {
    if (d->value_types[i] < 0) {
      delete s;
      return fail(KHIP_E_INVALID, "value column type: negative KHIP_SINK_ARRAY bits");
    }
    q.vtype[i] = d->value_types[i] & 0xFFFF;
    q.varr[i] = d->value_types[i] >> 16;  // KHIP_SINK_ARRAY(L): 1..32767, 0 = scalar
    q.vsrc[i] = d->value_src[i];
    if (q.varr[i] && vf != KHIP_FMT_JSON && vf != KHIP_FMT_AVRO && !pb) {
      delete s;
      return fail(KHIP_E_INVALID, "an ARRAY value column needs the JSON or AVRO value format, or PROTOBUF / PROTOBUF_NOSR (KAFKA / DELIMITED carry no arrays)");
    }
    if (q.varr[i] && (q.vsrc[i] == KHIP_SINK_SRC_WS || q.vsrc[i] == KHIP_SINK_SRC_WE)) {
      delete s;
      return fail(KHIP_E_INVALID, "WINDOWSTART / WINDOWEND are scalar BIGINT columns, not ARRAYs");
    }
    if (!sk_type_ok(q.vtype[i], false) || q.vsrc[i] < KHIP_SINK_SRC_WE || q.vsrc[i] >= SK_MAX ||
        q.vsrc[i] == -1) {
      delete s;
      return fail(KHIP_E_INVALID, "value column type (INT32/INT64/DOUBLE) and source");
    }
    if (q.vsrc[i] < 0 && q.vtype[i] != KHIP_TYPE_INT64) {
      delete s;
      return fail(KHIP_E_INVALID, "WINDOWSTART / WINDOWEND are BIGINT");
    }
    if (q.vsrc[i] >= 0) {  // two readers of one rows column agree on its layout when one is an ARRAY
      const int c = q.vsrc[i];
      if (src_type[c] >= 0 && (s->src_len[c] || q.varr[i]) && (s->src_len[c] != q.varr[i] || src_type[c] != q.vtype[i])) {
        delete s;
        return fail(KHIP_E_INVALID, "value columns read rows column " + std::to_string(c) + " with different ARRAY lengths or types");
      }
      src_type[c] = q.vtype[i];
      s->src_len[c] = q.varr[i];
      s->has_arr |= q.varr[i] > 0;
    }
    if (vf == KHIP_FMT_JSON && !name(d->value_names, i, q.vname[i], &q.vname_len[i])) {
      delete s;
      return fail(KHIP_E_INVALID, "JSON value column names (<= 64 bytes) required");
    }
  }
  auto prefix = [](int i, const uint8_t* nm, int len, uint8_t* dst, int32_t* dlen) {
    HostW w{dst, 0, SK_PRE};
    w.put(i ? ',' : '{');
    put_json_str(w, nm, len);
    w.put(':');
    *dlen = w.n <= SK_PRE ? w.n : -1;
  };
  for (int i = 0; i < SK_MAX; i++) q.kpre_len[i] = q.vpre_len[i] = -1;
  if (kf == KHIP_FMT_JSON && q.n_key > 1)
    for (int i = 0; i < q.n_key; i++) prefix(i, q.kname[i], q.kname_len[i], q.kpre[i], &q.kpre_len[i]);
  if (vf == KHIP_FMT_JSON)
    for (int i = 0; i < q.n_val; i++) prefix(i, q.vname[i], q.vname_len[i], q.vpre[i], &q.vpre_len[i]);
  s->device = d->device;
  DeviceGuard g(s->device);
  if (hipStreamCreateWithFlags(&s->stream, hipStreamDefault) != hipSuccess) {
    delete s;
    return fail(KHIP_E_DEVICE, "hipStreamCreate failed (no device?)");
  }
  khip_status st = s->dq.ensure(sizeof(SinkParams));
  if (st == KHIP_OK && hipMemcpy(s->dq.p, &s->q, sizeof(SinkParams), hipMemcpyHostToDevice) != hipSuccess)
    st = fail(KHIP_E_DEVICE, "copying the sink parameters");
  if (st != KHIP_OK) {
    khip_sink_destroy(s);
    return st;
  }
  *out = s;
  return KHIP_OK;
}

khip_status khip_sink_set_avro_schema_id(khip_sink* s, int32_t schema_id) {
  return sk_set_schema_id(s, schema_id, {KHIP_FMT_AVRO}, "a schema id belongs to the AVRO value format");
}

khip_status khip_sink_set_schema_id(khip_sink* s, int32_t schema_id) {
  return sk_set_schema_id(s, schema_id, {KHIP_FMT_AVRO, KHIP_FMT_PROTOBUF},
                          "a schema id belongs to the AVRO and PROTOBUF value formats");
}

khip_status khip_sink_key(khip_sink* s, const khip_batch* in, const khip_key_col* cols, khip_batch* out) {
  clear_error();
  if (!s || !in || !cols || !out) return fail(KHIP_E_INVALID, "null argument");
  const SinkParams& q = s->q;
  const int64_t n = in->n_rows;
  if (n < 0) return fail(KHIP_E_INVALID, "batch rows");
  if (in->mem != KHIP_MEM_HOST && in->mem != KHIP_MEM_DEVICE) return fail(KHIP_E_INVALID, "batch mem");
  KeySrcDev k{};
  for (int c = 0; c < q.n_key; c++) {
    const bool str = q.ktype[c] == KHIP_TYPE_STRING;
    if (n && (str ? !(cols[c].offsets && cols[c].bytes) : !cols[c].data))
      return fail(KHIP_E_INVALID, "key column " + std::to_string(c) + " arrays");
    k.data[c] = cols[c].data;
    k.off[c] = cols[c].offsets;
    k.bytes[c] = cols[c].bytes;
    k.valid[c] = cols[c].valid;
  }
  DeviceGuard g(s->device);
  const size_t bm = (size_t)(n + 7) / 8;
  if (in->mem == KHIP_MEM_HOST && n) {
    const void* p;
    for (int c = 0; c < q.n_key; c++) {
      if (q.ktype[c] == KHIP_TYPE_STRING) {
        KHIP_TRY(sk_stage(s, s->st_col[c], cols[c].offsets, (size_t)(n + 1) * 8, &p));
        k.off[c] = (const int64_t*)p;
        KHIP_TRY(sk_stage(s, s->st_null[c], cols[c].bytes, (size_t)cols[c].offsets[n], &p));
        k.bytes[c] = (const uint8_t*)p;
      } else {
        KHIP_TRY(sk_stage(s, s->st_col[c], cols[c].data, (size_t)n * (q.ktype[c] == KHIP_TYPE_INT32 ? 4 : 8), &p));
        k.data[c] = p;
      }
      KHIP_TRY(sk_stage(s, s->st_cv[c], cols[c].valid, bm, &p));
      k.valid[c] = (const uint8_t*)p;
    }
  }
  KHIP_TRY(s->koff.ensure((size_t)(n + 1) * 8));
  KHIP_TRY(s->kvalid.ensure(((size_t)(n + 63) / 64) * 8 + 8));
  int64_t* koff = s->koff.as<int64_t>();
  int64_t total = 0;
  if (n) {
    hipLaunchKernelGGL(k_key_measure, dim3(ceil_div(n, 256)), dim3(256), 0, s->stream, s->dq.as<SinkParams>(), k, n, koff,
                       s->kvalid.as<uint8_t>());
    KHIP_TRY_HIP(hipGetLastError());
    KHIP_TRY(sk_scan(s, s->bsum, koff, n, &total));
    KHIP_TRY(s->kbytes.ensure((size_t)std::max<int64_t>(total, 8)));
    hipLaunchKernelGGL(k_key_write, dim3(ceil_div(n, 256)), dim3(256), 0, s->stream, s->dq.as<SinkParams>(), k, n, koff,
                       s->kbytes.as<uint8_t>());
    KHIP_TRY_HIP(hipGetLastError());
  } else {
    KHIP_TRY(s->kbytes.ensure(8));
    KHIP_TRY_HIP(hipMemsetAsync(koff, 0, 8, s->stream));
  }
  *out = *in;
  out->key_i64 = nullptr;
  if (in->mem == KHIP_MEM_HOST) {  // a host batch gets host keys (the rest stays the caller's)
    s->h_koff.resize((size_t)n + 1);
    s->h_kbytes.resize((size_t)std::max<int64_t>(total, 1));
    s->h_kvalid.resize(bm + 8);
    KHIP_TRY_HIP(hipMemcpyAsync(s->h_koff.data(), koff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s->stream));
    if (total) KHIP_TRY_HIP(hipMemcpyAsync(s->h_kbytes.data(), s->kbytes.p, (size_t)total, hipMemcpyDeviceToHost, s->stream));
    if (n) KHIP_TRY_HIP(hipMemcpyAsync(s->h_kvalid.data(), s->kvalid.p, bm, hipMemcpyDeviceToHost, s->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(s->stream));
    out->key_offsets = s->h_koff.data();
    out->key_bytes = s->h_kbytes.data();
    out->key_valid = s->h_kvalid.data();
    return KHIP_OK;
  }
  out->key_offsets = koff;
  out->key_bytes = s->kbytes.as<uint8_t>();
  out->key_valid = s->kvalid.as<uint8_t>();
  return KHIP_OK;
}

khip_status khip_sink_encode(khip_sink* s, const khip_sink_rows* rows, khip_sink_out* out) {
  clear_error();
  if (!s || !rows || !out) return fail(KHIP_E_INVALID, "null argument");
  SinkCall c;
  KHIP_TRY(enc_check_args(s, rows, out, c));
  DeviceGuard g(s->device);
  KHIP_TRY(enc_stage_rows(s, rows, c));
  KHIP_TRY(enc_measure(s, rows, out, c));
  KHIP_TRY(enc_out_buffers(s, out, c));
  KHIP_TRY(enc_write(s, c));
  return enc_copy_out(s, out, c);
}

khip_status khip_sink_sync(khip_sink* s) {
  clear_error();
  if (!s) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(s->device);
  KHIP_TRY_HIP(hipStreamSynchronize(s->stream));
  return KHIP_OK;
}

khip_status khip_sink_destroy(khip_sink* s) {
  if (!s) return KHIP_OK;
  DeviceGuard g(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  DevBuf* bufs[] = {&s->dq, &s->bsum, &s->bsum2, &s->tsum, &s->koff, &s->kbytes, &s->kvalid, &s->voff, &s->vbytes, &s->vnull, &s->st_key,
                    &s->st_koff, &s->st_kbytes, &s->st_ws, &s->st_we, &s->st_tomb, &s->pb_bad};
  for (DevBuf* b : bufs) b->release();
  for (int c = 0; c < SK_MAX; c++) {
    s->st_col[c].release();
    s->st_null[c].release();
    s->st_cv[c].release();
  }
  if (s->stream) hipStreamDestroy(s->stream);
  delete s;
  return KHIP_OK;
}

}  // extern "C"
