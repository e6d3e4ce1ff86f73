// khip_expr.hpp — what the host and the device share of the expression step (khip_expr_*, DESIGN.md
// "Expression step"): the Java scalar operations, the three-state value, the executor of one lowered
// instruction and the program checker that types a postfix program and lowers it.  Host and device;
// only the public header is needed (tools/expr_check.cpp builds it alone, without HIP).
//
// A value is 64 bits plus two flag bits.  INT and BIGINT values are both held sign-extended in the
// 64 bits, so INT -> BIGINT promotion costs nothing and only an INT result has to be wrapped back
// to 32 bits; a DOUBLE is its raw bits; a BOOLEAN is 0 or 1.  X_NULL: the SQL NULL.  X_ERR: the
// Java expression threw (a NullPointerException from unboxing, an ArithmeticException from an
// integer division by zero).  The flags are data: x_exec derives a result's flags from its operands'
// flags with selects.  The value helpers below (java_idiv, java_imod, d2i, d2l) do test their
// operands per row; on the device the compiler turns those tests into selects, and on the host they
// keep the undefined cases (x / 0, MIN / -1, an out-of-range conversion) from ever executing.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ksqldb_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KHIP_X_HD __host__ __device__ inline
#else
#define KHIP_X_HD inline
#endif

// DOUBLE a * b + c must stay two roundings (Java has no fused multiply-add in an expression).  The
// executor below runs one operation per instruction, which leaves nothing to fuse; the pragma and
// the Makefile's -ffp-contract=off for khip_expr.hip keep that true whatever gets inlined.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace khip {
namespace expr {

constexpr int X_MAX_CODE = 64;   // program words
constexpr int X_MAX_STACK = 8;   // operand stack depth
constexpr int X_MAX_OUT = 32;    // OUT columns
constexpr int X_MAX_COLS = 64;   // input columns
constexpr int X_MAX_LINS = 128;  // lowered instructions: one per word plus at most one promotion
constexpr int X_T_BOOL = 4;      // the internal BOOLEAN (KHIP_TYPE_* are 0..3)

constexpr uint32_t X_NULL = 1, X_ERR = 2;

// comparison kinds (L_CMP_*'s arg)
enum { X_EQ = 0, X_NE, X_LT, X_LE, X_GT, X_GE, X_DISTINCT };

// Lowered instructions: typed, promotions explicit, the stack slot resolved.
enum LOp : int32_t {
  L_COL32 = 0,  // push column arg (int32 elements)
  L_COL64,      // push column arg (8-byte elements: BIGINT or DOUBLE bits)
  L_COLV,       // push column arg's validity only (STRING)
  L_CONST,      // push imm
  L_ADD_I, L_SUB_I, L_MUL_I, L_DIV_I, L_MOD_I,  // arg 1: INT (wrap to 32 bits), 0: BIGINT
  L_ADD_F, L_SUB_F, L_MUL_F, L_DIV_F, L_MOD_F,
  L_CMP_I, L_CMP_F,                             // arg: comparison kind
  L_AND, L_OR,
  L_NEG_I, L_NEG_F,                             // (unary from here)
  L_L2D,   // integer -> DOUBLE of the slot named (a cast, or the promotion of either operand)
  L_D2I, L_D2L, L_L2I,
  L_NOT, L_ISNULL, L_ISNOTNULL,
  L_WHERE, L_OUT, L_KEY,                        // sinks; L_OUT's arg: column | type << 8
};

KHIP_X_HD bool l_is_push(int op) { return op <= L_CONST; }
KHIP_X_HD bool l_is_binary(int op) { return op >= L_ADD_I && op <= L_OR; }
KHIP_X_HD bool l_is_sink(int op) { return op >= L_WHERE; }

struct LIns {
  int32_t op, arg;
  int32_t slot;  // push: the new top; unary / sink: the operand; binary: the left operand (right = slot + 1)
  int32_t pad;
  int64_t imm;
};

struct Val {
  uint64_t v;
  uint32_t f;
};

// ------------------------------------------------------------------ Java scalar operations

KHIP_X_HD double x_f64(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}
KHIP_X_HD uint64_t x_bits(double d) {
  uint64_t b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}
KHIP_X_HD uint64_t x_sext32(uint64_t v) { return (uint64_t)(int64_t)(int32_t)(uint32_t)v; }

// Java / and % on int (T = int32_t) and long (int64_t): truncating, MIN / -1 = MIN, x % -1 = 0; a
// zero divisor sets *err and the division is not executed.
template <class T>
KHIP_X_HD T java_idiv(T a, T b, bool* err) {
  if (b == 0) {
    *err = true;
    return 0;
  }
  if (b == (T)-1) {
    if (sizeof(T) == 4) return (T)(int32_t)(0u - (uint32_t)a);
    return (T)(int64_t)(0ull - (uint64_t)a);
  }
  return a / b;
}
template <class T>
KHIP_X_HD T java_imod(T a, T b, bool* err) {
  if (b == 0) {
    *err = true;
    return 0;
  }
  if (b == (T)-1) return 0;
  return a % b;
}

// Java (int) d and (long) d: NaN -> 0, out of range -> MIN / MAX, otherwise toward zero.
KHIP_X_HD int32_t d2i(double d) {
  if (d != d) return 0;
  if (d >= 2147483647.0) return INT32_MAX;
  if (d <= -2147483648.0) return INT32_MIN;
  return (int32_t)d;
}
KHIP_X_HD int64_t d2l(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}

// The generated comparison of two promoted primitives (SqlToJavaVisitor.visitScalarComparisonExpression).
template <class T>
KHIP_X_HD bool x_cmp(int kind, T a, T b) {
  switch (kind) {
    case X_EQ: return (a <= b) && (a >= b);
    case X_NE:
    case X_DISTINCT: return (a < b) || (a > b);
    case X_LT: return a < b;
    case X_LE: return a <= b;
    case X_GT: return a > b;
    default: return a >= b;
  }
}

// One lowered non-push, non-sink instruction over its operand(s): b is read by binary ones only.
// op and arg are uniform over a launch: on the device the switch is a scalar branch.
KHIP_X_HD Val x_exec(int op, int arg, Val a, Val b) {
  const bool aN = a.f & X_NULL, aE = a.f & X_ERR, bN = b.f & X_NULL, bE = b.f & X_ERR;
  Val r;
  r.v = 0;
  r.f = 0;
  switch (op) {
    // arithmetic unboxes: a NULL operand throws
    case L_ADD_I: r.v = a.v + b.v; break;
    case L_SUB_I: r.v = a.v - b.v; break;
    case L_MUL_I: r.v = a.v * b.v; break;
    case L_DIV_I:
    case L_MOD_I: {
      bool z = false;
      if (arg) {
        const int32_t x = (int32_t)(uint32_t)a.v, y = (int32_t)(uint32_t)b.v;
        r.v = (uint64_t)(int64_t)(op == L_DIV_I ? java_idiv<int32_t>(x, y, &z) : java_imod<int32_t>(x, y, &z));
      } else {
        const int64_t x = (int64_t)a.v, y = (int64_t)b.v;
        r.v = (uint64_t)(op == L_DIV_I ? java_idiv<int64_t>(x, y, &z) : java_imod<int64_t>(x, y, &z));
      }
      if (z) r.f = X_ERR;
      break;
    }
    case L_ADD_F: r.v = x_bits(x_f64(a.v) + x_f64(b.v)); break;
    case L_SUB_F: r.v = x_bits(x_f64(a.v) - x_f64(b.v)); break;
    case L_MUL_F: r.v = x_bits(x_f64(a.v) * x_f64(b.v)); break;
    case L_DIV_F: r.v = x_bits(x_f64(a.v) / x_f64(b.v)); break;
    case L_MOD_F: r.v = x_bits(fmod(x_f64(a.v), x_f64(b.v))); break;
    case L_NEG_I: r.v = 0ull - a.v; break;
    case L_NEG_F: r.v = a.v ^ 0x8000000000000000ull; break;
    // casts are null-safe: the flags pass
    case L_L2D: r.v = x_bits((double)(int64_t)a.v); r.f = a.f; return r;
    case L_D2I: r.v = (uint64_t)(int64_t)d2i(x_f64(a.v)); r.f = a.f; return r;
    case L_D2L: r.v = (uint64_t)d2l(x_f64(a.v)); r.f = a.f; return r;
    case L_L2I: r.v = x_sext32(a.v); r.f = a.f; return r;
    case L_CMP_I:
    case L_CMP_F: {
      const bool c = op == L_CMP_I ? x_cmp<int64_t>(arg, (int64_t)a.v, (int64_t)b.v)
                                   : x_cmp<double>(arg, x_f64(a.v), x_f64(b.v));
      if (arg == X_DISTINCT) {
        // (L == null || R == null) ? ((L == null) ^ (R == null)) : (L < R || L > R): both sides
        // are evaluated on every path, so either one's exception propagates
        r.f = (aE || bE) ? X_ERR : 0;
        r.v = (aN || bN) ? (uint64_t)(aN != bN) : (uint64_t)c;
      } else {
        // (L == null || R == null) ? false : cmp: a NULL left short-circuits past the right side
        r.f = (aE || (!aN && bE)) ? X_ERR : 0;
        r.v = (aN || bN) ? 0 : (uint64_t)c;
      }
      return r;
    }
    case L_AND: r.f = (aE || (a.v && bE)) ? X_ERR : 0; r.v = a.v & b.v & 1; return r;
    case L_OR: r.f = (aE || (!a.v && bE)) ? X_ERR : 0; r.v = (a.v | b.v) & 1; return r;
    case L_NOT: r.v = a.v ^ 1; r.f = a.f; return r;
    case L_ISNULL: r.v = aN; r.f = a.f & X_ERR; return r;
    case L_ISNOTNULL: r.v = !aN; r.f = a.f & X_ERR; return r;
    default: return a;
  }
  // the arithmetic tail: INT results wrap to 32 bits; any NULL or ERROR operand is an ERROR
  if ((op <= L_MOD_I || op == L_NEG_I) && arg) r.v = x_sext32(r.v);
  const bool two = l_is_binary(op);
  if (a.f || (two && b.f)) r.f = X_ERR;
  return r;
}

// ------------------------------------------------------------------ the program checker

struct Program {
  LIns ins[X_MAX_LINS];
  int n_ins = 0;
  int n_out = 0;
  int out_type[X_MAX_OUT] = {};
  bool has_where = false, has_key = false;
  int where_end = 0;  // one past the L_WHERE (the keep pass runs [0, where_end))
  int start2 = 0;     // the output pass runs [start2, n_ins): where_end when the stack is empty there
  int max_col = -1;   // largest column index named
  uint64_t used = 0;  // columns named
};

inline bool x_numeric(int t) { return t == KHIP_TYPE_INT32 || t == KHIP_TYPE_INT64 || t == KHIP_TYPE_DOUBLE; }
inline int x_promote(int a, int b) {
  if (a == KHIP_TYPE_DOUBLE || b == KHIP_TYPE_DOUBLE) return KHIP_TYPE_DOUBLE;
  if (a == KHIP_TYPE_INT64 || b == KHIP_TYPE_INT64) return KHIP_TYPE_INT64;
  return KHIP_TYPE_INT32;
}

// Types the postfix program and lowers it.  Returns KHIP_OK, KHIP_E_INVALID or KHIP_E_UNSUPPORTED;
// *msg then points at a static text.
inline khip_status x_compile(int32_t n_cols, const int32_t* col_types, const int64_t* code, int32_t n_code,
                             Program* p, const char** msg) {
#define X_FAIL(st, text) \
  do {                   \
    *msg = text;         \
    return st;           \
  } while (0)
  *msg = "";
  *p = Program();
  if (n_cols < 0 || (n_cols && !col_types)) X_FAIL(KHIP_E_INVALID, "column types missing");
  if (n_cols > X_MAX_COLS) X_FAIL(KHIP_E_UNSUPPORTED, "more than 64 input columns");
  for (int c = 0; c < n_cols; c++)
    if (col_types[c] < KHIP_TYPE_INT32 || col_types[c] > KHIP_TYPE_STRING) X_FAIL(KHIP_E_INVALID, "unknown column type");
  if (n_code <= 0 || !code) X_FAIL(KHIP_E_INVALID, "empty program");
  if (n_code > X_MAX_CODE) X_FAIL(KHIP_E_UNSUPPORTED, "more than 64 instruction words");
  int st[X_MAX_STACK];
  int sp = 0;
  bool any_sink = false;
  auto emit = [&](int op, int arg, int slot, int64_t imm) {
    LIns& i = p->ins[p->n_ins++];
    i.op = op;
    i.arg = arg;
    i.slot = slot;
    i.pad = 0;
    i.imm = imm;
  };
  for (int pc = 0; pc < n_code; pc++) {
    const int64_t w = code[pc];
    const int op = (int)(w & 0xff);
    if (op >= KHIP_X_COL && op <= KHIP_X_CONST_F64) {  // pushes
      if (sp == X_MAX_STACK) X_FAIL(KHIP_E_UNSUPPORTED, "operand stack deeper than 8");
      if (op == KHIP_X_COL) {
        const int64_t c = w >> 32;
        if (c < 0 || c >= n_cols) X_FAIL(KHIP_E_INVALID, "column index out of range");
        const int t = col_types[c];
        emit(t == KHIP_TYPE_INT32 ? L_COL32 : t == KHIP_TYPE_STRING ? L_COLV : L_COL64, (int)c, sp, 0);
        if ((int)c > p->max_col) p->max_col = (int)c;
        p->used |= 1ull << c;
        st[sp++] = t;
      } else {
        if (pc + 1 >= n_code) X_FAIL(KHIP_E_INVALID, "truncated constant");
        const int64_t k = code[++pc];
        emit(L_CONST, 0, sp, op == KHIP_X_CONST_I32 ? (int64_t)(int32_t)(uint32_t)(uint64_t)k : k);
        st[sp++] = op == KHIP_X_CONST_I32 ? KHIP_TYPE_INT32 : op == KHIP_X_CONST_I64 ? KHIP_TYPE_INT64 : KHIP_TYPE_DOUBLE;
      }
      continue;
    }
    const bool arith = op >= KHIP_X_ADD && op <= KHIP_X_MOD, cmp = op >= KHIP_X_EQ && op <= KHIP_X_DISTINCT;
    const bool logic = op == KHIP_X_AND || op == KHIP_X_OR;
    if (arith || cmp || logic) {
      if (sp < 2) X_FAIL(KHIP_E_INVALID, "stack underflow");
      const int a = st[sp - 2], b = st[sp - 1], s = sp - 2;
      if (logic) {
        if (a != X_T_BOOL || b != X_T_BOOL) X_FAIL(KHIP_E_INVALID, "type error: AND / OR need BOOLEAN operands");
        emit(op == KHIP_X_AND ? L_AND : L_OR, 0, s, 0);
        st[s] = X_T_BOOL;
      } else {
        if (!x_numeric(a) || !x_numeric(b)) X_FAIL(KHIP_E_INVALID, "type error: numeric operands needed");
        const int t = x_promote(a, b);
        if (t == KHIP_TYPE_DOUBLE) {
          if (a != KHIP_TYPE_DOUBLE) emit(L_L2D, 0, s, 0);
          if (b != KHIP_TYPE_DOUBLE) emit(L_L2D, 0, s + 1, 0);
        }
        const bool f = t == KHIP_TYPE_DOUBLE;
        if (arith) {
          emit((f ? L_ADD_F : L_ADD_I) + (op - KHIP_X_ADD), t == KHIP_TYPE_INT32, s, 0);
          st[s] = t;
        } else {
          emit(f ? L_CMP_F : L_CMP_I, op - KHIP_X_EQ, s, 0);
          st[s] = X_T_BOOL;
        }
      }
      sp--;
      continue;
    }
    // everything else pops one value
    const bool known = op == KHIP_X_NEG || (op >= KHIP_X_CAST_I32 && op <= KHIP_X_CAST_F64) || op == KHIP_X_NOT ||
                       op == KHIP_X_IS_NULL || op == KHIP_X_IS_NOT_NULL || (op >= KHIP_X_WHERE && op <= KHIP_X_KEY);
    if (!known) X_FAIL(KHIP_E_INVALID, "unknown opcode");
    if (sp < 1) X_FAIL(KHIP_E_INVALID, "stack underflow");
    const int a = st[sp - 1], s = sp - 1;
    switch (op) {
      case KHIP_X_NEG:
        if (!x_numeric(a)) X_FAIL(KHIP_E_INVALID, "type error: NEG needs a numeric operand");
        emit(a == KHIP_TYPE_DOUBLE ? L_NEG_F : L_NEG_I, a == KHIP_TYPE_INT32, s, 0);
        break;
      case KHIP_X_CAST_I32:
      case KHIP_X_CAST_I64:
      case KHIP_X_CAST_F64: {
        if (!x_numeric(a)) X_FAIL(KHIP_E_INVALID, "type error: a cast needs a numeric operand");
        const int t = op == KHIP_X_CAST_I32 ? KHIP_TYPE_INT32 : op == KHIP_X_CAST_I64 ? KHIP_TYPE_INT64 : KHIP_TYPE_DOUBLE;
        if (t == KHIP_TYPE_DOUBLE && a != KHIP_TYPE_DOUBLE) emit(L_L2D, 0, s, 0);
        if (t == KHIP_TYPE_INT32 && a == KHIP_TYPE_INT64) emit(L_L2I, 0, s, 0);
        if (t == KHIP_TYPE_INT32 && a == KHIP_TYPE_DOUBLE) emit(L_D2I, 0, s, 0);
        if (t == KHIP_TYPE_INT64 && a == KHIP_TYPE_DOUBLE) emit(L_D2L, 0, s, 0);
        st[s] = t;  // INT -> BIGINT: the sign-extended value already is the BIGINT
        break;
      }
      case KHIP_X_NOT:
        if (a != X_T_BOOL) X_FAIL(KHIP_E_INVALID, "type error: NOT needs a BOOLEAN operand");
        emit(L_NOT, 0, s, 0);
        break;
      case KHIP_X_IS_NULL:
      case KHIP_X_IS_NOT_NULL:
        // a STRING is legal here alone, and then only as a bare column: nothing else yields one
        if (!x_numeric(a) && a != KHIP_TYPE_STRING) X_FAIL(KHIP_E_INVALID, "type error: IS [NOT] NULL of a BOOLEAN");
        emit(op == KHIP_X_IS_NULL ? L_ISNULL : L_ISNOTNULL, 0, s, 0);
        st[s] = X_T_BOOL;
        break;
      case KHIP_X_WHERE:
        if (any_sink) X_FAIL(KHIP_E_INVALID, "at most one WHERE, and it must be the program's first sink");
        if (a != X_T_BOOL) X_FAIL(KHIP_E_INVALID, "type error: WHERE needs a BOOLEAN");
        emit(L_WHERE, 0, s, 0);
        p->has_where = true;
        p->where_end = p->n_ins;
        p->start2 = s == 0 ? p->n_ins : 0;
        break;
      case KHIP_X_OUT:
        if (!x_numeric(a)) X_FAIL(KHIP_E_INVALID, "type error: OUT needs a numeric value");
        if (p->n_out == X_MAX_OUT) X_FAIL(KHIP_E_UNSUPPORTED, "more than 32 OUT columns");
        emit(L_OUT, p->n_out | (a << 8), s, 0);
        p->out_type[p->n_out++] = a;
        break;
      default:  // KHIP_X_KEY
        if (p->has_key) X_FAIL(KHIP_E_INVALID, "a second KEY");
        if (a != KHIP_TYPE_INT32 && a != KHIP_TYPE_INT64) X_FAIL(KHIP_E_INVALID, "type error: KEY needs an INT or BIGINT");
        emit(L_KEY, 0, s, 0);
        p->has_key = true;
        break;
    }
    if (op >= KHIP_X_WHERE) {
      any_sink = true;
      sp--;
    }
  }
  if (sp != 0) X_FAIL(KHIP_E_INVALID, "values left on the stack at the end of the program");
#undef X_FAIL
  return KHIP_OK;
}

// ------------------------------------------------------------------ host interpreter (one row)

// What the sinks of one row saw, for tools/expr_check.cpp: the device kernels run the same lowered
// instructions through x_exec, with the stack in LDS.
struct RowResult {
  bool keep = true;     // no WHERE: true
  uint32_t where_f = 0;
  Val out[X_MAX_OUT];
  Val key;
  int n_errors = 0;     // (sink) evaluations that ended in ERROR; OUT / KEY only when the row is kept
};

// cols[c]: the row's value of column c (sign-extended INT, BIGINT, or DOUBLE bits); nulls bit c: NULL.
inline void x_eval_row(const Program& p, const uint64_t* cols, uint64_t nulls, RowResult* r) {
  Val st[X_MAX_STACK + 1];
  *r = RowResult();
  for (int pc = 0; pc < p.n_ins; pc++) {
    const LIns& i = p.ins[pc];
    if (l_is_push(i.op)) {
      Val v;
      v.v = i.op == L_CONST ? (uint64_t)i.imm : i.op == L_COLV ? 0 : cols[i.arg];
      v.f = i.op != L_CONST && ((nulls >> i.arg) & 1) ? X_NULL : 0;
      if (v.f) v.v = 0;
      st[i.slot] = v;
    } else if (!l_is_sink(i.op)) {
      Val b;
      b.v = 0;
      b.f = 0;
      if (l_is_binary(i.op)) b = st[i.slot + 1];
      st[i.slot] = x_exec(i.op, i.arg, st[i.slot], b);
    } else {
      const Val v = st[i.slot];
      if (i.op == L_WHERE) {
        r->where_f = v.f;
        r->keep = !(v.f & X_ERR) && v.v;
        if (v.f & X_ERR) r->n_errors++;
        if (!r->keep) return;  // the projection never sees a filtered row
      } else {
        if (v.f & X_ERR) r->n_errors++;
        if (i.op == L_OUT) r->out[i.arg & 0xff] = v;
        else r->key = v;
      }
    }
  }
}

}  // namespace expr
}  // namespace khip
