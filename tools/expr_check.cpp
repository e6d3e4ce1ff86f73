// CPU check of ksql_amd/csrc/khip_expr.hpp (test infrastructure; tests/test_expr_helpers.py builds it
// plainly and with -fsanitize=address,undefined).
//
//   expr_check selftest     a table of edge vectors through the scalar helpers (java_idiv, java_imod,
//                           d2i, d2l, x_cmp) and through whole programs run by the host interpreter;
//                           exit 1 and a line per mismatch.
//   expr_check              reads lines:
//     P <n_cols> <type>... <n_code> <word>...   type-check and lower a program; prints
//                                                "P <status> <n_out> <has_where> <has_key> <message>"
//     R <null mask> <value>...                  one row through the last program (values: the columns'
//                                                64 bits as signed decimals); prints
//                                                "R <keep> <n_errors> <flags value>... " for every OUT,
//                                                then the KEY's (flags 1: NULL, 2: ERROR; value unsigned)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ksql_amd/csrc/khip_expr.hpp"

using namespace khip::expr;

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                            \
    }                                                        \
  } while (0)

static int64_t col(int c) { return KHIP_X_COL | ((int64_t)c << 32); }

// One row through a program: OUT 0 (or the WHERE's keep as value) and the error count.
struct One {
  Val v;
  bool keep;
  int errors;
};
static One run(const std::vector<int32_t>& types, const std::vector<int64_t>& code, const std::vector<uint64_t>& vals,
               uint64_t nulls) {
  Program p;
  const char* msg = "";
  const khip_status st = x_compile((int32_t)types.size(), types.data(), code.data(), (int32_t)code.size(), &p, &msg);
  if (st != KHIP_OK) {
    std::printf("FAIL compile: %s\n", msg);
    failures++;
    return One{};
  }
  RowResult r;
  x_eval_row(p, vals.data(), nulls, &r);
  One o;
  o.v = r.out[0];
  o.keep = r.keep;
  o.errors = r.n_errors;
  return o;
}

static int selftest() {
  bool e = false;
  // helpers
  CHECK(java_idiv<int32_t>(INT32_MIN, -1, &e) == INT32_MIN && !e);
  CHECK(java_idiv<int64_t>(INT64_MIN, -1, &e) == INT64_MIN && !e);
  CHECK(java_imod<int32_t>(INT32_MIN, -1, &e) == 0 && !e);
  CHECK(java_imod<int64_t>(INT64_MIN, -1, &e) == 0 && !e);
  CHECK(java_idiv<int32_t>(-7, 2, &e) == -3 && java_imod<int32_t>(-7, 2, &e) == -1 && java_imod<int64_t>(7, -2, &e) == 1);
  CHECK(!e);
  for (int64_t a : {(int64_t)0, (int64_t)1, (int64_t)-1, INT64_MIN, INT64_MAX}) {
    bool z = false;
    CHECK(java_idiv<int64_t>(a, 0, &z) == 0 && z);
    z = false;
    CHECK(java_imod<int64_t>(a, 0, &z) == 0 && z);
    z = false;
    CHECK(java_idiv<int32_t>((int32_t)a, 0, &z) == 0 && z);
    z = false;
    CHECK(java_imod<int32_t>((int32_t)a, 0, &z) == 0 && z);
  }
  const double inf = INFINITY, nan = NAN;
  CHECK(d2i(nan) == 0 && d2i(inf) == INT32_MAX && d2i(-inf) == INT32_MIN);
  CHECK(d2i(2147483648.0) == INT32_MAX && d2i(-2147483648.0) == INT32_MIN && d2i(2147483647.5) == INT32_MAX);
  CHECK(d2i(-2147483649.5) == INT32_MIN && d2i(9223372036854775808.0) == INT32_MAX && d2i(-1.9) == -1 && d2i(1.9) == 1);
  CHECK(d2l(nan) == 0 && d2l(inf) == INT64_MAX && d2l(-inf) == INT64_MIN);
  CHECK(d2l(9223372036854775808.0) == INT64_MAX && d2l(-9223372036854775808.0) == INT64_MIN);
  CHECK(d2l(9223372036854774784.0) == 9223372036854774784LL && d2l(2147483648.0) == 2147483648LL && d2l(-1.9) == -1);
  for (int k = X_EQ; k <= X_DISTINCT; k++) {
    CHECK(!x_cmp<double>(k, nan, 1.0) && !x_cmp<double>(k, 1.0, nan) && !x_cmp<double>(k, nan, nan));
  }
  CHECK(x_cmp<double>(X_EQ, -0.0, 0.0) && !x_cmp<double>(X_NE, -0.0, 0.0));
  // programs
  const int32_t I = KHIP_TYPE_INT32, L = KHIP_TYPE_INT64, D = KHIP_TYPE_DOUBLE;
  One o = run({I, I}, {col(0), col(1), KHIP_X_DIV, KHIP_X_OUT}, {(uint64_t)(int64_t)INT32_MIN, (uint64_t)-1LL}, 0);
  CHECK(o.v.f == 0 && (int64_t)o.v.v == INT32_MIN && o.errors == 0);
  o = run({L, L}, {col(0), col(1), KHIP_X_MOD, KHIP_X_OUT}, {5, 0}, 0);
  CHECK(o.v.f == X_ERR && o.errors == 1);
  o = run({L, L}, {col(0), col(1), KHIP_X_ADD, KHIP_X_OUT}, {5, 0}, 2);  // NULL operand: the unboxing throws
  CHECK(o.v.f == X_ERR && o.errors == 1);
  o = run({I, I}, {col(0), col(1), KHIP_X_MUL, KHIP_X_OUT}, {65536, 65536}, 0);  // INT * INT wraps at 32 bits
  CHECK(o.v.f == 0 && o.v.v == 0);
  o = run({I, L}, {col(0), col(1), KHIP_X_MUL, KHIP_X_OUT}, {65536, 65536}, 0);
  CHECK(o.v.f == 0 && o.v.v == (1ull << 32));
  o = run({L, D}, {col(0), col(1), KHIP_X_ADD, KHIP_X_OUT}, {(1ull << 53) + 1, x_bits(0.0)}, 0);  // long -> double: to even
  CHECK(o.v.f == 0 && x_f64(o.v.v) == 9007199254740992.0);
  o = run({L}, {col(0), KHIP_X_CAST_F64, KHIP_X_OUT}, {0}, 1);  // casts are null-safe
  CHECK(o.v.f == X_NULL && o.errors == 0);
  o = run({D, D}, {col(0), col(1), KHIP_X_DIV, KHIP_X_OUT}, {x_bits(1.0), x_bits(-0.0)}, 0);
  CHECK(o.v.f == 0 && x_f64(o.v.v) == -inf);
  // a NULL left operand hides the right side's ERROR; the mirror does not
  const std::vector<int64_t> err = {KHIP_X_CONST_I64, 1, col(1), KHIP_X_DIV};  // 1 / col1
  std::vector<int64_t> c = {col(0)};
  c.insert(c.end(), err.begin(), err.end());
  c.push_back(KHIP_X_EQ);
  c.push_back(KHIP_X_WHERE);
  o = run({L, L}, c, {0, 0}, 1);
  CHECK(!o.keep && o.errors == 0);
  c = err;
  c.push_back(col(0));
  c.push_back(KHIP_X_EQ);
  c.push_back(KHIP_X_WHERE);
  o = run({L, L}, c, {0, 0}, 1);
  CHECK(!o.keep && o.errors == 1);
  // create-time checks
  Program p;
  const char* msg;
  const int32_t types[2] = {L, KHIP_TYPE_STRING};
  const int64_t bad_op[] = {99};
  CHECK(x_compile(2, types, bad_op, 1, &p, &msg) == KHIP_E_INVALID);
  const int64_t trunc[] = {KHIP_X_CONST_I64};
  CHECK(x_compile(2, types, trunc, 1, &p, &msg) == KHIP_E_INVALID);
  const int64_t str_out[] = {col(1), KHIP_X_OUT};
  CHECK(x_compile(2, types, str_out, 2, &p, &msg) == KHIP_E_INVALID);
  const int64_t str_null[] = {col(1), KHIP_X_IS_NULL, KHIP_X_WHERE};
  CHECK(x_compile(2, types, str_null, 3, &p, &msg) == KHIP_OK && p.has_where && p.start2 == p.where_end);
  CHECK(x_compile(2, types, nullptr, 0, &p, &msg) == KHIP_E_INVALID);
  std::vector<int64_t> deep(9, col(0));
  CHECK(x_compile(2, types, deep.data(), 9, &p, &msg) == KHIP_E_UNSUPPORTED);
  std::vector<int64_t> lng(65, col(0));
  CHECK(x_compile(2, types, lng.data(), 65, &p, &msg) == KHIP_E_UNSUPPORTED);
  if (failures) return 1;
  std::printf("selftest ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "selftest")) return selftest();
  Program p;
  std::vector<int32_t> types;
  bool have = false;
  char tag[8];
  while (std::scanf("%7s", tag) == 1) {
    if (tag[0] == 'P') {
      int n_cols = 0, n_code = 0;
      if (std::scanf("%d", &n_cols) != 1 || n_cols < 0 || n_cols > 1000) return 2;
      types.assign(n_cols, 0);
      for (int c = 0; c < n_cols; c++)
        if (std::scanf("%" SCNd32, &types[c]) != 1) return 2;
      if (std::scanf("%d", &n_code) != 1 || n_code < 0 || n_code > 1000) return 2;
      std::vector<int64_t> code(n_code);
      for (int i = 0; i < n_code; i++)
        if (std::scanf("%" SCNd64, &code[i]) != 1) return 2;
      const char* msg = "";
      const khip_status st = x_compile(n_cols, types.data(), code.data(), n_code, &p, &msg);
      have = st == KHIP_OK;
      std::printf("P %d %d %d %d %s\n", (int)st, have ? p.n_out : 0, have ? (int)p.has_where : 0,
                  have ? (int)p.has_key : 0, msg);
    } else if (tag[0] == 'R') {
      if (!have) return 3;
      unsigned long long nulls = 0;
      if (std::scanf("%llu", &nulls) != 1) return 2;
      std::vector<uint64_t> vals(types.size() + 1, 0);
      for (size_t c = 0; c < types.size(); c++) {
        int64_t v;
        if (std::scanf("%" SCNd64, &v) != 1) return 2;
        vals[c] = (uint64_t)v;
      }
      RowResult r;
      x_eval_row(p, vals.data(), nulls, &r);
      std::printf("R %d %d", (int)r.keep, r.n_errors);
      for (int c = 0; c < p.n_out; c++) std::printf(" %u %" PRIu64, r.out[c].f, r.out[c].f ? 0 : r.out[c].v);
      std::printf(" %u %" PRIu64 "\n", r.key.f, r.key.f ? 0 : r.key.v);
    } else {
      return 2;
    }
  }
  return 0;
}
