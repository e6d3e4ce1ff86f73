// khip_expr.hip — WHERE filters and computed columns between decode and push (khip_expr_*; gfx950).
//
// The program (include/ksqldb_hip.h, "WHERE filters and computed columns") is typed and lowered
// once at create (khip_expr.hpp, x_compile) into a list of typed instructions with their stack slot
// resolved.  The kernels interpret that list with one thread per row.  The list is uniform over the
// grid: its words are read through scalar loads and the dispatch is a scalar branch; only the values
// are per lane.  The operand stack lives in LDS slot-major, [slot][thread]: the slot is uniform, so
// every access of a wave is one conflict-free row, and nothing is indexed at run time in registers
// (no scratch; profiles/expr/README.md).  A value's NULL and ERROR states are two flag bits beside
// it (khip_expr.hpp): data, not control flow.
//
//   no WHERE   k_expr_out over the input rows: output position = input row.
//   WHERE      k_expr_keep   the program up to the WHERE: one keep byte per row, ERRORs counted
//              scan_excl     output positions of the kept rows (khip_sort.hpp)
//              k_expr_list   row list: idx[position] = row
//              k_expr_out    over the OUTPUT positions: gathers row idx[p], evaluates the rest of
//                            the program for kept rows only and copies ts / key / partition /
//                            stream_time along.  A wave owns 64 consecutive output positions, so a
//                            validity bitmap is one ballot and one 8-byte store per wave: no two
//                            threads ever touch the same bitmap byte.
//              UTF-8 keys    the kept rows' byte lengths (written by k_expr_out) -> scan_excl ->
//                            offsets from 0; k_expr_keycopy copies each key's bytes.
//
// This file is compiled with -ffp-contract=off (Makefile): a DOUBLE a * b + c stays two roundings.
#include <string.h>

#include <algorithm>
#include <vector>

#include "khip_expr.hpp"
#include "khip_sort.hpp"
#include "khip_util.hpp"

using namespace khip;
using namespace khip::expr;

namespace {

constexpr int XB = 256;  // threads per block (abi.py states it as EXPR_BLOCK for the tests' shapes)

struct XIn {
  const void* col[X_MAX_COLS];
  const uint8_t* cvalid[X_MAX_COLS];
  const uint8_t* row_valid;
  const uint8_t* key_valid;
  const int64_t* key_i64;
  const int64_t* ts;
  const int32_t* partition;
  const int64_t* stream_time;
  const int64_t* koff;
};

struct XOut {
  void* col[X_MAX_OUT];
  uint64_t* cvalid[X_MAX_OUT];  // bitmaps, written a 64-row word at a time
  uint64_t* row_valid;
  uint64_t* key_valid;
  int64_t* key_i64;
  int64_t* ts;
  int32_t* partition;
  int64_t* stream_time;
  int64_t* klen;
};

struct XStack {
  uint64_t v[X_MAX_STACK][XB];
  uint32_t f[X_MAX_STACK][XB];
};

// One non-sink instruction on the calling thread's stack column.  op / arg / slot are uniform.
__device__ __forceinline__ void x_step(XStack& s, int op, int arg, int slot, int64_t imm, const XIn& in, int64_t row,
                                       bool inr) {
  const int t = threadIdx.x;
  if (l_is_push(op)) {
    Val v;
    v.v = (uint64_t)imm;
    v.f = 0;
    if (op != L_CONST) {
      const bool ok = inr && bit_get(in.cvalid[arg], row);
      v.v = 0;
      if (ok && op == L_COL32) v.v = (uint64_t)(int64_t)((const int32_t*)in.col[arg])[row];
      if (ok && op == L_COL64) v.v = ((const uint64_t*)in.col[arg])[row];
      v.f = ok ? 0 : X_NULL;
    }
    s.v[slot][t] = v.v;
    s.f[slot][t] = v.f;
    return;
  }
  Val a, b;
  a.v = s.v[slot][t];
  a.f = s.f[slot][t];
  b.v = 0;
  b.f = 0;
  if (l_is_binary(op)) {
    b.v = s.v[slot + 1][t];
    b.f = s.f[slot + 1][t];
  }
  const Val r = x_exec(op, arg, a, b);
  s.v[slot][t] = r.v;
  s.f[slot][t] = r.f;
}

__device__ __forceinline__ void count_errors(bool err, unsigned long long* n_err) {
  const unsigned long long m = __ballot(err);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(n_err, (unsigned long long)__popcll(m));
}

// The program's prefix up to its WHERE: keep[i] = the row passes.  A null-value row is dropped
// unevaluated (its ERRORs are not counted).
__global__ __launch_bounds__(XB) void k_expr_keep(const LIns* __restrict__ prog, int n_ins, XIn in, int64_t n,
                                                   uint8_t* __restrict__ keep, unsigned long long* __restrict__ n_err) {
  __shared__ XStack s;
  const int64_t row = (int64_t)blockIdx.x * XB + threadIdx.x;
  const bool inr = row < n;
  const bool live = inr && bit_get(in.row_valid, row);
  for (int pc = 0; pc < n_ins; pc++) {
    const int op = __builtin_amdgcn_readfirstlane(prog[pc].op);
    const int arg = __builtin_amdgcn_readfirstlane(prog[pc].arg);
    const int slot = __builtin_amdgcn_readfirstlane(prog[pc].slot);
    if (op == L_WHERE) {
      const uint64_t v = s.v[slot][threadIdx.x];
      const uint32_t f = s.f[slot][threadIdx.x];
      const bool err = live && (f & X_ERR);
      if (inr) keep[row] = live && !(f & X_ERR) && v;
      count_errors(err, n_err);
    } else {
      x_step(s, op, arg, slot, prog[pc].imm, in, row, inr);
    }
  }
}

__global__ __launch_bounds__(256) void k_expr_list(const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos,
                                                   int64_t n, int64_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && keep[i]) idx[pos[i]] = i;
}

__device__ __forceinline__ void put_bits(uint64_t* bm, int64_t p, bool bit, bool wave_in) {
  const unsigned long long m = __ballot(bit);
  if (bm != nullptr && wave_in && (threadIdx.x & 63) == 0) bm[p >> 6] = m;
}

// Instructions [first, last) over the n_out output positions; idx (WHERE) names each position's
// input row, null: position = row.  OUT / KEY write at the output position; with idx the row's
// other arrays are copied along.  Every lane stays in the loop (the ballots need the whole wave);
// lanes past n_out compute on nothing and store nothing.
__global__ __launch_bounds__(XB) void k_expr_out(const LIns* __restrict__ prog, int first, int last, XIn in, XOut out,
                                                  int64_t n_out, const int64_t* __restrict__ idx, int copy_key,
                                                  unsigned long long* __restrict__ n_err) {
  __shared__ XStack s;
  const int64_t p = (int64_t)blockIdx.x * XB + threadIdx.x;
  const bool inr = p < n_out;
  const bool wave_in = (p & ~(int64_t)63) < n_out;  // the wave's first position exists: it owns a bitmap word
  const int64_t row = !inr ? 0 : idx != nullptr ? idx[p] : p;
  const bool live = inr && bit_get(in.row_valid, row);
  for (int pc = first; pc < last; pc++) {
    const int op = __builtin_amdgcn_readfirstlane(prog[pc].op);
    const int arg = __builtin_amdgcn_readfirstlane(prog[pc].arg);
    const int slot = __builtin_amdgcn_readfirstlane(prog[pc].slot);
    if (!l_is_sink(op)) {
      x_step(s, op, arg, slot, prog[pc].imm, in, row, inr);
      continue;
    }
    if (op == L_WHERE) continue;  // (re-run prefix: the keep pass has judged it)
    const uint64_t v = s.v[slot][threadIdx.x];
    const uint32_t f = s.f[slot][threadIdx.x];
    const bool ok = live && f == 0;
    count_errors(live && (f & X_ERR), n_err);
    if (op == L_OUT) {
      const int c = arg & 0xff, ty = arg >> 8;
      if (inr) {
        if (ty == KHIP_TYPE_INT32) ((int32_t*)out.col[c])[p] = ok ? (int32_t)(uint32_t)v : 0;
        else ((uint64_t*)out.col[c])[p] = ok ? v : 0;
      }
      put_bits(out.cvalid[c], p, ok, wave_in);
    } else {  // L_KEY
      if (inr) out.key_i64[p] = ok ? (int64_t)v : 0;
      put_bits(out.key_valid, p, ok, wave_in);
    }
  }
  if (idx == nullptr) return;  // nothing else moves: the pass-through arrays are the input's
  if (inr) {
    out.ts[p] = in.ts[row];
    if (copy_key && in.key_i64 != nullptr) out.key_i64[p] = in.key_i64[row];
    if (copy_key && in.koff != nullptr) out.klen[p] = in.koff[row + 1] - in.koff[row];
    if (in.partition != nullptr) out.partition[p] = in.partition[row];
    if (in.stream_time != nullptr) out.stream_time[p] = in.stream_time[row];
  }
  put_bits(out.row_valid, p, live, wave_in);
  if (copy_key) put_bits(out.key_valid, p, inr && bit_get(in.key_valid, row), wave_in);
}

// One thread per kept row: its key bytes to the rebuilt offsets.
__global__ __launch_bounds__(256) void k_expr_keycopy(const int64_t* __restrict__ idx, int64_t n,
                                                      const int64_t* __restrict__ in_off,
                                                      const uint8_t* __restrict__ in_bytes,
                                                      const int64_t* __restrict__ out_off,
                                                      uint8_t* __restrict__ out_bytes) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int64_t row = idx[p];
  const int64_t a = in_off[row], len = in_off[row + 1] - a, o = out_off[p];
  for (int64_t k = 0; k < len; k++) out_bytes[o + k] = in_bytes[a + k];
}

}  // namespace

struct khip_expr {
  Program prog;
  std::vector<int32_t> col_types;
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf d_prog, ctr, keep, pos, idx, scan_tmp;
  DevBuf o_col[X_MAX_OUT], o_cvalid[X_MAX_OUT], o_row_valid, o_key_valid, o_key, o_ts, o_part, o_st, o_koff, o_kbytes;
  DevBuf st_col[X_MAX_COLS], st_cvalid[X_MAX_COLS], st_row_valid, st_key_valid, st_key, st_ts, st_part, st_st, st_koff,
      st_kbytes;
  std::vector<const void*> col_ptrs;
  std::vector<const uint8_t*> val_ptrs;
};

static khip_status xstage(khip_expr* e, DevBuf& b, const void* src, size_t bytes, const void** dev) {
  KHIP_TRY(b.ensure(std::max<size_t>(bytes, 8)));
  if (bytes) KHIP_TRY_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, e->stream));
  *dev = b.p;
  return KHIP_OK;
}

template <class T>
static khip_status xstage_opt(khip_expr* e, DevBuf& b, const T*& ptr, size_t bytes) {
  if (!ptr) return KHIP_OK;
  const void* d = nullptr;
  KHIP_TRY(xstage(e, b, ptr, bytes, &d));
  ptr = (const T*)d;
  return KHIP_OK;
}

extern "C" {

khip_status khip_expr_create(int32_t device, int32_t n_cols, const int32_t* col_types, const int64_t* code,
                             int32_t n_code, khip_expr** out) {
  clear_error();
  if (!out) return fail(KHIP_E_INVALID, "null argument");
  *out = nullptr;
  khip_expr* e = new khip_expr();
  const char* msg = "";
  const khip_status st = x_compile(n_cols, col_types, code, n_code, &e->prog, &msg);
  if (st != KHIP_OK) {
    delete e;
    return fail(st, std::string("khip_expr_create: ") + msg);
  }
  e->col_types.assign(col_types, col_types + n_cols);
  e->device = device;
  DeviceGuard g(device);
  if (hipStreamCreateWithFlags(&e->stream, hipStreamDefault) != hipSuccess) {
    delete e;
    return fail(KHIP_E_DEVICE, "hipStreamCreate failed (no device?)");
  }
  khip_status s2 = e->d_prog.ensure(sizeof(LIns) * X_MAX_LINS);
  if (s2 == KHIP_OK && hipMemcpyAsync(e->d_prog.p, e->prog.ins, sizeof(LIns) * X_MAX_LINS, hipMemcpyHostToDevice,
                                      e->stream) != hipSuccess)
    s2 = fail(KHIP_E_DEVICE, "program upload failed");
  if (s2 == KHIP_OK) s2 = e->ctr.ensure(8);
  if (s2 == KHIP_OK && hipStreamSynchronize(e->stream) != hipSuccess) s2 = fail(KHIP_E_DEVICE, "program upload failed");
  if (s2 != KHIP_OK) {
    khip_expr_destroy(e);
    return s2;
  }
  *out = e;
  return KHIP_OK;
}

khip_status khip_expr_n_out(const khip_expr* e, int32_t* n_out) {
  clear_error();
  if (!e || !n_out) return fail(KHIP_E_INVALID, "null argument");
  *n_out = e->prog.n_out;
  return KHIP_OK;
}

khip_status khip_expr_out_type(const khip_expr* e, int32_t i, int32_t* out_type) {
  clear_error();
  if (!e || !out_type) return fail(KHIP_E_INVALID, "null argument");
  if (i < 0 || i >= e->prog.n_out) return fail(KHIP_E_INVALID, "OUT column index out of range");
  *out_type = e->prog.out_type[i];
  return KHIP_OK;
}

khip_status khip_expr_apply(khip_expr* e, const khip_batch* in, khip_batch* out, int64_t* n_errors) {
  clear_error();
  if (!e || !in || !out) return fail(KHIP_E_INVALID, "null argument");
  const Program& P = e->prog;
  const int64_t n = in->n_rows;
  if (n < 0) return fail(KHIP_E_INVALID, "batch shape");
  if (in->mem != KHIP_MEM_HOST && in->mem != KHIP_MEM_DEVICE) return fail(KHIP_E_INVALID, "batch mem");
  if (in->n_cols <= P.max_col)
    return fail(KHIP_E_INVALID, "the batch has " + std::to_string(in->n_cols) + " columns, the program names column " +
                                    std::to_string(P.max_col));
  if (n > 0 && !in->ts) return fail(KHIP_E_INVALID, "batch without ts");
  if (P.max_col >= 0 && !in->col_data) return fail(KHIP_E_INVALID, "batch without col_data");
  for (int c = 0; c <= P.max_col; c++)
    if (((P.used >> c) & 1) && n > 0 && e->col_types[c] != KHIP_TYPE_STRING && !in->col_data[c])
      return fail(KHIP_E_INVALID, "null column " + std::to_string(c));
  DeviceGuard g(e->device);
  hipStream_t st = e->stream;
  const size_t bm = (size_t)(n + 7) / 8;
  const bool utf8 = in->key_offsets != nullptr;

  XIn xi{};
  xi.row_valid = in->row_valid;
  xi.key_valid = in->key_valid;
  xi.key_i64 = utf8 ? nullptr : in->key_i64;
  xi.ts = in->ts;
  xi.partition = in->partition;
  xi.stream_time = in->stream_time;
  xi.koff = in->key_offsets;
  const uint8_t* kbytes = in->key_bytes;
  for (int c = 0; c <= P.max_col; c++)
    if ((P.used >> c) & 1) {
      xi.col[c] = in->col_data[c];
      xi.cvalid[c] = in->col_valid ? in->col_valid[c] : nullptr;
    }
  if (in->mem == KHIP_MEM_HOST) {
    KHIP_TRY(xstage_opt(e, e->st_ts, xi.ts, (size_t)n * 8));
    KHIP_TRY(xstage_opt(e, e->st_row_valid, xi.row_valid, bm));
    KHIP_TRY(xstage_opt(e, e->st_key_valid, xi.key_valid, bm));
    KHIP_TRY(xstage_opt(e, e->st_key, xi.key_i64, (size_t)n * 8));
    KHIP_TRY(xstage_opt(e, e->st_part, xi.partition, (size_t)n * 4));
    KHIP_TRY(xstage_opt(e, e->st_st, xi.stream_time, (size_t)n * 8));
    if (utf8) {
      const int64_t kb = in->key_offsets[n];
      KHIP_TRY(xstage_opt(e, e->st_koff, xi.koff, (size_t)(n + 1) * 8));
      KHIP_TRY(xstage_opt(e, e->st_kbytes, kbytes, (size_t)kb));
    }
    for (int c = 0; c <= P.max_col; c++)
      if ((P.used >> c) & 1) {
        const size_t w = e->col_types[c] == KHIP_TYPE_INT32 ? 4 : 8;
        KHIP_TRY(xstage_opt(e, e->st_col[c], xi.col[c], (size_t)n * w));
        KHIP_TRY(xstage_opt(e, e->st_cvalid[c], xi.cvalid[c], bm));
      }
  }

  KHIP_TRY_HIP(hipMemsetAsync(e->ctr.p, 0, 8, st));
  unsigned long long* n_err = e->ctr.as<unsigned long long>();
  const LIns* prog = e->d_prog.as<LIns>();

  int64_t n_out = n;
  const int64_t* idx = nullptr;
  if (P.has_where) {
    n_out = 0;
    if (n > 0) {
      KHIP_TRY(e->keep.ensure((size_t)n));
      KHIP_TRY(e->pos.ensure((size_t)n * 8));
      KHIP_TRY(e->idx.ensure((size_t)n * 8));
      hipLaunchKernelGGL(k_expr_keep, dim3((unsigned)ceil_div(n, XB)), dim3(XB), 0, st, prog, P.where_end, xi, n,
                         e->keep.as<uint8_t>(), n_err);
      KHIP_TRY_HIP(hipGetLastError());
      KHIP_TRY((ksort::scan_excl<uint8_t, int64_t>(st, e->scan_tmp, e->keep.as<uint8_t>(), e->pos.as<int64_t>(), n, false,
                                                   &n_out)));
      if (n_out > 0) {
        hipLaunchKernelGGL(k_expr_list, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, e->keep.as<uint8_t>(),
                           e->pos.as<int64_t>(), n, e->idx.as<int64_t>());
        KHIP_TRY_HIP(hipGetLastError());
      }
    }
    idx = e->idx.as<int64_t>();
  }

  // outputs (a bitmap is whole 64-row words)
  const size_t rows = (size_t)std::max<int64_t>(n_out, 1);
  const size_t obm = (size_t)ceil_div((int64_t)rows, 64) * 8;
  const bool copy_key = P.has_where && !P.has_key;
  XOut xo{};
  for (int c = 0; c < P.n_out; c++) {
    KHIP_TRY(e->o_col[c].ensure(rows * (P.out_type[c] == KHIP_TYPE_INT32 ? 4 : 8)));
    KHIP_TRY(e->o_cvalid[c].ensure(obm));
    xo.col[c] = e->o_col[c].p;
    xo.cvalid[c] = e->o_cvalid[c].as<uint64_t>();
  }
  if (P.has_key || (copy_key && xi.key_i64)) {
    KHIP_TRY(e->o_key.ensure(rows * 8));
    xo.key_i64 = e->o_key.as<int64_t>();
  }
  if (P.has_key || P.has_where) {
    KHIP_TRY(e->o_key_valid.ensure(obm));
    xo.key_valid = e->o_key_valid.as<uint64_t>();
  }
  if (P.has_where) {
    KHIP_TRY(e->o_row_valid.ensure(obm));
    KHIP_TRY(e->o_ts.ensure(rows * 8));
    xo.row_valid = e->o_row_valid.as<uint64_t>();
    xo.ts = e->o_ts.as<int64_t>();
    if (xi.partition) {
      KHIP_TRY(e->o_part.ensure(rows * 4));
      xo.partition = e->o_part.as<int32_t>();
    }
    if (xi.stream_time) {
      KHIP_TRY(e->o_st.ensure(rows * 8));
      xo.stream_time = e->o_st.as<int64_t>();
    }
    if (copy_key && utf8) {
      KHIP_TRY(e->o_koff.ensure((rows + 1) * 8));
      xo.klen = e->o_koff.as<int64_t>();  // lengths first, scanned in place into offsets
    }
  }
  const int first = P.has_where ? P.start2 : 0;
  if (n_out > 0 && (P.has_where || first < P.n_ins)) {
    hipLaunchKernelGGL(k_expr_out, dim3((unsigned)ceil_div(n_out, XB)), dim3(XB), 0, st, prog, first, P.n_ins, xi, xo,
                       n_out, P.has_where ? idx : nullptr, copy_key ? 1 : 0, n_err);
    KHIP_TRY_HIP(hipGetLastError());
  }
  const uint8_t* o_kbytes = nullptr;
  if (copy_key && utf8) {
    int64_t kb = 0;
    KHIP_TRY((ksort::scan_excl<int64_t, int64_t>(st, e->scan_tmp, xo.klen, xo.klen, n_out, true, &kb)));
    KHIP_TRY(e->o_kbytes.ensure((size_t)std::max<int64_t>(kb, 1)));
    if (n_out > 0 && kb > 0) {
      hipLaunchKernelGGL(k_expr_keycopy, dim3((unsigned)ceil_div(n_out, 256)), dim3(256), 0, st, idx, n_out, xi.koff,
                         kbytes, xo.klen, e->o_kbytes.as<uint8_t>());
      KHIP_TRY_HIP(hipGetLastError());
    }
    o_kbytes = e->o_kbytes.as<uint8_t>();
  }
  // The call returns with the work done, as khip_serde_decode does: the consumer of *out (another
  // handle's stream, which does not order against this one) may read it at once, and a host input's
  // arrays are free again.
  unsigned long long c = 0;
  if (n_errors) KHIP_TRY_HIP(hipMemcpyAsync(&c, e->ctr.p, 8, hipMemcpyDeviceToHost, st));
  KHIP_TRY_HIP(hipStreamSynchronize(st));
  if (n_errors) *n_errors = (int64_t)c;

  e->col_ptrs.assign(std::max(P.n_out, 1), nullptr);
  e->val_ptrs.assign(std::max(P.n_out, 1), nullptr);
  for (int c = 0; c < P.n_out; c++) {
    e->col_ptrs[c] = xo.col[c];
    e->val_ptrs[c] = (const uint8_t*)xo.cvalid[c];
  }
  memset(out, 0, sizeof(*out));
  out->n_rows = n_out;
  out->mem = KHIP_MEM_DEVICE;
  out->n_cols = P.n_out;
  out->col_data = e->col_ptrs.data();
  out->col_valid = e->val_ptrs.data();
  if (P.has_where) {
    out->ts = xo.ts;
    out->row_valid = (const uint8_t*)xo.row_valid;
    out->partition = xo.partition;
    out->stream_time = xo.stream_time;
  } else {
    out->ts = xi.ts;
    out->row_valid = xi.row_valid;
    out->partition = xi.partition;
    out->stream_time = xi.stream_time;
  }
  if (P.has_key) {
    out->key_i64 = xo.key_i64;
    out->key_valid = (const uint8_t*)xo.key_valid;
  } else if (P.has_where) {
    out->key_valid = (const uint8_t*)xo.key_valid;
    if (utf8) {
      out->key_offsets = xo.klen;
      out->key_bytes = o_kbytes;
    } else {
      out->key_i64 = xo.key_i64;
    }
  } else {
    out->key_valid = xi.key_valid;
    out->key_i64 = xi.key_i64;
    out->key_offsets = xi.koff;
    out->key_bytes = utf8 ? kbytes : nullptr;
  }
  return KHIP_OK;
}

khip_status khip_expr_sync(khip_expr* e) {
  clear_error();
  if (!e) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(e->device);
  KHIP_TRY_HIP(hipStreamSynchronize(e->stream));
  return KHIP_OK;
}

khip_status khip_expr_destroy(khip_expr* e) {
  if (!e) return KHIP_OK;
  DeviceGuard g(e->device);
  if (e->stream) {
    hipStreamSynchronize(e->stream);
    hipStreamDestroy(e->stream);
  }
  delete e;  // the DevBufs free with it
  return KHIP_OK;
}

}  // extern "C"
