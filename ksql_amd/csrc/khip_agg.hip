// khip_agg.hip — windowed / unwindowed GROUP BY aggregation on MI355X (gfx950).
//
// Replaces, for one query task, the Kafka Streams KStreamWindowAggregate /
// KStreamAggregate processor + RocksDB window store + KudafAggregator chain that
// KSPlanBuilder.visitStreamWindowedAggregate / visitStreamAggregate build
// (S/KSPlanBuilder.java:293-304, :144-155; S/StreamAggregateBuilder.java:156-222,
// :81-138).  Semantics: SURVEY.md §8.0, restated in oracle/oracle.c R1–R6.
//
// Data layout in HBM (one handle):
//   table   : cap slots (power of two) × slot_words u64, AoS, 32 or 64 B per slot so a
//             group is one cache line: [w0 key | claim ref][w1 windowStart | EMPTY]
//             [rowtime][state words ...].
//   state   : deduplicated per input column: non-null count, sum (i64 / f64 bits),
//             min / max as total-order int64 keys; one COUNT(*) word.
//   dict    : UTF8 keys only — open-addressing dictionary → stable key id
//             (= byte offset of the key's entry in an append-only arena): khip_dict.hip.
//
// Per micro-batch (all on the handle's stream):
//   k_blockmax → k_scan_blocks : stream time before each 2048-record block
//                                (exclusive prefix max, carried across batches)
//   [UTF8] k_dict_probe → k_dict_commit → k_dict_resolve (khip_dict.hip)
//   k_apply     : in-block prefix max → late test → window fan-out → find-or-claim the
//                 (key, ws) slot with one 64-bit CAS whose value references the batch
//                 row (no spin, no fence) → agent-scope atomics for the state
//   k_finalize  : turn this batch's claim references into resident (key, ws)
//   failures (probe budget exhausted) are resumed after a table doubling, exactly.
//   [LATEST / EARLIEST_BY_OFFSET] k_off_iota before, a k_off_resolve_* kernel after the engine
//                 (either engine): see "offset aggregates" below.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "khip_util.hpp"

#include "khip_agg_internal.hpp"
#include "khip_variance.hpp"
#include "khip_correlation.hpp"

namespace khip {

// ------------------------------------------------------------------- kernels

__global__ __launch_bounds__(BLOCK) void k_blockmax(const int64_t* __restrict__ ts,
                                                    const uint8_t* __restrict__ kv,
                                                    const uint8_t* __restrict__ rv, int64_t n,
                                                    int64_t* __restrict__ blockmax,
                                                    const int64_t* __restrict__ st_at) {
  __shared__ int64_t lds[BLOCK / 64];
  const int64_t base = (int64_t)blockIdx.x * RPB;
  int64_t m = -1;
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    const int64_t i = base + k * BLOCK + threadIdx.x;
    if (i < n && bit_get(kv, i) && bit_get(rv, i)) {
      // ABI 5 domains: the row's given stream time (an upper bound of its ts), else its ts
      const int64_t t = ts[i] < 0 ? -1 : (st_at ? st_at[i] : ts[i]);
      m = t > m ? t : m;
    }
  }
  int64_t tot;
  block_incl_max(m, lds, &tot);
  if (threadIdx.x == 0) blockmax[blockIdx.x] = tot;
}

// Exclusive prefix max over nb block maxima, seeded and updated with *stream_time.
__global__ __launch_bounds__(1024) void k_scan_blocks(const int64_t* __restrict__ blockmax,
                                                      int64_t nb, int64_t* __restrict__ prefix,
                                                      int64_t* __restrict__ stream_time) {
  __shared__ int64_t lds[1024 / 64];
  __shared__ int64_t incl_all[1024];
  int64_t carry = *stream_time;
  for (int64_t b0 = 0; b0 < nb; b0 += blockDim.x) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < nb ? blockmax[b] : INT64_MIN;
    int64_t tot;
    const int64_t incl = block_incl_max(v, lds, &tot);
    incl_all[threadIdx.x] = incl;
    __syncthreads();
    const int64_t excl = threadIdx.x == 0 ? INT64_MIN : incl_all[threadIdx.x - 1];
    if (b < nb) prefix[b] = excl > carry ? excl : carry;
    carry = tot > carry ? tot : carry;
    __syncthreads();
  }
  if (threadIdx.x == 0) *stream_time = carry;
}

// EMIT FINAL (S/StreamAggregateBuilder.java:282-285, Kafka Streams EmitStrategy.onWindowClose):
// with the emission check after every record, a window is emitted by the record whose stream
// time first reaches ws + size + grace, unless the window store had already expired it there:
// the store's observed time is then floor(M / adv) * adv (M = that record's stream time), so
// the window is lost iff ws < floor(M / adv) * adv - retention.  That needs M to jump into a later
// advance bucket in one record.  Per record (arrival order, accepted rows only; prefix = stream
// time before each RPB block): a record that moves the stream time from Mp to M > Mp with
// floor(M / adv) > floor(Mp / adv) loses the window starts in
//   [Mp - size - grace + 1, min(M - size - grace, floor(M / adv) * adv - retention - 1)]
// (rounded to multiples of adv); non-empty ranges are appended to lost[] as (lo, hi) pairs.
__global__ __launch_bounds__(BLOCK) void k_emit_lost(const int64_t* __restrict__ ts, const uint8_t* __restrict__ kv,
                                                     const uint8_t* __restrict__ rv, int64_t n,
                                                     const int64_t* __restrict__ prefix, int64_t size, int64_t adv,
                                                     int64_t grace, int64_t retention, int64_t* __restrict__ lost,
                                                     int64_t cap, unsigned long long* __restrict__ ctr) {
  __shared__ int64_t lmax[BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * RPB + (int64_t)threadIdx.x * ITEMS;
  int64_t m = -1;
  for (int k = 0; k < ITEMS; k++) {
    const int64_t i = i0 + k;
    if (i < n && bit_get(kv, i) && bit_get(rv, i) && ts[i] > m) m = ts[i];
  }
  lmax[threadIdx.x] = m;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {  // inclusive prefix max over the block's threads
    const int64_t y = threadIdx.x >= off ? lmax[threadIdx.x - off] : -1;
    __syncthreads();
    if (y > lmax[threadIdx.x]) lmax[threadIdx.x] = y;
    __syncthreads();
  }
  int64_t mp = prefix[blockIdx.x];
  if (threadIdx.x > 0 && lmax[threadIdx.x - 1] > mp) mp = lmax[threadIdx.x - 1];
  const int64_t sg = size + grace;
  for (int k = 0; k < ITEMS; k++) {
    const int64_t i = i0 + k;
    if (i >= n || !bit_get(kv, i) || !bit_get(rv, i)) continue;
    const int64_t t = ts[i];
    if (t <= mp) continue;
    const int64_t bp = mp < 0 ? -1 : mp / adv, b = t / adv;
    if (b > bp) {
      int64_t lo = mp - sg + 1;
      int64_t hi = t - sg;
      const int64_t exp_hi = b * adv - retention - 1;
      hi = hi < exp_hi ? hi : exp_hi;
      lo = lo < 0 ? 0 : lo;
      lo = (lo + adv - 1) / adv * adv;  // window starts are multiples of adv
      if (lo <= hi) {
        const unsigned long long slot = atomicAdd(ctr, 1ULL);
        if ((int64_t)slot < cap) {
          lost[2 * slot] = lo;
          lost[2 * slot + 1] = hi;
        }
      }
    }
    mp = t;
  }
}

// Find or claim the (key, ws) slot and apply the record's aggregate updates.
// Claim reference: bit63 | fp15 << 48 | window index j << 36 | batch row (36 bits).
__device__ __forceinline__ int upsert_apply(const ApplyParams& p, uint64_t* __restrict__ table,
                                             uint64_t mask, int64_t hkey, int64_t key, int64_t ws,
                                             int64_t j, int64_t row, int64_t t,
                                             const int64_t* __restrict__ keys,
                                             const int64_t* __restrict__ ts, const ColPtrs& cols) {
  const uint64_t h = group_hash(hkey, ws);
  const uint64_t fp = (h >> 49) & 0x7FFFULL;
  const uint64_t myref = (1ULL << 63) | (fp << 48) | ((uint64_t)j << 36) | (uint64_t)row;
  uint64_t slot = h & mask;
  const int sw = p.slot_words;
  for (int probe = 0; probe < MAX_PROBE; probe++) {
    uint64_t* s = table + slot * (uint64_t)sw;
    const int64_t w1 = (int64_t)s[1];
    bool hit = false;
    int isnew = 0;
    if (w1 != EMPTY_WS) {
      hit = (w1 == ws) && ((int64_t)s[0] == key);
    } else {
      uint64_t w0 = ld_relaxed(s);
      if (w0 == 0) {
        const uint64_t old = atomicCAS((unsigned long long*)s, 0ULL, (unsigned long long)myref);
        if (old == 0) {
          hit = true;
          isnew = 1;
        } else {
          w0 = old;
        }
      }
      if (!hit && ((w0 >> 48) & 0x7FFFULL) == fp) {
        const int64_t idx = (int64_t)(w0 & ((1ULL << 36) - 1));
        const int64_t jj = (int64_t)((w0 >> 36) & 0xFFFULL);
        if (keys[idx] == key) {
          const int64_t ws2 = p.windowed ? first_window_start(ts[idx], p.size, p.adv) + jj * p.adv : 0;
          hit = ws2 == ws;
        }
      }
    }
    if (hit) {
      __hip_atomic_fetch_max((int64_t*)&s[2], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int o = 0; o < p.n_ops; o++) {
        const UpdOp op = p.ops[o];
        int64_t* w = (int64_t*)&s[op_word(op)];
        if (op.kind == OP_INC) {
          __hip_atomic_fetch_add(w, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          continue;
        }
        if (!bit_get(cols.valid[op.col], row)) continue;
        const int32_t ty = p.col_type[op.col];
        switch (op.kind) {
          case OP_INC_VALID:
            __hip_atomic_fetch_add(w, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          case OP_ADD_I64:
            __hip_atomic_fetch_add((uint64_t*)w, (uint64_t)load_col_raw(cols, ty, op.col, row),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          case OP_ADD_F64: {
            const double v = ((const double*)cols.data[op.col])[row];
            unsafeAtomicAdd((double*)w, v);
            break;
          }
          case OP_MIN:
          case OP_MAX: {
            int64_t k = load_col_raw(cols, ty, op.col, row);
            if (ty == KHIP_TYPE_DOUBLE) {
              double d;
              __builtin_memcpy(&d, &k, 8);
              k = f64_order_key(d);
            }
            if (op.kind == OP_MIN)
              __hip_atomic_fetch_min(w, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
              __hip_atomic_fetch_max(w, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          case OP_TOPK:
          case OP_TOPK_DISTINCT: {
            // The insertion chain of k_part_agg's lds_apply (DESIGN.md "TOPK aggregates") on the
            // slot's words in HBM: returning agent-scope max atomics (global_atomic_smax_x2), any
            // interleaving with the other records of the group.  A record resumed after a table
            // doubling restarts at its first unapplied window, so no chain runs twice.
            int64_t v = load_col_raw(cols, ty, op.col, row);
            if (ty == KHIP_TYPE_DOUBLE) {
              double d;
              __builtin_memcpy(&d, &v, 8);
              v = f64_order_key(d);
            }
            const bool distinct = op.kind == OP_TOPK_DISTINCT;
            const int ns = op_slots(op);
            if (distinct && v == INT64_MIN)  // TOPKDISTINCT(BIGINT) Long.MIN_VALUE: the flag word
              __hip_atomic_fetch_max(w + ns, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int j = 0; j < ns && v != INT64_MIN; j++) {
              const int64_t old = __hip_atomic_fetch_max(w + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (distinct && old == v) break;
              v = old < v ? old : v;
            }
            break;
          }
          default:  // OP_ADD_HI32 / OP_ADD_SQ (STDDEV: x >> 32 / a limb of x², khip_variance.hpp); here, so
                    // that the dispatch of the kinds above stays what it was
            if (op.kind == OP_ADD_HI32 || op.kind == OP_ADD_SQ) {
              __hip_atomic_fetch_add((uint64_t*)w, var_addend(op, load_col_raw(cols, ty, op.col, row)),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (op_is_pair(op)) {
              // CORRELATION (khip_correlation.hpp): only a record with both arguments non-null counts
              const int c2 = op_col2(op);
              if (!bit_get(cols.valid[c2], row)) break;
              __hip_atomic_fetch_add((uint64_t*)w,
                                     pair_addend(op, load_col_raw(cols, ty, op.col, row),
                                                 load_col_raw(cols, p.col_type[c2], c2, row)),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            break;
        }
      }
      return 1 + isnew;
    }
    slot = (slot + 1) & mask;
  }
  return 0;
}

__global__ __launch_bounds__(BLOCK) void k_apply(ApplyParams p, const int64_t* __restrict__ hkeys,
                                                 const int64_t* __restrict__ keys,
                                                 const int64_t* __restrict__ ts,
                                                 const uint8_t* __restrict__ kv,
                                                 const uint8_t* __restrict__ rv, ColPtrs cols,
                                                 const int64_t* __restrict__ blockprefix, int64_t n,
                                                 uint64_t* __restrict__ table, uint64_t mask,
                                                 int32_t* __restrict__ resume,
                                                 int64_t* __restrict__ partials, int resume_mode,
                                                 const int64_t* __restrict__ st_at) {
  __shared__ int64_t lds_scan[BLOCK / 64];
  __shared__ unsigned long long lds_cnt[NPART];
  if (threadIdx.x < NPART) lds_cnt[threadIdx.x] = 0;
  int64_t cnt[NPART];
#pragma unroll
  for (int k = 0; k < NPART; k++) cnt[k] = 0;
  const int64_t base = (int64_t)blockIdx.x * RPB;
  int64_t carry = blockprefix[blockIdx.x];
  for (int k = 0; k < ITEMS; k++) {
    const int64_t i = base + k * BLOCK + threadIdx.x;
    const bool in = i < n;
    const int64_t t = in ? ts[i] : -1;
    const bool kval = in && bit_get(kv, i);
    const bool rval = in && bit_get(rv, i);
    const bool valid = kval && rval && t >= 0;
    int64_t tot;
    const int64_t incl = block_incl_max(valid ? t : -1, lds_scan, &tot);
    int64_t st = incl > carry ? incl : carry;  // stream time after this record
    carry = tot > carry ? tot : carry;
    if (!in) continue;
    if (st_at) st = st_at[i];  // ABI 5 domains: given per row
    int64_t j0 = 0;
    if (resume_mode) {
      j0 = resume[i];
      if (j0 < 0) continue;
      resume[i] = -1;
    } else {
      if (!kval) { cnt[P_NULL_KEY]++; continue; }
      if (!rval) { cnt[P_NULL_ROW]++; continue; }
      if (t < 0) { cnt[P_BAD_TS]++; continue; }
      cnt[P_ACCEPTED]++;
    }
    const int64_t key = keys[i];
    const int64_t hkey = hkeys[i];
    if (p.windowed) {
      const int64_t close = st - p.grace;
      const int64_t ws0 = first_window_start(t, p.size, p.adv);
      int64_t j = j0;
      for (int64_t ws = ws0 + j0 * p.adv; ws <= t; ws += p.adv, j++) {
        if (ws + p.size <= close) {  // window closed: late
          cnt[P_LATE]++;
          continue;
        }
        const int r = upsert_apply(p, table, mask, hkey, key, ws, j, i, t, keys, ts, cols);
        if (r == 0) {
          resume[i] = (int32_t)j;
          cnt[P_FAILED]++;
          break;
        }
        cnt[P_APPLIED]++;
        cnt[P_NEW] += r - 1;
      }
    } else {
      const int r = upsert_apply(p, table, mask, hkey, key, 0, 0, i, t, keys, ts, cols);
      if (r == 0) {
        resume[i] = 0;
        cnt[P_FAILED]++;
      } else {
        cnt[P_APPLIED]++;
        cnt[P_NEW] += r - 1;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NPART; k++) {
    const int64_t s = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&lds_cnt[k], (unsigned long long)s);
  }
  __syncthreads();
  if (threadIdx.x < NPART) partials[(int64_t)blockIdx.x * NPART + threadIdx.x] = (int64_t)lds_cnt[threadIdx.x];
}

// Claim references of this batch → resident (key, ws).
__global__ __launch_bounds__(256) void k_finalize(uint64_t* __restrict__ table, int64_t cap, int sw,
                                                  const int64_t* __restrict__ keys,
                                                  const int64_t* __restrict__ ts, int windowed,
                                                  int64_t size, int64_t adv) {
  for (int64_t slot = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; slot < cap;
       slot += (int64_t)gridDim.x * blockDim.x) {
    uint64_t* s = table + slot * (uint64_t)sw;
    if ((int64_t)s[1] != EMPTY_WS) continue;
    const uint64_t w0 = s[0];
    if (w0 == 0) continue;
    const int64_t idx = (int64_t)(w0 & ((1ULL << 36) - 1));
    const int64_t jj = (int64_t)((w0 >> 36) & 0xFFFULL);
    s[0] = (uint64_t)keys[idx];
    s[1] = (uint64_t)(windowed ? first_window_start(ts[idx], size, adv) + jj * adv : 0);
  }
}

__global__ __launch_bounds__(256) void k_init_table(uint64_t* __restrict__ table, int64_t cap, int sw,
                                                    InitWords init) {
  const int64_t total = cap * sw;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x)
    table[e] = (uint64_t)init.w[e & (sw - 1)];
}

// Sum nb rows of K partial counters into out[K] (accumulating).
__global__ __launch_bounds__(256) void k_reduce_partials(const int64_t* __restrict__ partials, int64_t nb,
                                                         int K, int64_t* __restrict__ out) {
  __shared__ unsigned long long acc[NPART];
  if (threadIdx.x < NPART) acc[threadIdx.x] = 0;
  __syncthreads();
  for (int k = 0; k < K; k++) {
    int64_t s = 0;
    for (int64_t b = threadIdx.x; b < nb; b += blockDim.x) s += partials[b * K + k];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) atomicAdd(&acc[k], (unsigned long long)s);
  }
  __syncthreads();
  if (threadIdx.x < K) out[threadIdx.x] += (int64_t)acc[threadIdx.x];
}

// Re-insert resident slots into a larger table.
__global__ __launch_bounds__(256) void k_rehash(const uint64_t* __restrict__ old, int64_t oldcap,
                                                uint64_t* __restrict__ nt, uint64_t nmask, int sw,
                                                int utf8, const uint8_t* __restrict__ arena) {
  for (int64_t slot = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; slot < oldcap;
       slot += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t* s = old + slot * (uint64_t)sw;
    const int64_t ws = (int64_t)s[1];
    if (ws == EMPTY_WS) continue;
    const int64_t key = (int64_t)s[0];
    // (a UTF8 group's hash key: its key hash, or an inline id itself — as k_dict_probe's khash)
    const int64_t hkey = utf8 && !kid_inline(key) ? *(const int64_t*)(arena + key) : key;
    uint64_t d = group_hash(hkey, ws) & nmask;
    while (true) {
      uint64_t* q = nt + d * (uint64_t)sw;
      if (atomicCAS((unsigned long long*)&q[1], (unsigned long long)EMPTY_WS, (unsigned long long)ws) ==
          (unsigned long long)EMPTY_WS) {
        q[0] = (uint64_t)key;
        for (int w = 2; w < sw; w++) q[w] = s[w];
        break;
      }
      d = (d + 1) & nmask;
    }
  }
}

// Compact resident slots passing HAVING into `out` (sw words per row); out may be null
// (count only).  One atomic per block reserves the output range.
__global__ __launch_bounds__(256) void k_compact(const uint64_t* __restrict__ table, int64_t cap, int sw,
                                                 HavingDev h, uint64_t* __restrict__ out, int64_t max_rows,
                                                 unsigned long long* __restrict__ counter) {
  __shared__ int lds_n[256 / 64];
  __shared__ unsigned long long lds_base;
  for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x; s0 < cap; s0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t slot = s0 + threadIdx.x;
    const uint64_t* s = table + slot * (uint64_t)sw;
    const bool take = slot < cap && (int64_t)s[1] != EMPTY_WS && having_ok(s, h);
    const uint64_t bal = __ballot(take);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int before = __popcll(bal & ((1ULL << lane) - 1));
    if (lane == 0) lds_n[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) {
      if (w < wave) off += lds_n[w];
      tot += lds_n[w];
    }
    if (threadIdx.x == 0) lds_base = tot ? atomicAdd(counter, (unsigned long long)tot) : 0;
    __syncthreads();
    if (take && out && (int64_t)(lds_base + off + before) < max_rows) {
      uint64_t* o = out + (lds_base + off + before) * (uint64_t)sw;
      for (int w = 0; w < sw; w++) o[w] = s[w];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- offset aggregates
// LATEST_BY_OFFSET / EARLIEST_BY_OFFSET (khip_agg_internal.hpp OffResolve).  Per push: k_off_iota
// writes the hidden sequence column; the engine keeps MAX / MIN of it per group in whatever order
// it applies the records; a resolve kernel then turns the sequence words won by this push into
// values, before anything reads the rows.  Groups won by earlier pushes are left alone, which keeps
// EARLIEST stable and LATEST independent of how the stream is cut into pushes.
// The N forms (col, N) keep the N largest keys of a hidden column with the TOPK chain (sequence for
// LATEST, complemented sequence for EARLIEST) and the same resolve kernels bring the N values along
// (off_resolve_list; DESIGN.md "Offset aggregates, N forms").

__global__ __launch_bounds__(256) void k_off_iota(int64_t* __restrict__ seq, int64_t n, int64_t base) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    seq[i] = base + i;
}

// The complemented sequence column of EARLIEST's N forms: the N largest ~seq are the N smallest
// sequences, oldest first.  ~seq is never INT64_MIN, the empty slot's key.
__global__ __launch_bounds__(256) void k_off_iota_not(int64_t* __restrict__ nseq, int64_t n, int64_t base) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    nseq[i] = ~(base + i);
}

// Partitioned engine: a block per partition; only partitions the push's records reached are read
// (k_part_chg's test: prn after a pipeline push, else the scatter's partition bases), the rows of
// their current buffer.
template <bool LISTS>
__global__ __launch_bounds__(256) void k_off_resolve_part(uint64_t* __restrict__ b0, uint64_t* __restrict__ b1,
                                                          const uint8_t* __restrict__ sel,
                                                          const int64_t* __restrict__ cnt, int64_t cmax, int sw,
                                                          const int64_t* __restrict__ pbase,
                                                          const uint32_t* __restrict__ prn, OffResolve q) {
  const int64_t p = blockIdx.x;
  if (prn ? prn[p] == 0 : pbase[p + 1] == pbase[p]) return;
  uint64_t* rows = (sel[p] ? b1 : b0) + (uint64_t)p * cmax * sw;
  const int64_t n = cnt[p] < cmax ? cnt[p] : cmax;
  for (int64_t r = threadIdx.x; r < n; r += 256) off_resolve_row<LISTS>(rows + r * sw, q, -1);
}

// Rows [r0, r1) of a flat row array (the closed store's rows appended by this push).
template <bool LISTS>
__global__ __launch_bounds__(256) void k_off_resolve_rows(uint64_t* __restrict__ rows, int64_t r0, int64_t r1, int sw,
                                                          OffResolve q) {
  for (int64_t r = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < r1; r += (int64_t)gridDim.x * blockDim.x)
    off_resolve_row<LISTS>(rows + r * sw, q, -1);
}

// Global-atomic engine, after k_finalize: one thread per accepted record finds the resident slots
// of its (key, window)s again and stores where the slot's sequence word is its own.  Work scales
// with the push (<= fan-out probes per record), not with the table.
template <bool LISTS>
__global__ __launch_bounds__(256) void k_off_resolve_probe(ApplyParams p, const int64_t* __restrict__ hkeys,
                                                           const int64_t* __restrict__ keys,
                                                           const int64_t* __restrict__ ts,
                                                           const uint8_t* __restrict__ kv,
                                                           const uint8_t* __restrict__ rv, int64_t n,
                                                           uint64_t* __restrict__ table, uint64_t mask, OffResolve q) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || !bit_get(kv, i) || !bit_get(rv, i)) return;
  const int64_t t = ts[i];
  if (t < 0) return;
  const int64_t key = keys[i], hkey = hkeys[i], seq = q.base + i;
  const int64_t ws0 = p.windowed ? first_window_start(t, p.size, p.adv) : 0;
  const int64_t wsN = p.windowed ? t : 0;
  const int64_t step = p.windowed ? p.adv : 1;
  for (int64_t ws = ws0; ws <= wsN; ws += step) {
    uint64_t slot = group_hash(hkey, ws) & mask;
    for (int probe = 0; probe < MAX_PROBE; probe++) {
      uint64_t* s = table + slot * (uint64_t)p.slot_words;
      const int64_t w1 = (int64_t)s[1];
      if (w1 == EMPTY_WS) break;  // (a late window of this record may have no group)
      if (w1 == ws && (int64_t)s[0] == key) {
        off_resolve_row<LISTS>(s, q, seq);
        break;
      }
      slot = (slot + 1) & mask;
    }
  }
}

// Exclusive prefix sum of v[0..n) in place (single block); total added to *total.  Each thread
// owns 16 consecutive elements of a 16K-element chunk: one wave scan and one barrier per chunk.
__global__ __launch_bounds__(1024) void k_scan_excl(int64_t* __restrict__ v, int64_t n, int64_t* __restrict__ total) {
  __shared__ int64_t wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < n; b0 += 1024 * 16) {
    const int64_t base = b0 + (int64_t)threadIdx.x * 16;
    int64_t x[16], s = 0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      x[u] = base + u < n ? v[base + u] : 0;
      s += x[u];
    }
    int64_t incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int64_t before = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
      before += k < wave ? wsum[k] : 0;
      tot += wsum[k];
    }
    int64_t run = carry + before + incl - s;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      if (base + u < n) v[base + u] = run;
      run += x[u];
    }
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total += carry;
}

}  // namespace khip

// ------------------------------------------------------------------- host side

using namespace khip;

static inline int agg_base_kind(int32_t kind) { return kind & 0xFFFF & ~KHIP_AGG_KEEP_NULLS; }  // without flag / k bits
static inline int agg_k_bits(int32_t kind) { return kind >> 16; }  // KHIP_AGG_K(k), signed
static inline bool agg_is_topk(int32_t kind) {
  const int b = agg_base_kind(kind);
  return b == KHIP_AGG_TOPK || b == KHIP_AGG_TOPKDISTINCT;
}
static inline bool agg_is_var(int32_t kind) {
  const int b = agg_base_kind(kind);
  return b == KHIP_AGG_STDDEV_SAMP || b == KHIP_AGG_STDDEV_SAMPLE;
}
static inline bool agg_is_pair(int32_t kind) { return agg_base_kind(kind) == KHIP_AGG_CORRELATION; }
static inline bool off_has_lists(const OffResolve& q) {
  for (int k = 0; k < q.n; k++)
    if (q.a[k].n) return true;
  return false;
}
static inline bool agg_is_offset(int32_t kind) {
  const int b = agg_base_kind(kind);
  return b == KHIP_AGG_LATEST_BY_OFFSET || b == KHIP_AGG_EARLIEST_BY_OFFSET;
}

static khip_status plan_state(khip_agg* a) {
  const khip_agg_desc& d = a->desc;
  int word = 3;  // w0, w1, rowtime
  int w_star = -1;
  // offset aggregates: the hidden sequence columns (one per argument column of an ignore-nulls
  // form, whose validity it takes, and one without validity for the KEEP_NULLS forms; EARLIEST's
  // N forms have complemented twins of these), and first
  // in the row the value / null words no update op writes (the sequence words come last: the
  // engines keep every word up to the highest op word)
  a->n_hidden = 0;
  a->offs = OffResolve{};
  a->out_off.assign(d.n_aggs, -1);
  std::vector<int> off_hid(d.n_aggs, -1);
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = a->aggs[i];
    if (!agg_is_offset(s.kind)) continue;
    const int src = (s.kind & KHIP_AGG_KEEP_NULLS) ? -1 : s.arg_col;
    // the N forms (agg_k[i] = N >= 1): N value words, one null-mask word (KEEP_NULLS), LATEST's
    // resolve mark; EARLIEST reads the complemented sequence column (OffSpec)
    const int N = a->agg_k[i];
    const bool latest = agg_base_kind(s.kind) == KHIP_AGG_LATEST_BY_OFFSET;
    const bool neg = N > 0 && !latest;
    if (N > 29 || a->offs.n >= MAX_OFFS) return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
    int h = -1;
    for (int k = 0; k < a->n_hidden; k++)
      if (a->hid_src[k] == src && a->hid_not[k] == neg) h = k;
    if (h < 0) {
      if (d.n_cols + a->n_hidden >= MAX_COLS)
        return fail(KHIP_E_UNSUPPORTED, "offset aggregates: value columns + hidden sequence columns above 8");
      h = a->n_hidden++;
      a->hid_src[h] = src;
      a->hid_not[h] = neg;
    }
    off_hid[i] = d.n_cols + h;
    OffSpec o{};
    o.col = (int8_t)s.arg_col;
    o.type = (int8_t)a->col_types[s.arg_col];
    o.n = (int8_t)N;
    o.earliest = neg ? 1 : 0;
    o.w_val = (int16_t)word;
    word += std::max(N, 1);
    o.w_null = (s.kind & KHIP_AGG_KEEP_NULLS) ? (int16_t)word++ : (int16_t)-1;
    o.w_mark = (N > 0 && latest) ? (int16_t)word++ : (int16_t)-1;
    o.w_seq = -1;
    if (word > 32) return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
    a->out_off[i] = a->offs.n;
    a->offs.a[a->offs.n++] = o;
  }
  const int nc = d.n_cols + a->n_hidden;  // internal argument columns
  std::vector<int> w_cnt(nc, -1), w_sum(nc, -1), w_min(nc, -1), w_max(nc, -1), w_hi(nc, -1), w_sq(nc, -1);
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = a->aggs[i];
    if (agg_is_offset(s.kind)) continue;
    if (s.kind == KHIP_AGG_COUNT_STAR) {
      if (w_star < 0) w_star = word++;
      continue;
    }
    if (agg_is_pair(s.kind)) continue;  // (its own words: below)
    const int c = s.arg_col;
    if (agg_is_topk(s.kind)) {  // TOPK's length is min(the column's non-null count, k); its slots: below
      if (s.kind == KHIP_AGG_TOPK && w_cnt[c] < 0) w_cnt[c] = word++;
      continue;
    }
    // the column's non-null count: COUNT(col), AVG's divisor, MIN/MAX's null test.  SUM alone needs
    // none (SUM over only NULLs is 0, SumKudaf's initial value): its rows stay 32 bytes
    if (s.kind != KHIP_AGG_SUM && w_cnt[c] < 0) w_cnt[c] = word++;
    if ((s.kind == KHIP_AGG_SUM || s.kind == KHIP_AGG_AVG || agg_is_var(s.kind)) && w_sum[c] < 0) w_sum[c] = word++;
    // STDDEV_SAMP / STDDEV_SAMPLE (khip_variance.hpp): beside the count and the sum, Σ (x >> 32) for
    // a BIGINT and the 32-bit limbs of Σx², one word each; both kinds of a column share them
    if (agg_is_var(s.kind) && w_sq[c] < 0) {
      const bool big = a->col_types[c] == KHIP_TYPE_INT64;
      if (big) w_hi[c] = word++;
      w_sq[c] = word;
      word += big ? 4 : 2;
    }
    if (s.kind == KHIP_AGG_MIN && w_min[c] < 0) w_min[c] = word++;
    if (s.kind == KHIP_AGG_MAX && w_max[c] < 0) w_max[c] = word++;
  }
  // CORRELATION(x, y) (khip_correlation.hpp): words that apply only when x and y are both non-null, so
  // none is shared with COUNT / SUM / STDDEV of either column.  A run of consecutive words per
  // (quantity, column, gate column); the pair count and Σxy are keyed by the unordered pair.  So an
  // identical spec adds no word, CORRELATION(y, x) shares all of CORRELATION(x, y)'s, and
  // CORRELATION(x, x) has one Σx run and one Σx² run.
  struct PairRun { int kind, col, col2, word, limbs; };
  std::vector<PairRun> pruns;
  a->out_pair.assign(d.n_aggs, khip_agg::PairWords{});
  a->has_pair = false;
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = a->aggs[i];
    if (!agg_is_pair(s.kind)) continue;
    a->has_pair = true;
    const int x = s.arg_col, y = a->agg_k[i];
    const bool big = a->col_types[x] == KHIP_TYPE_INT64;
    auto run = [&](int kind, int col, int col2, int limbs) {
      for (const PairRun& r : pruns)
        if (r.kind == kind && r.col == col && r.col2 == col2) return r.word;
      if (word + limbs > 32) return -1;
      pruns.push_back(PairRun{kind, col, col2, word, limbs});
      word += limbs;
      return pruns.back().word;
    };
    khip_agg::PairWords& w = a->out_pair[i];
    w.w_n = run(OP_PAIR_N, std::min(x, y), std::max(x, y), 1);
    w.w_sx = run(OP_PAIR_SUM, x, y, big ? 2 : 1);
    w.w_sy = run(OP_PAIR_SUM, y, x, big ? 2 : 1);
    w.w_sxx = run(OP_PAIR_SQ, x, y, big ? 4 : 2);
    w.w_syy = run(OP_PAIR_SQ, y, x, big ? 4 : 2);
    w.w_sxy = run(OP_PAIR_XY, std::min(x, y), std::max(x, y), big ? 4 : 2);
    if (w.w_n < 0 || w.w_sx < 0 || w.w_sy < 0 || w.w_sxx < 0 || w.w_syy < 0 || w.w_sxy < 0)
      return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
  }
  for (int i = 0; i < d.n_aggs; i++) {  // latest = MAX(seq), earliest = MIN(seq); no non-null count:
    if (off_hid[i] < 0) continue;       // the initial value itself says "no record yet"
    if (a->agg_k[i] > 0) continue;      // (the N forms: slots, below)
    const int h = off_hid[i];
    const bool latest = agg_base_kind(a->aggs[i].kind) == KHIP_AGG_LATEST_BY_OFFSET;
    int& w = latest ? w_max[h] : w_min[h];
    if (w < 0) w = word++;
    a->offs.a[a->out_off[i]].w_seq = (int16_t)w;
  }
  // TOPK / TOPKDISTINCT: per (kind, column, k) k consecutive words of order keys, sorted descending,
  // INT64_MIN = empty; TOPKDISTINCT over BIGINT one more, "Long.MIN_VALUE seen" (that value's key is
  // the empty slot's, so it never enters the slots)
  struct TopkSpan { int kind, col, k, word; };
  std::vector<TopkSpan> spans;
  std::vector<int> out_span(d.n_aggs, -1);
  a->out_flag.assign(d.n_aggs, -1);
  a->has_topk = false;
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = a->aggs[i];
    if (off_hid[i] >= 0 && a->agg_k[i] > 0) {
      // the N forms of the offset aggregates: "the last / first N records" = the N largest keys of
      // the hidden (complemented) sequence column, a TOPK span per (hidden column, N).  A key is
      // never INT64_MIN (seq >= 0, ~seq > INT64_MIN): the list's length is the leading non-empty
      // slots, no count word
      a->has_topk = true;
      const int k = a->agg_k[i];
      for (size_t j = 0; j < spans.size(); j++)
        if (spans[j].kind == KHIP_AGG_TOPK && spans[j].col == off_hid[i] && spans[j].k == k) out_span[i] = (int)j;
      if (out_span[i] < 0) {
        if (word + k > 32) return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
        out_span[i] = (int)spans.size();
        spans.push_back(TopkSpan{KHIP_AGG_TOPK, off_hid[i], k, word});
        word += k;
      }
      a->offs.a[a->out_off[i]].w_seq = (int16_t)spans[out_span[i]].word;
      continue;
    }
    if (!agg_is_topk(s.kind)) continue;
    a->has_topk = true;
    const int k = a->agg_k[i];
    for (size_t j = 0; j < spans.size(); j++)
      if (spans[j].kind == s.kind && spans[j].col == s.arg_col && spans[j].k == k) out_span[i] = (int)j;
    if (out_span[i] < 0) {
      const bool flag = s.kind == KHIP_AGG_TOPKDISTINCT && a->col_types[s.arg_col] == KHIP_TYPE_INT64;
      if (word + k + (flag ? 1 : 0) > 32) return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
      out_span[i] = (int)spans.size();
      spans.push_back(TopkSpan{s.kind, s.arg_col, k, word});
      word += k + (flag ? 1 : 0);
    }
    const TopkSpan& sp = spans[out_span[i]];
    if (s.kind == KHIP_AGG_TOPKDISTINCT && a->col_types[s.arg_col] == KHIP_TYPE_INT64) a->out_flag[i] = sp.word + sp.k;
  }
  if (word > 32) return fail(KHIP_E_UNSUPPORTED, "too many aggregate state words (max 29)");
  a->sw = (int)next_pow2(std::max(word, 4));
  ApplyParams& p = a->ap;
  p.windowed = a->windowed;
  p.slot_words = a->sw;
  p.size = d.size_ms;
  p.adv = d.advance_ms;
  p.grace = a->grace;
  p.n_cols = nc;
  for (int c = 0; c < nc; c++) p.col_type[c] = c < d.n_cols ? a->col_types[c] : KHIP_TYPE_INT64;
  int n = 0;
  auto add = [&](int8_t kind, int col, int w) {
    p.ops[n].kind = kind;
    p.ops[n].col = (int8_t)col;
    p.ops[n].word = (int16_t)w;
    n++;
  };
  if (w_star >= 0) add(OP_INC, 0, w_star);
  for (int c = 0; c < nc; c++) {
    if (w_cnt[c] >= 0) add(OP_INC_VALID, c, w_cnt[c]);
    if (w_sum[c] >= 0) add(p.col_type[c] == KHIP_TYPE_DOUBLE ? OP_ADD_F64 : OP_ADD_I64, c, w_sum[c]);
    if (w_hi[c] >= 0) add(OP_ADD_HI32, c, w_hi[c]);
    if (w_sq[c] >= 0)  // (op_word / op_slots: the limb index)
      for (int j = 0; j < (p.col_type[c] == KHIP_TYPE_INT64 ? 4 : 2); j++) add(OP_ADD_SQ, c, (w_sq[c] + j) | (j << 8));
    if (w_min[c] >= 0) add(OP_MIN, c, w_min[c]);
    if (w_max[c] >= 0) add(OP_MAX, c, w_max[c]);
  }
  for (const PairRun& r : pruns)  // (op_word / op_limb / op_col2 / op_big)
    for (int j = 0; j < r.limbs; j++)
      add((int8_t)r.kind, r.col,
          (r.word + j) | (j << 8) | (r.col2 << 11) | ((p.col_type[r.col] == KHIP_TYPE_INT64 ? 1 : 0) << 14));
  for (const TopkSpan& sp : spans)  // (op_word / op_slots)
    add(sp.kind == KHIP_AGG_TOPK ? OP_TOPK : OP_TOPK_DISTINCT, sp.col, sp.word | (sp.k << 8));
  p.n_ops = n;
  for (int w = 0; w < 32; w++) a->init.w[w] = 0;
  a->init.w[1] = EMPTY_WS;
  a->init.w[2] = INT64_MIN;
  for (int c = 0; c < nc; c++) {
    if (w_min[c] >= 0) a->init.w[w_min[c]] = INT64_MAX;
    if (w_max[c] >= 0) a->init.w[w_max[c]] = INT64_MIN;
  }
  for (const TopkSpan& sp : spans)  // (the flag word stays 0)
    for (int j = 0; j < sp.k; j++) a->init.w[sp.word + j] = INT64_MIN;
  a->outs.clear();
  a->out_var.assign(d.n_aggs, khip_agg::VarWords{});
  a->has_var = false;
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = a->aggs[i];
    AggOut o{};
    o.kind = agg_base_kind(s.kind);
    o.type = s.kind == KHIP_AGG_COUNT_STAR ? KHIP_TYPE_INT64 : a->col_types[s.arg_col];
    o.w_cnt = s.kind == KHIP_AGG_COUNT_STAR ? -1 : (agg_is_offset(s.kind) || agg_is_pair(s.kind) ? -1 : w_cnt[s.arg_col]);
    switch (o.kind) {
      case KHIP_AGG_COUNT_STAR: o.w_val = w_star; break;
      case KHIP_AGG_COUNT: o.w_val = w_cnt[s.arg_col]; break;
      case KHIP_AGG_SUM:
      case KHIP_AGG_AVG: o.w_val = w_sum[s.arg_col]; break;
      case KHIP_AGG_STDDEV_SAMP:
      case KHIP_AGG_STDDEV_SAMPLE:  // (decoded by emit_snapshot: variance_result)
        o.w_val = w_sum[s.arg_col];
        a->out_var[i].w_hi = w_hi[s.arg_col];
        a->out_var[i].w_sq = w_sq[s.arg_col];
        a->has_var = true;
        break;
      case KHIP_AGG_CORRELATION:  // (decoded by emit_snapshot: correlation_result over out_pair[i])
        o.w_val = a->out_pair[i].w_n;
        break;
      case KHIP_AGG_MIN: o.w_val = w_min[s.arg_col]; break;
      case KHIP_AGG_MAX: o.w_val = w_max[s.arg_col]; break;
      case KHIP_AGG_LATEST_BY_OFFSET:
      case KHIP_AGG_EARLIEST_BY_OFFSET: o.w_val = a->offs.a[a->out_off[i]].w_val; break;  // (decoded by emit_snapshot)
      case KHIP_AGG_TOPK:
      case KHIP_AGG_TOPKDISTINCT:  // the first slot word (decoded by emit_snapshot); TOPKDISTINCT has no count
        o.w_val = spans[out_span[i]].word;
        if (o.kind == KHIP_AGG_TOPKDISTINCT) o.w_cnt = -1;
        break;
    }
    a->outs.push_back(o);
  }
  return KHIP_OK;
}

static khip_status init_table(khip_agg* a, DevBuf& buf, int64_t cap) {
  KHIP_TRY(buf.ensure((size_t)cap * a->sw * 8));
  hipLaunchKernelGGL(k_init_table, dim3(grid_for(cap * a->sw, 256)), dim3(256), 0, a->stream,
                     buf.as<uint64_t>(), cap, a->sw, a->init);
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

khip_status khip::agg_grow_table(khip_agg* a, int64_t new_cap) {
  DevBuf nt;
  KHIP_TRY(init_table(a, nt, new_cap));
  if (a->cap > 0 && a->occ > 0) {
    hipLaunchKernelGGL(k_rehash, dim3(grid_for(a->cap, 256)), dim3(256), 0, a->stream, a->table.as<uint64_t>(),
                       a->cap, nt.as<uint64_t>(), (uint64_t)(new_cap - 1), a->sw,
                       a->desc.key_type == KHIP_KEY_UTF8 ? 1 : 0, a->dict.arena.as<uint8_t>());
    KHIP_TRY_HIP(hipGetLastError());
  }
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  a->table.release();
  a->table = std::move(nt);
  nt.p = nullptr;
  nt.bytes = 0;
  a->cap = new_cap;
  return KHIP_OK;
}

namespace khip {

int64_t visible_from(const khip_agg* a) {
  if (!a->windowed) return INT64_MIN;
  // PARTITION: every task's store expires by its own stream time (per row through the key map,
  // partition_bounds); the handle-wide bound is the smallest of the tasks' (what every task has
  // expired), INT64_MIN while some task has expired nothing
  if (a->desc.time_domain == KHIP_TIME_PARTITION) {
    if (a->pst_host.empty()) return INT64_MIN;
    int64_t m = INT64_MAX;
    for (int64_t t : a->pst_host) m = std::min(m, partition_vis_from(a, t));
    return m;
  }
  if (a->host_stream_time < 0) return INT64_MIN;
  const int64_t adv = a->desc.advance_ms;
  const int64_t vf = a->host_stream_time / adv * adv - a->retention;  // the store's observed time - retention
  return vf > 0 ? vf : INT64_MIN;  // window starts are >= 0: nothing has expired yet
}

// EMIT FINAL: the window starts this batch closes after they expired (k_emit_lost), computed from
// the batch alone before the engine runs; collected by finish_lost_seed() after the push's sync.
khip_status emit_final_lost(khip_agg* a, const int64_t* ts, const uint8_t* kv, const uint8_t* rv, int64_t n,
                            int64_t seed_st) {
  const int64_t nb = ceil_div(n, RPB);
  KHIP_TRY(a->blockmax.ensure(nb * 8));
  KHIP_TRY(a->blockprefix.ensure(nb * 8 + 8));
  KHIP_TRY(a->lostctr.ensure(16));
  if (a->lost_cap == 0) {
    a->lost_cap = 4096;
    KHIP_TRY(a->lostbuf.ensure((size_t)a->lost_cap * 16));
  }
  int64_t* seed = a->blockprefix.as<int64_t>() + nb;  // stream time before the batch
  KHIP_TRY(a->part.pinfo.ensure(sizeof(PushInfo)));
  int64_t* hs = &a->part.info()->seed_st;
  hs[0] = seed_st;  // the stream time before the batch
  KHIP_TRY_HIP(hipMemcpyAsync(seed, hs, 8, hipMemcpyHostToDevice, a->stream));
  KHIP_TRY_HIP(hipMemsetAsync(a->lostctr.p, 0, 8, a->stream));
  hipLaunchKernelGGL(k_blockmax, dim3(nb), dim3(BLOCK), 0, a->stream, ts, kv, rv, n, a->blockmax.as<int64_t>(),
                     (const int64_t*)nullptr);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, a->stream, a->blockmax.as<int64_t>(), nb,
                     a->blockprefix.as<int64_t>(), seed);
  hipLaunchKernelGGL(k_emit_lost, dim3(nb), dim3(BLOCK), 0, a->stream, ts, kv, rv, n, a->blockprefix.as<int64_t>(),
                     a->desc.size_ms, a->desc.advance_ms, a->grace, a->retention, a->lostbuf.as<int64_t>(), a->lost_cap,
                     a->lostctr.as<unsigned long long>());
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

// Sorted [lo, hi] pairs, overlapping or adjacent ones merged.
static std::vector<int64_t> merge_ranges(std::vector<std::pair<int64_t, int64_t>> r) {
  std::sort(r.begin(), r.end());
  std::vector<int64_t> out;
  for (auto& x : r) {
    if (!out.empty() && x.first <= out.back() + 1) {
      out.back() = std::max(out.back(), x.second);
    } else {
      out.push_back(x.first);
      out.push_back(x.second);
    }
  }
  return out;
}

// After the push's sync: the lost ranges → host (sorted, merged); re-run with room if the
// buffer overflowed (the batch is still valid: the caller owns it until the push returns).
static khip_status finish_lost_seed(khip_agg* a, const int64_t* ts, const uint8_t* kv, const uint8_t* rv, int64_t n,
                                   int64_t seed_st) {
  int64_t cnt = 0;
  KHIP_TRY_HIP(hipMemcpy(&cnt, a->lostctr.p, 8, hipMemcpyDeviceToHost));
  if (cnt > a->lost_cap) {
    a->lost_cap = next_pow2(cnt);
    a->lostbuf.release();
    KHIP_TRY(a->lostbuf.ensure((size_t)a->lost_cap * 16));
    KHIP_TRY(emit_final_lost(a, ts, kv, rv, n, seed_st));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
    KHIP_TRY_HIP(hipMemcpy(&cnt, a->lostctr.p, 8, hipMemcpyDeviceToHost));
  }
  std::vector<std::pair<int64_t, int64_t>> r((size_t)cnt);
  if (cnt) KHIP_TRY_HIP(hipMemcpy(r.data(), a->lostbuf.p, (size_t)cnt * 16, hipMemcpyDeviceToHost));
  a->lost = merge_ranges(std::move(r));
  return KHIP_OK;
}

}  // namespace khip

extern "C" {

khip_status khip_agg_result_type(const khip_agg_desc* d, int32_t i, int32_t* out) {
  if (!d || !out || i < 0 || i >= d->n_aggs) return fail(KHIP_E_INVALID, "bad aggregate index");
  const khip_agg_spec& s = d->aggs[i];
  if (s.kind == KHIP_AGG_COUNT_STAR || s.kind == KHIP_AGG_COUNT) *out = KHIP_TYPE_INT64;
  else if (s.kind == KHIP_AGG_AVG || agg_is_var(s.kind) || agg_is_pair(s.kind)) *out = KHIP_TYPE_DOUBLE;
  else *out = d->col_types[s.arg_col];  // (TOPK / TOPKDISTINCT: the element type)
  return KHIP_OK;
}

khip_status khip_agg_result_len(const khip_agg_desc* d, int32_t i, int32_t* out) {
  if (!d || !out || i < 0 || i >= d->n_aggs) return fail(KHIP_E_INVALID, "bad aggregate index");
  const khip_agg_spec& s = d->aggs[i];
  // (the N forms of LATEST / EARLIEST_BY_OFFSET: N; their scalar forms carry no k bits)
  *out = (agg_is_topk(s.kind) || agg_is_offset(s.kind)) ? std::max(agg_k_bits(s.kind), 1) : 1;
  return KHIP_OK;
}

khip_status khip_agg_create(const khip_agg_desc* desc, khip_agg** out) {
  clear_error();
  if (!desc || !out) return fail(KHIP_E_INVALID, "null argument");
  const khip_agg_desc& d = *desc;
  if (d.window_kind < KHIP_WINDOW_NONE || d.window_kind > KHIP_WINDOW_SESSION)
    return fail(KHIP_E_INVALID, "unknown window kind");
  if (d.window_kind != KHIP_WINDOW_NONE) {
    if (d.size_ms <= 0) return fail(KHIP_E_INVALID, "window size must be > 0");
    if (d.window_kind == KHIP_WINDOW_HOPPING && (d.advance_ms <= 0 || d.advance_ms > d.size_ms))
      return fail(KHIP_E_INVALID, "hopping advance must be in (0, size]");
  }
  if (d.key_type != KHIP_KEY_INT64 && d.key_type != KHIP_KEY_UTF8) return fail(KHIP_E_INVALID, "key type");
  if (d.n_cols < 0 || d.n_cols > MAX_COLS) return fail(KHIP_E_UNSUPPORTED, "at most 8 value columns");
  if (d.n_aggs < 0 || d.n_aggs > 16) return fail(KHIP_E_UNSUPPORTED, "at most 16 aggregates");
  for (int c = 0; c < d.n_cols; c++)
    if (d.col_types[c] < KHIP_TYPE_INT32 || d.col_types[c] > KHIP_TYPE_DOUBLE)
      return fail(KHIP_E_INVALID, "column type");
  bool has_offset = false, has_topk = false;
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = d.aggs[i];
    const int bk = agg_base_kind(s.kind);
    if (bk < KHIP_AGG_COUNT_STAR || bk > KHIP_AGG_CORRELATION) return fail(KHIP_E_INVALID, "aggregate kind");
    if ((s.kind & KHIP_AGG_KEEP_NULLS) && !agg_is_offset(s.kind))
      return fail(KHIP_E_INVALID, "KHIP_AGG_KEEP_NULLS on an aggregate other than LATEST / EARLIEST_BY_OFFSET");
    if (agg_is_offset(s.kind)) {  // no k bits: the scalar form; N >= 1: the N form (an ARRAY, also for N = 1)
      if (agg_k_bits(s.kind) < 0)
        return fail(KHIP_E_INVALID, "LATEST / EARLIEST_BY_OFFSET: N (KHIP_AGG_K) must be at least 1");
    } else if (agg_is_pair(s.kind)) {  // KHIP_AGG_ARG2: the second argument column in the k bits
      if (agg_k_bits(s.kind) < 0 || agg_k_bits(s.kind) >= d.n_cols)
        return fail(KHIP_E_INVALID, "CORRELATION: second argument column (KHIP_AGG_ARG2)");
    } else if (agg_is_topk(s.kind) ? agg_k_bits(s.kind) < 1 : agg_k_bits(s.kind) != 0)
      return fail(KHIP_E_INVALID, agg_is_topk(s.kind)
                                      ? "TOPK / TOPKDISTINCT: k (KHIP_AGG_K) must be at least 1"
                                      : "KHIP_AGG_K on an aggregate other than TOPK / TOPKDISTINCT / the offset kinds");
    if (bk != KHIP_AGG_COUNT_STAR && (s.arg_col < 0 || s.arg_col >= d.n_cols))
      return fail(KHIP_E_INVALID, "aggregate argument column");
    has_offset = has_offset || agg_is_offset(s.kind);
    has_topk = has_topk || agg_is_topk(s.kind);
    if (agg_is_var(s.kind)) {
      // a DOUBLE argument: no order-free state reproduces the reference's fold within a bound that
      // does not depend on the data's mean and spread
      if (d.col_types[s.arg_col] == KHIP_TYPE_DOUBLE)
        return fail(KHIP_E_UNSUPPORTED, "STDDEV_SAMP / STDDEV_SAMPLE of a DOUBLE column");
      // the reference's session merge divides the integer sums with integer division
      // (StandardDeviationSampUdaf.java:68-71): its merged sessions are not the variance of the union
      if (d.window_kind == KHIP_WINDOW_SESSION)
        return fail(KHIP_E_UNSUPPORTED, "STDDEV_SAMP / STDDEV_SAMPLE with SESSION windows");
      if (d.has_having && d.having.agg_index == i)
        return fail(KHIP_E_UNSUPPORTED, "HAVING on a STDDEV_SAMP / STDDEV_SAMPLE aggregate");
    }
  }
  for (int i = 0; i < d.n_aggs; i++) {
    const khip_agg_spec& s = d.aggs[i];
    if (!agg_is_pair(s.kind)) continue;
    const int tx = d.col_types[s.arg_col], ty = d.col_types[agg_k_bits(s.kind)];
    // a DOUBLE argument: the reference's one-pass formula cancels (CorrelationUdaf.java:127-133), so
    // no order-free state reproduces its fold within a bound that does not depend on the data
    if (tx == KHIP_TYPE_DOUBLE || ty == KHIP_TYPE_DOUBLE)
      return fail(KHIP_E_UNSUPPORTED, "CORRELATION of a DOUBLE column");
    if (tx != ty) return fail(KHIP_E_UNSUPPORTED, "CORRELATION of an INT and a BIGINT column (cast one)");
    if (d.window_kind == KHIP_WINDOW_SESSION) return fail(KHIP_E_UNSUPPORTED, "CORRELATION with SESSION windows");
    if (d.has_having && d.having.agg_index == i) return fail(KHIP_E_UNSUPPORTED, "HAVING on a CORRELATION aggregate");
  }
  if (has_topk) {
    // merged list by list (TopkKudaf.merge) in the reference: not on the device
    if (d.window_kind == KHIP_WINDOW_SESSION) return fail(KHIP_E_UNSUPPORTED, "TOPK / TOPKDISTINCT with SESSION windows");
    // Udafs, not TableUdafs (no undo): the reference rejects them on a table source as it rejects MIN/MAX
    if (d.flags & KHIP_FLAG_TABLE_SOURCE)
      return fail(KHIP_E_UNSUPPORTED, "TOPK / TOPKDISTINCT cannot be applied to a table source");
    if (d.has_having && d.having.agg_index >= 0 && d.having.agg_index < d.n_aggs &&
        agg_is_topk(d.aggs[d.having.agg_index].kind))
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a TOPK / TOPKDISTINCT aggregate (an ARRAY)");
  }
  if (has_offset) {
    // merged by sequence (Udaf.merge) in the reference: not on the device
    if (d.window_kind == KHIP_WINDOW_SESSION)
      return fail(KHIP_E_UNSUPPORTED, "LATEST / EARLIEST_BY_OFFSET with SESSION windows");
    // not TableUdafs: the reference rejects them on a table source as it rejects MIN/MAX
    if (d.flags & KHIP_FLAG_TABLE_SOURCE)
      return fail(KHIP_E_UNSUPPORTED, "LATEST / EARLIEST_BY_OFFSET cannot be applied to a table source");
    if (d.has_having && d.having.agg_index >= 0 && d.having.agg_index < d.n_aggs &&
        agg_is_offset(d.aggs[d.having.agg_index].kind))
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a LATEST / EARLIEST_BY_OFFSET aggregate");
  }
  if (d.emit != KHIP_EMIT_CHANGES && d.emit != KHIP_EMIT_FINAL) return fail(KHIP_E_INVALID, "emit strategy");
  if (d.flags & KHIP_FLAG_TABLE_SOURCE) {  // table aggregation: undoable aggregates, no windows
    if (d.window_kind != KHIP_WINDOW_NONE) return fail(KHIP_E_UNSUPPORTED, "windowed aggregation of a table source");
    for (int i = 0; i < d.n_aggs; i++)
      if (d.aggs[i].kind == KHIP_AGG_MIN || d.aggs[i].kind == KHIP_AGG_MAX)  // E/structured/SchemaKGroupedTable.java:82-95
        return fail(KHIP_E_UNSUPPORTED, "MIN/MAX cannot be applied to a table source, only to a stream source");
    if (d.flags & KHIP_FLAG_CHANGELOG) return fail(KHIP_E_UNSUPPORTED, "changelog of a table-source aggregation");
  }
  if (d.emit == KHIP_EMIT_FINAL && d.window_kind == KHIP_WINDOW_NONE)
    return fail(KHIP_E_INVALID, "EMIT FINAL needs a windowed aggregation");
  if (d.window_kind != KHIP_WINDOW_NONE && d.retention_ms != KHIP_RETENTION_DEFAULT) {
    // TimeWindowedKStreamImpl: retention < size + grace is an IllegalArgumentException
    const int64_t g = grace_of(d);
    if (d.retention_ms < 0 || d.retention_ms < d.size_ms + g)
      return fail(KHIP_E_INVALID, "retention must be at least window size + grace");
  }
  if (d.time_domain < KHIP_TIME_TASK || d.time_domain > KHIP_TIME_SUPPLIED) return fail(KHIP_E_INVALID, "time domain");
  if (d.time_domain != KHIP_TIME_TASK) {
    // SESSION windows take the SUPPLIED (GLOBAL) stream time with EMIT CHANGES: the replay reads
    // each row's given stream time.  EMIT FINAL needs the stream time BEFORE each row, which the
    // shuffle does not carry; PARTITION needs per-task session expiry.
    if (d.window_kind == KHIP_WINDOW_SESSION && (d.time_domain == KHIP_TIME_PARTITION || d.emit == KHIP_EMIT_FINAL))
      return fail(KHIP_E_UNSUPPORTED, "SESSION windows: PARTITION stream time, or EMIT FINAL under SUPPLIED");
    if (d.flags & KHIP_FLAG_TABLE_SOURCE) return fail(KHIP_E_UNSUPPORTED, "stream-time domains of a table source");
    if (d.time_domain == KHIP_TIME_PARTITION && (d.n_partitions < 1 || d.n_partitions > 65536))
      return fail(KHIP_E_INVALID, "n_partitions must be in [1, 65536]");
  }
  if (d.has_having) {
    if (d.having.agg_index < 0 || d.having.agg_index >= d.n_aggs) return fail(KHIP_E_INVALID, "having agg index");
    if (d.having.op < KHIP_OP_GT || d.having.op > KHIP_OP_NE) return fail(KHIP_E_INVALID, "having op");
  }
  khip_agg* a = new khip_agg();
  a->desc = d;
  a->col_types.assign(d.col_types, d.col_types + d.n_cols);
  a->aggs.assign(d.aggs, d.aggs + d.n_aggs);
  a->agg_k.assign(d.n_aggs, 0);
  for (int i = 0; i < d.n_aggs; i++) {  // the handle's specs keep the bare kind (and KEEP_NULLS); k apart
    a->agg_k[i] = agg_k_bits(a->aggs[i].kind);
    a->aggs[i].kind &= 0xFFFF;
  }
  a->desc.col_types = a->col_types.data();
  a->desc.aggs = a->aggs.data();
  if (d.window_kind == KHIP_WINDOW_TUMBLING || d.window_kind == KHIP_WINDOW_SESSION) a->desc.advance_ms = d.size_ms;
  a->windowed = d.window_kind != KHIP_WINDOW_NONE;
  a->grace = grace_of(a->desc);
  a->max_fanout = a->windowed ? (int)ceil_div(a->desc.size_ms, a->desc.advance_ms) : 1;
  if (a->windowed && ceil_div(a->desc.size_ms, a->desc.advance_ms) > MAX_FANOUT) {
    delete a;
    return fail(KHIP_E_UNSUPPORTED, "hopping fan-out above 4095 windows per record");
  }
  a->device = d.device;
  khip_status st = plan_state(a);
  if (st != KHIP_OK) {
    delete a;
    return st;
  }
  if (d.has_having) {
    a->having.active = 1;
    a->having.op = d.having.op;
    a->having.a = a->outs[d.having.agg_index];
    a->having.i64 = d.having.i64;
    a->having.f64 = d.having.f64;
  }
  DeviceGuard g(a->device);
  if (hipStreamCreateWithFlags(&a->stream, hipStreamDefault) != hipSuccess) {
    delete a;
    return fail(KHIP_E_DEVICE, "hipStreamCreate failed (no device?)");
  }
  a->profile = (d.flags & KHIP_FLAG_PROFILE) != 0;
  a->engine = d.window_kind == KHIP_WINDOW_SESSION ? 2
              : (d.flags & KHIP_FLAG_TABLE_SOURCE) ? 3
              : ((d.flags & KHIP_FLAG_ENGINE_ATOMIC) ? 1 : 0);
  a->changelog = (d.flags & KHIP_FLAG_CHANGELOG) != 0 && d.emit == KHIP_EMIT_CHANGES;
  if (a->windowed)
    a->retention = d.retention_ms == KHIP_RETENTION_DEFAULT ? a->desc.size_ms + a->grace : d.retention_ms;
  if (a->changelog && a->engine == 1) {  // (SESSION windows keep their changelog themselves)
    khip_agg_destroy(a);
    return fail(KHIP_E_UNSUPPORTED, "EMIT CHANGES changelog needs the partitioned engine");
  }
  if (a->profile)
    // timing only (KHIP_FLAG_PROFILE): no system-scope fence at each event — with it every
    // event wrote back and invalidated the L2 (≈ 54 µs per C2 push over its 4-5 events)
    for (int e = 0; e < 8; e++) hipEventCreateWithFlags(&a->ev[e], hipEventDisableSystemFence);
  int64_t cap = (a->engine == 1 || a->engine == 3) ? next_pow2(std::max<int64_t>(1024, d.capacity_hint > 0 ? d.capacity_hint * 2 : 1 << 16))
                                : 1024;
  if ((st = init_table(a, a->table, cap)) != KHIP_OK || (st = a->stream_time.ensure(8)) != KHIP_OK ||
      (st = a->counters.ensure(8 * NPART)) != KHIP_OK ||
      (a->engine == 0 && (st = part_init(a, d.capacity_hint > 0 ? d.capacity_hint : (1 << 20))) != KHIP_OK)) {
    khip_agg_destroy(a);
    return st;
  }
  a->cap = cap;
  int64_t m1 = -1;
  hipMemcpyAsync(a->stream_time.p, &m1, 8, hipMemcpyHostToDevice, a->stream);
  if (d.time_domain == KHIP_TIME_PARTITION) {  // every partition's stream time: none yet
    if ((st = a->pst.ensure((size_t)d.n_partitions * 8)) != KHIP_OK ||
        (st = a->pst2.ensure((size_t)d.n_partitions * 8)) != KHIP_OK) {
      khip_agg_destroy(a);
      return st;
    }
    hipMemsetAsync(a->pst.p, 0xFF, (size_t)d.n_partitions * 8, a->stream);
  }
  if (d.key_type == KHIP_KEY_UTF8) {
    if ((st = dict_init(a->dict, a->stream)) != KHIP_OK) {
      khip_agg_destroy(a);
      return st;
    }
  }
  if (hipStreamSynchronize(a->stream) != hipSuccess) {
    khip_agg_destroy(a);
    return fail(KHIP_E_DEVICE, "device init failed");
  }
  *out = a;
  return KHIP_OK;
}

static khip_status stage(khip_agg* a, DevBuf& buf, const void* src, size_t bytes) {
  KHIP_TRY(buf.ensure(bytes));
  if (bytes) KHIP_TRY_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, a->stream));
  return KHIP_OK;
}

// The device-side view of one batch: what the push's stages hand to each other.  It lives on the
// entry point's stack; resolve_batch fills the columns, the later stages the rest.
struct BatchIn {
  int64_t n = 0;
  const int64_t* keys = nullptr;   // GROUP BY keys: the INT64 column, or the UTF8 keys' ids (key_ids)
  const int64_t* hkeys = nullptr;  // what the hashing engines hash: keys, or the UTF8 keys' hashes
  const int64_t* ts = nullptr;
  const uint8_t *kv = nullptr, *rv = nullptr;
  const int64_t* koff = nullptr;  // UTF8 keys: offsets[n + 1] into kbytes
  const uint8_t* kbytes = nullptr;
  int64_t key_bytes_total = 0;    // = koff[n] (a device batch: valid after the next synchronisation)
  ColPtrs cols{};                 // the user columns, then the hidden sequence columns
  const int64_t* st_at = nullptr;  // ABI 5 domains: the stream time observed at every row
  const int32_t* part = nullptr;   // KHIP_TIME_PARTITION: every row's source partition
};

// n, ts, key_valid and row_valid of a batch: a host batch's are staged into the handle's buffers
// (asynchronously, on its stream), a device batch's are used where they lie.
static khip_status stage_ts_valid(khip_agg* a, const khip_batch* b, BatchIn& in) {
  in.n = b->n_rows;
  in.ts = b->ts;
  in.kv = b->key_valid;
  in.rv = b->row_valid;
  if (b->mem == KHIP_MEM_DEVICE) return KHIP_OK;
  if (b->mem != KHIP_MEM_HOST) return fail(KHIP_E_INVALID, "batch mem");
  const size_t bm = (size_t)(in.n + 7) / 8;
  KHIP_TRY(stage(a, a->st_ts, b->ts, in.n * 8));
  in.ts = a->st_ts.as<int64_t>();
  if (in.kv) { KHIP_TRY(stage(a, a->st_kv, in.kv, bm)); in.kv = a->st_kv.as<uint8_t>(); }
  if (in.rv) { KHIP_TRY(stage(a, a->st_rv, in.rv, bm)); in.rv = a->st_rv.as<uint8_t>(); }
  return KHIP_OK;
}

// The batch's device pointers: host batches are staged into the handle's buffers (asynchronously,
// on its stream); UTF8 key byte totals of device batches are fetched (synchronise before use).
static khip_status resolve_batch(khip_agg* a, const khip_batch* b, BatchIn& in) {
  KHIP_TRY(stage_ts_valid(a, b, in));
  const int64_t n = in.n;
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8;
  in.keys = b->key_i64;
  in.koff = b->key_offsets;
  in.kbytes = b->key_bytes;
  if (b->mem == KHIP_MEM_HOST) {
    if (utf8) {
      in.key_bytes_total = b->key_offsets[n];
      KHIP_TRY(stage(a, a->st_koff, b->key_offsets, (n + 1) * 8));
      KHIP_TRY(stage(a, a->st_kbytes, b->key_bytes, (size_t)std::max<int64_t>(in.key_bytes_total, 1)));
      in.koff = a->st_koff.as<int64_t>();
      in.kbytes = a->st_kbytes.as<uint8_t>();
    } else {
      KHIP_TRY(stage(a, a->st_keys, b->key_i64, n * 8));
      in.keys = a->st_keys.as<int64_t>();
    }
    const size_t bm = (size_t)(n + 7) / 8;
    for (int c = 0; c < a->desc.n_cols; c++) {
      const size_t es = a->col_types[c] == KHIP_TYPE_INT32 ? 4 : 8;
      KHIP_TRY(stage(a, a->st_cols[c], b->col_data[c], n * es));
      in.cols.data[c] = a->st_cols[c].p;
      const uint8_t* cv = b->col_valid ? b->col_valid[c] : nullptr;
      if (cv) {
        KHIP_TRY(stage(a, a->st_cval[c], cv, bm));
        in.cols.valid[c] = a->st_cval[c].as<uint8_t>();
      }
    }
  } else {
    for (int c = 0; c < a->desc.n_cols; c++) {
      in.cols.data[c] = b->col_data[c];
      in.cols.valid[c] = b->col_valid ? b->col_valid[c] : nullptr;
    }
    if (utf8)
      KHIP_TRY_HIP(hipMemcpyAsync(&in.key_bytes_total, in.koff + n, 8, hipMemcpyDeviceToHost, a->stream));
  }
  in.hkeys = in.keys;
  return KHIP_OK;
}

// UTF8 GROUP BY keys → stable key ids (in.keys) through the handle's dictionary, with the key hashes
// (in.hkeys) when want_hash: they only feed the slot hashing of the global-atomic table (the other
// engines hash the ids).  timed: synchronise first (a device batch's key_bytes_total) and bracket the
// map with the profile events 1 and 2; khip_agg_push_table has synchronised already and times nothing.
static khip_status key_ids(khip_agg* a, BatchIn& in, bool want_hash, bool timed) {
  if (timed) {
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
    ev_record(a, 1);
  }
  KHIP_TRY(a->kid.ensure(in.n * 8));
  if (want_hash) KHIP_TRY(a->khash.ensure(in.n * 8));
  KHIP_TRY(dict_map(a->dict, a->stream, in.koff, in.kbytes, in.key_bytes_total, in.kv, in.rv, in.ts, in.n,
                    a->kid.as<int64_t>(), want_hash ? a->khash.as<int64_t>() : nullptr));
  in.keys = a->kid.as<int64_t>();
  in.hkeys = want_hash ? a->khash.as<int64_t>() : in.keys;
  if (timed) ev_record(a, 2);
  return KHIP_OK;
}

// A push's statistics from its counters tot[P_*] (null: an empty push, every count 0).  The table
// aggregation fills neither dropped_null_row nor windows_late.
static void put_stats(const khip_agg* a, int64_t rows_in, const int64_t* tot, bool table_source,
                      khip_batch_stats* stats) {
  if (!stats) return;
  khip_batch_stats s{};
  s.rows_in = rows_in;
  if (tot) {
    s.rows_accepted = tot[P_ACCEPTED];
    s.dropped_null_key = tot[P_NULL_KEY];
    if (!table_source) s.dropped_null_row = tot[P_NULL_ROW];
    s.dropped_bad_ts = tot[P_BAD_TS];
    s.windows_applied = tot[P_APPLIED];
    if (!table_source) s.windows_late = tot[P_LATE];
  }
  s.stream_time = a->host_stream_time;
  *stats = s;
}

// KHIP_FLAG_PROFILE, partitioned engine: a push's phase times from the events its last part_push /
// part_push_rows left, its records and its one apply launch.  dict: the key dictionary's time too
// (events 1-2 of key_ids).
static void part_profile(khip_agg* a, int64_t n, bool dict) {
  if (!a->profile) return;
  a->times.stream_time_ms += ev_ms(a, 3, 4);
  a->times.partition_ms += ev_ms(a, 4, 5);
  a->times.apply_ms += ev_ms(a, 5, 6);
  if (dict) a->times.dict_ms += ev_ms(a, 1, 2);
  a->times.records += n;
  a->times.apply_launches++;
}

// Retention, partitioned engine: drop expired windows from the closed store.  bounds: under
// KHIP_TIME_PARTITION each row expires by its own task's bound (partition_bounds).
static khip_status purge_expired(khip_agg* a, bool bounds) {
  if (!a->windowed) return KHIP_OK;
  HavingDev vis{};
  vis.vis = 1;
  vis.vis_from = visible_from(a);
  if (vis.vis_from == INT64_MIN) return KHIP_OK;
  if (bounds) KHIP_TRY(partition_bounds(a, vis));
  return part_purge_closed(a, vis);
}

// The resolve kernels' argument for rows [base, base + rows) of the sequence: the handle's offset
// aggregates and the push's (or slice's) user columns.
static OffResolve off_query(const khip_agg* a, const ColPtrs& cols, int64_t base, int64_t rows) {
  OffResolve q = a->offs;
  for (int c = 0; c < a->desc.n_cols; c++) {
    q.data[c] = cols.data[c];
    q.valid[c] = cols.valid[c];
  }
  q.base = base;
  q.rows = rows;
  return q;
}

// KHIP_TIME_SUPPLIED with a close context: the handle's stream time becomes the GLOBAL one after the
// batch (closing windows and retention as one task over the whole stream).
static khip_status supplied_advance(khip_agg* a) {
  if (a->sup_after > a->host_stream_time) {
    a->host_stream_time = a->sup_after;
    KHIP_TRY(a->part.pinfo.ensure(sizeof(PushInfo)));
    int64_t* hs = &a->part.info()->sup_after;
    hs[0] = a->sup_after;
    KHIP_TRY_HIP(hipMemcpyAsync(a->stream_time.p, hs, 8, hipMemcpyHostToDevice, a->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  }
  return KHIP_OK;
}

// ABI 6.  Received shuffle rows into the aggregation: the value pipeline reads them where they lie
// (khip_agg_c1.hip, RowsIn); any other push unpacks them into the handle's staging columns and runs
// as a device batch.  Same results and statistics as khip_agg_push of the unpacked batch.
khip_status khip_agg_push_shuffled(khip_agg* a, const khip_shuffle* sh, const uint64_t* rows, int64_t n,
                                   khip_batch_stats* stats) {
  clear_error();
  if (!a || !sh || (n > 0 && !rows)) return fail(KHIP_E_INVALID, "null argument");
  if (n < 0) return fail(KHIP_E_INVALID, "row count");
  int kc = 0, nc = 0;
  const int32_t* types = nullptr;
  shuffle_layout(sh, &kc, &nc, &types);
  if (nc != a->desc.n_cols) return fail(KHIP_E_INVALID, "the shuffle's columns are not the aggregation's");
  for (int c = 0; c < nc; c++)
    if (types[c] != a->col_types[c]) return fail(KHIP_E_INVALID, "the shuffle's column types are not the aggregation's");
  if (a->desc.key_type == KHIP_KEY_UTF8) return fail(KHIP_E_UNSUPPORTED, "shuffled rows carry an integer GROUP BY key");
  if (a->engine == 3) return fail(KHIP_E_STATE, "table-source aggregation: use khip_agg_push_table");
  if (a->desc.time_domain == KHIP_TIME_PARTITION)
    return fail(KHIP_E_UNSUPPORTED, "KHIP_TIME_PARTITION: received rows carry no source partition");
  if (a->offs.n) return fail(KHIP_E_UNSUPPORTED, "LATEST / EARLIEST_BY_OFFSET: shuffled rows carry no arrival order");
  const bool sup = a->desc.time_domain == KHIP_TIME_SUPPLIED;
  const int rw = khip_shuffle_row_words(sh);
  if (sup && rw != 3 + nc)
    return fail(KHIP_E_INVALID, "KHIP_TIME_SUPPLIED: the shuffle carries no stream time (KHIP_SHUFFLE_STREAM_TIME)");
  DeviceGuard g(a->device);
  if (n > 0 && n < (1LL << 31) && a->engine == 0 && a->desc.emit != KHIP_EMIT_FINAL) {
    // (the pipeline's push: no SUPPLIED close context is consumed, no dictionary, no PARTITION domain)
    a->st_before = a->host_stream_time;
    a->chg_ready = false;
    a->lost.clear();
    int64_t tot[NPART] = {0};
    bool done = false;
    KHIP_TRY(part_push_rows(a, n, RowsIn{rows, rw, 0, 0}, kc, tot, &done, sup));
    if (done) {
      a->occ += tot[P_NEW];
      part_profile(a, n, false);
      KHIP_TRY(purge_expired(a, false));
      put_stats(a, n, tot, false, stats);
      return KHIP_OK;
    }
  }
  // the rows as columns (the staging buffers: a device batch never uses them)
  const size_t bm = (size_t)(n + 7) / 8;
  KHIP_TRY(a->st_keys.ensure((size_t)std::max<int64_t>(n, 1) * 8));
  KHIP_TRY(a->st_ts.ensure((size_t)std::max<int64_t>(n, 1) * 8));
  void* cd[MAX_COLS] = {};
  uint8_t* cv[MAX_COLS] = {};
  for (int c = 0; c < nc; c++) {
    KHIP_TRY(a->st_cols[c].ensure((size_t)std::max<int64_t>(n, 1) * 8));
    KHIP_TRY(a->st_cval[c].ensure(std::max<size_t>(bm, 1)));
    cd[c] = a->st_cols[c].p;
    cv[c] = a->st_cval[c].as<uint8_t>();
  }
  if (n > 0)
    KHIP_TRY(khip_shuffle_unpack(const_cast<khip_shuffle*>(sh), rows, n, a->st_keys.as<int64_t>(), a->st_ts.as<int64_t>(),
                                 cd, cv));
  khip_batch b{};
  if (sup) {  // the GLOBAL stream time each row was routed with
    KHIP_TRY(a->st_col.ensure((size_t)std::max<int64_t>(n, 1) * 8));
    if (n > 0) KHIP_TRY(khip_shuffle_unpack_stream_time(const_cast<khip_shuffle*>(sh), rows, n, a->st_col.as<int64_t>()));
    b.stream_time = a->st_col.as<int64_t>();
  }
  b.mem = KHIP_MEM_DEVICE;
  b.n_rows = n;
  b.n_cols = nc;
  b.key_i64 = a->st_keys.as<int64_t>();
  b.ts = a->st_ts.as<int64_t>();
  b.col_data = (const void* const*)cd;
  b.col_valid = (const uint8_t* const*)cv;
  return khip_agg_push(a, &b, stats);
}

khip_status khip_agg_push_table(khip_agg* a, const khip_batch* b, const khip_table_src* src,
                                khip_batch_stats* stats) {
  clear_error();
  if (!a || !b || !src) return fail(KHIP_E_INVALID, "null argument");
  if (a->engine != 3) return fail(KHIP_E_STATE, "handle not created with KHIP_FLAG_TABLE_SOURCE");
  if (b->n_rows < 0 || b->n_cols < a->desc.n_cols) return fail(KHIP_E_INVALID, "batch shape");
  if (src->key_type != KHIP_KEY_INT64 && src->key_type != KHIP_KEY_UTF8) return fail(KHIP_E_INVALID, "source key type");
  TaggState& T = a->tagg;
  if (T.key_type >= 0 && T.key_type != src->key_type) return fail(KHIP_E_INVALID, "source key type changed");
  const int64_t n = b->n_rows;
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8, src_utf8 = src->key_type == KHIP_KEY_UTF8;
  if (n > 0) {
    if (!b->ts || (utf8 ? (!b->key_offsets || !b->key_bytes) : !b->key_i64))
      return fail(KHIP_E_INVALID, "missing GROUP BY key or timestamp column");
    if (src_utf8 ? (!src->key_offsets || !src->key_bytes) : !src->key_i64)
      return fail(KHIP_E_INVALID, "missing source PRIMARY KEY column");
    for (int c = 0; c < a->desc.n_cols; c++)
      if (!b->col_data || !b->col_data[c]) return fail(KHIP_E_INVALID, "missing value column");
  }
  DeviceGuard g(a->device);
  if (T.key_type < 0) {
    if (src_utf8) KHIP_TRY(dict_init(T.dict, a->stream));
    T.key_type = src->key_type;
  }
  a->chg_ready = false;
  if (n == 0) {
    put_stats(a, 0, nullptr, true, stats);
    return KHIP_OK;
  }
  BatchIn in;
  KHIP_TRY(resolve_batch(a, b, in));
  // the source PRIMARY KEYs on the device
  const int64_t* sk = src->key_i64;
  const int64_t* skoff = src->key_offsets;
  const uint8_t* skb = src->key_bytes;
  const uint8_t* skv = src->key_valid;
  int64_t src_bytes = 0;
  if (b->mem == KHIP_MEM_HOST) {
    const size_t bm = (size_t)(n + 7) / 8;
    if (skv) { KHIP_TRY(stage(a, T.st_kv, skv, bm)); skv = T.st_kv.as<uint8_t>(); }
    if (src_utf8) {
      src_bytes = src->key_offsets[n];
      KHIP_TRY(stage(a, T.st_koff, src->key_offsets, (n + 1) * 8));
      KHIP_TRY(stage(a, T.st_kbytes, src->key_bytes, (size_t)std::max<int64_t>(src_bytes, 1)));
      skoff = T.st_koff.as<int64_t>();
      skb = T.st_kbytes.as<uint8_t>();
    } else {
      KHIP_TRY(stage(a, T.st_key, src->key_i64, n * 8));
      sk = T.st_key.as<int64_t>();
    }
  } else if (src_utf8) {
    KHIP_TRY_HIP(hipMemcpyAsync(&src_bytes, skoff + n, 8, hipMemcpyDeviceToHost, a->stream));
  }
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));  // key byte totals of device batches
  // GROUP BY keys → ids (UTF8: the group dictionary; rows that cannot add to a group are skipped)
  if (utf8) KHIP_TRY(key_ids(a, in, true, false));
  if (src_utf8) {
    KHIP_TRY(T.sid.ensure(n * 8));
    KHIP_TRY(T.shash.ensure(n * 8));
    KHIP_TRY(dict_map(T.dict, a->stream, skoff, skb, src_bytes, skv, nullptr, in.ts, n, T.sid.as<int64_t>(),
                      T.shash.as<int64_t>()));
    sk = T.sid.as<int64_t>();
  }
  int64_t tot[NPART] = {0};
  KHIP_TRY(tagg_push(a, n, in.keys, in.hkeys, in.kv, in.rv, in.ts, in.cols, sk, skv, tot));
  put_stats(a, n, tot, true, stats);
  return KHIP_OK;
}

// Offset aggregates after one partitioned push slice (cols: the slice's columns; its sequence
// numbers are [base, base + m)): the partitions the slice reached, and the rows it appended to the
// closed store (a window can be updated and closed by the same push).
static khip_status off_resolve_part(khip_agg* a, const ColPtrs& cols, int64_t base, int64_t m, int64_t closed0) {
  PartState& s = a->part;
  const OffResolve q = off_query(a, cols, base, m);
  const bool lists = off_has_lists(q);  // (an N form: the kernels' list code)
  auto rpart = lists ? k_off_resolve_part<true> : k_off_resolve_part<false>;
  auto rrows = lists ? k_off_resolve_rows<true> : k_off_resolve_rows<false>;
  hipLaunchKernelGGL(rpart, dim3((unsigned)s.P), dim3(256), 0, a->stream, s.buf[0].as<uint64_t>(),
                     s.buf[1].as<uint64_t>(), s.sel.as<uint8_t>(), s.cnt.as<int64_t>(), s.cmax, a->sw,
                     s.pbase.as<int64_t>(), s.last_c1 ? s.prn.as<uint32_t>() : (const uint32_t*)nullptr, q);
  if (s.closed_n > closed0)
    hipLaunchKernelGGL(rrows, dim3(grid_for(s.closed_n - closed0, 256, 4096)), dim3(256), 0, a->stream,
                       s.closed.as<uint64_t>(), closed0, s.closed_n, a->sw, q);
  KHIP_TRY_HIP(hipGetLastError());
  // the caller's columns (and a host batch's staging copies) are only valid until the push returns
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  return KHIP_OK;
}

// ---- khip_agg_push: its stages, in the order they run

static khip_status push_check(const khip_agg* a, const khip_batch* b) {
  if (!a || !b) return fail(KHIP_E_INVALID, "null argument");
  if (b->n_rows < 0 || b->n_cols < a->desc.n_cols) return fail(KHIP_E_INVALID, "batch shape");
  if (b->n_rows >= (1LL << 36)) return fail(KHIP_E_UNSUPPORTED, "batch larger than 2^36 rows");
  if (a->engine == 3) return fail(KHIP_E_STATE, "table-source aggregation: use khip_agg_push_table");
  const int64_t n = b->n_rows;
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8;
  if (!b->ts || (utf8 ? (!b->key_offsets || !b->key_bytes) : !b->key_i64))
    if (n > 0) return fail(KHIP_E_INVALID, "missing key or timestamp column");
  for (int c = 0; c < a->desc.n_cols; c++)
    if (n > 0 && (!b->col_data || !b->col_data[c])) return fail(KHIP_E_INVALID, "missing value column");
  return KHIP_OK;
}

// The SUPPLIED close context (*sctx: this push consumes one), the emission state of the last push
// forgotten, and the two empty batches, which end the push here (*done).
static khip_status push_begin(khip_agg* a, int64_t n, bool* sctx, bool* done, khip_batch_stats* stats) {
  const bool supd = a->desc.time_domain == KHIP_TIME_SUPPLIED;
  if (supd && a->desc.emit == KHIP_EMIT_FINAL && !a->sup_set)
    return fail(KHIP_E_INVALID, "KHIP_TIME_SUPPLIED + EMIT FINAL: khip_agg_supplied_close before every push");
  *sctx = supd && a->sup_set;
  a->sup_set = false;
  a->st_before = *sctx ? a->sup_before : a->host_stream_time;
  a->chg_ready = false;
  a->lost.clear();
  *done = n == 0;
  if (n == 0 && !*sctx) {  // nothing changes, nothing closes
    a->chg_ready = true;
    a->chg_n = 0;
    put_stats(a, 0, nullptr, false, stats);
    return KHIP_OK;
  }
  if (n == 0) {  // SUPPLIED: nothing arrived here, but the GLOBAL stream time may close windows
    KHIP_TRY(supplied_advance(a));
    if (a->desc.emit == KHIP_EMIT_FINAL) a->lost = a->sup_lost;
    else a->chg_ready = true, a->chg_n = 0;
    put_stats(a, 0, nullptr, false, stats);
    return KHIP_OK;
  }
  if (a->changelog && n >= (1LL << 31)) return fail(KHIP_E_UNSUPPORTED, "changelog pushes above 2^31 rows");
  return KHIP_OK;
}

// Offset aggregates: the hidden sequence columns behind the user columns (one iota, the arguments'
// validity).
static khip_status push_hidden_cols(khip_agg* a, BatchIn& in) {
  if (!a->n_hidden) return KHIP_OK;
  const int64_t n = in.n;
  KHIP_TRY(a->seqbuf.ensure((size_t)n * 8));
  hipLaunchKernelGGL(k_off_iota, dim3(grid_for(n, 256, 4096)), dim3(256), 0, a->stream, a->seqbuf.as<int64_t>(), n,
                     a->seq_base);
  KHIP_TRY_HIP(hipGetLastError());
  bool any_not = false;
  for (int h = 0; h < a->n_hidden; h++) any_not = any_not || a->hid_not[h];
  if (any_not) {  // EARLIEST's N forms: the complemented sequence
    KHIP_TRY(a->nseqbuf.ensure((size_t)n * 8));
    hipLaunchKernelGGL(k_off_iota_not, dim3(grid_for(n, 256, 4096)), dim3(256), 0, a->stream,
                       a->nseqbuf.as<int64_t>(), n, a->seq_base);
    KHIP_TRY_HIP(hipGetLastError());
  }
  for (int h = 0; h < a->n_hidden; h++) {
    in.cols.data[a->desc.n_cols + h] = a->hid_not[h] ? a->nseqbuf.p : a->seqbuf.p;
    in.cols.valid[a->desc.n_cols + h] = a->hid_src[h] >= 0 ? in.cols.valid[a->hid_src[h]] : nullptr;
  }
  return KHIP_OK;
}

// What the batch's times decide before the engine runs: EMIT FINAL's lost windows in the TASK
// domain, and the ABI 5 stream-time domains' column in.st_at, the stream time observed at every row
// (SUPPLIED: the caller's; PARTITION: scanned per source partition, with its lost windows).
static khip_status push_stream_time(khip_agg* a, const khip_batch* b, BatchIn& in, bool sctx) {
  const int64_t n = in.n;
  const bool final_emit = a->desc.emit == KHIP_EMIT_FINAL;
  const bool pdomain = a->desc.time_domain == KHIP_TIME_PARTITION;
  // (SESSION windows close sessions themselves: sess_push)
  if (final_emit && !pdomain && !sctx && a->engine != 2)
    KHIP_TRY(emit_final_lost(a, in.ts, in.kv, in.rv, n, a->st_before));
  if (a->desc.time_domain == KHIP_TIME_SUPPLIED) {
    if (!b->stream_time) return fail(KHIP_E_INVALID, "KHIP_TIME_SUPPLIED: the batch has no stream_time column");
    if (b->mem == KHIP_MEM_HOST) {
      KHIP_TRY(stage(a, a->st_col, b->stream_time, n * 8));
      in.st_at = a->st_col.as<int64_t>();
    } else {
      in.st_at = b->stream_time;
    }
  } else if (pdomain) {
    if (!b->partition) return fail(KHIP_E_INVALID, "KHIP_TIME_PARTITION: the batch has no partition column");
    in.part = b->partition;
    if (b->mem == KHIP_MEM_HOST) {
      KHIP_TRY(stage(a, a->st_part, b->partition, n * 4));
      in.part = a->st_part.as<int32_t>();
    }
    KHIP_TRY(a->st_col.ensure((size_t)n * 8));
    KHIP_TRY(stream_time_column(a, in.ts, in.kv, in.rv, in.part, n, -1, a->st_col.as<int64_t>(), nullptr));
    in.st_at = a->st_col.as<int64_t>();
    if (final_emit) KHIP_TRY(partition_lost(a, in.ts, in.kv, in.rv, in.part, in.st_at, n));
  }
  return KHIP_OK;
}

// PARTITION domain, per-task retention / EMIT FINAL: every accepted key's partition (the tasks share
// one table).  A batch that puts a key on a second partition is rejected before it changes the
// handle's stream times: the partitions' stream times go back to their values before the batch (the
// batch's new keys stay recorded with the partitions it named, as its dictionary entries stay).
static khip_status push_key_partitions(khip_agg* a, const BatchIn& in) {
  if (a->desc.time_domain != KHIP_TIME_PARTITION || !a->windowed) return KHIP_OK;
  const khip_status ps = pmap_insert(a, in.keys, in.kv, in.rv, in.ts, in.part, in.n);
  if (ps != KHIP_OK) std::swap(a->pst, a->pst2);
  return ps;
}

// Partitioned engine: part_push in slices of < 2^31 records (multiple of 8: bitmaps stay byte
// aligned), each followed by its offset aggregates' resolve.
static khip_status part_push_slices(khip_agg* a, const BatchIn& in, int64_t* tot) {
  const int64_t n = in.n, slice = 1LL << 31;
  for (int64_t off = 0; off < n; off += slice) {
    const int64_t m = std::min(slice, n - off);
    ColPtrs cs = in.cols;
    for (int c = 0; c < a->ap.n_cols; c++) {  // (the hidden sequence columns too: the base advances per slice)
      cs.data[c] = (const char*)in.cols.data[c] + off * (a->ap.col_type[c] == KHIP_TYPE_INT32 ? 4 : 8);
      if (cs.valid[c]) cs.valid[c] += off / 8;
    }
    const int64_t closed0 = a->part.closed_n;
    KHIP_TRY(part_push(a, m, in.keys + off, in.ts + off, in.kv ? in.kv + off / 8 : nullptr,
                       in.rv ? in.rv + off / 8 : nullptr, cs, tot, in.st_at ? in.st_at + off : nullptr));
    // offset aggregates: the slice's winning sequence numbers become values, before the closed
    // store is purged and before anything reads rows or changes
    if (a->offs.n) KHIP_TRY(off_resolve_part(a, cs, a->seq_base + off, m, closed0));
  }
  return KHIP_OK;
}

// Global-atomic engine (engine 1), the sibling of part_push / sess_push: the stream time before
// each block, then apply → reduce → finalize passes, resumed after a table doubling while records
// ran out of probes; the offset aggregates re-probe their groups in the final table.  Profile: the
// records count on pass 0, an apply launch per pass.
static khip_status atomic_push(khip_agg* a, const BatchIn& in, int64_t* tot) {
  const int64_t n = in.n;
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8;
  // ---- scratch
  const int64_t nb = ceil_div(n, RPB);
  KHIP_TRY(a->blockmax.ensure(nb * 8));
  KHIP_TRY(a->blockprefix.ensure(nb * 8));
  KHIP_TRY(a->partials.ensure(nb * 8 * NPART));
  if (a->resume_n < n) {
    KHIP_TRY(a->resume.ensure(n * 4));
    KHIP_TRY_HIP(hipMemsetAsync(a->resume.p, 0xFF, n * 4, a->stream));
    a->resume_n = n;
  }
  KHIP_TRY_HIP(hipMemsetAsync(a->counters.p, 0, 8 * NPART, a->stream));
  // ---- stream time before each block
  ev_record(a, 0);
  hipLaunchKernelGGL(k_blockmax, dim3(nb), dim3(BLOCK), 0, a->stream, in.ts, in.kv, in.rv, n,
                     a->blockmax.as<int64_t>(), in.st_at);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, a->stream, a->blockmax.as<int64_t>(), nb,
                     a->blockprefix.as<int64_t>(), a->stream_time.as<int64_t>());
  KHIP_TRY_HIP(hipGetLastError());
  ev_record(a, 2);
  // ---- grow the group table ahead of time if the resident load is high
  if (2 * a->occ > a->cap) KHIP_TRY(agg_grow_table(a, a->cap * 4));
  // ---- apply (+ resume passes after doubling on probe exhaustion)
  const int64_t occ0 = a->occ;
  double apply_ms = 0, fin_ms = 0;
  for (int pass = 0;; pass++) {
    ev_record(a, 3);
    hipLaunchKernelGGL(k_apply, dim3(nb), dim3(BLOCK), 0, a->stream, a->ap, in.hkeys, in.keys, in.ts, in.kv, in.rv,
                       in.cols, a->blockprefix.as<int64_t>(), n, a->table.as<uint64_t>(), (uint64_t)(a->cap - 1),
                       a->resume.as<int32_t>(), a->partials.as<int64_t>(), pass > 0 ? 1 : 0, in.st_at);
    ev_record(a, 4);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, a->stream, a->partials.as<int64_t>(), nb, NPART,
                       a->counters.as<int64_t>());
    hipLaunchKernelGGL(k_finalize, dim3(grid_for(a->cap, 256)), dim3(256), 0, a->stream, a->table.as<uint64_t>(),
                       a->cap, a->sw, in.keys, in.ts, a->windowed, a->desc.size_ms, a->desc.advance_ms);
    KHIP_TRY_HIP(hipGetLastError());
    ev_record(a, 5);
    int64_t c[NPART];
    KHIP_TRY_HIP(hipMemcpyAsync(c, a->counters.p, 8 * NPART, hipMemcpyDeviceToHost, a->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
    const int64_t failed = c[P_FAILED] - tot[P_FAILED];
    for (int k = 0; k < NPART; k++) tot[k] = c[k];
    a->occ = occ0 + tot[P_NEW];  // every claim is counted exactly once
    if (a->profile) {
      apply_ms += ev_ms(a, 3, 4);
      fin_ms += ev_ms(a, 4, 5);
      if (pass == 0) {
        a->times.stream_time_ms += ev_ms(a, 0, 3);
        if (utf8) a->times.dict_ms += ev_ms(a, 1, 2);
        a->times.records += n;
      }
      a->times.apply_launches++;
    }
    if (failed == 0) break;
    if (pass > 40) return fail(KHIP_E_DEVICE, "aggregate table could not absorb the batch");
    KHIP_TRY(agg_grow_table(a, a->cap * 2));
  }
  a->times.apply_ms += apply_ms;
  a->times.finalize_ms += fin_ms;
  if (a->offs.n) {  // offset aggregates: every record re-probes its groups (the table is final now)
    const OffResolve q = off_query(a, in.cols, a->seq_base, n);
    auto probe = off_has_lists(q) ? k_off_resolve_probe<true> : k_off_resolve_probe<false>;
    hipLaunchKernelGGL(probe, dim3(grid_for(n, 256)), dim3(256), 0, a->stream, a->ap, in.hkeys, in.keys, in.ts,
                       in.kv, in.rv, n, a->table.as<uint64_t>(), (uint64_t)(a->cap - 1), q);
    KHIP_TRY_HIP(hipGetLastError());
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));  // (a host batch's staging buffers are reused by the next push)
  }
  return KHIP_OK;
}

// The batch into the handle's engine; tot[P_*]: the push's counters.
static khip_status push_engine(khip_agg* a, const BatchIn& in, bool sctx, int64_t* tot) {
  if (a->engine == 2) {
    if (in.n >= (1LL << 31)) return fail(KHIP_E_UNSUPPORTED, "SESSION pushes above 2^31 rows");
    // SUPPLIED with a close context: the GLOBAL stream time after the batch bounds the store's
    // expiry (sess_push expires against the handle's stream time after the push)
    if (sctx) KHIP_TRY(supplied_advance(a));
    return sess_push(a, in.n, in.keys, in.ts, in.kv, in.rv, in.cols, tot, in.st_at);
  }
  if (a->engine == 1) return atomic_push(a, in, tot);
  KHIP_TRY(part_push_slices(a, in, tot));
  a->occ += tot[P_NEW];
  part_profile(a, in.n, a->desc.key_type == KHIP_KEY_UTF8);  // (once per push, from the last slice's events)
  return KHIP_OK;
}

// The end of a push: the handle's stream time after the batch in its domain, EMIT FINAL's lost
// windows, the retention purge of the closed store, the statistics.
static khip_status push_finish(khip_agg* a, const BatchIn& in, bool sctx, const int64_t* tot,
                               khip_batch_stats* stats) {
  const bool final_emit = a->desc.emit == KHIP_EMIT_FINAL;
  const bool pdomain = a->desc.time_domain == KHIP_TIME_PARTITION;
  a->seq_base += in.n;
  if (a->engine == 1) {  // the other engines brought it back with their end-of-push counters
    KHIP_TRY_HIP(hipMemcpyAsync(&a->host_stream_time, a->stream_time.p, 8, hipMemcpyDeviceToHost, a->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  }
  // one task per partition: the handle's stream time (closing windows, retention) is the slowest's
  if (pdomain) KHIP_TRY(stream_time_partition_min(a));
  if (sctx) KHIP_TRY(supplied_advance(a));  // one task over the whole stream: the GLOBAL stream time
  if (final_emit && sctx) a->lost = a->sup_lost;
  else if (final_emit && a->engine != 2)
    KHIP_TRY(pdomain ? partition_lost_finish(a) : finish_lost_seed(a, in.ts, in.kv, in.rv, in.n, a->st_before));
  if (a->engine == 0) KHIP_TRY(purge_expired(a, true));  // (PARTITION: each row by its own task's bound)
  put_stats(a, in.n, tot, false, stats);
  return KHIP_OK;
}

khip_status khip_agg_push(khip_agg* a, const khip_batch* b, khip_batch_stats* stats) {
  clear_error();
  KHIP_TRY(push_check(a, b));
  DeviceGuard g(a->device);
  bool sctx = false, done = false;
  KHIP_TRY(push_begin(a, b->n_rows, &sctx, &done, stats));
  if (done) return KHIP_OK;
  BatchIn in;
  KHIP_TRY(resolve_batch(a, b, in));  // device pointers (host batches staged)
  KHIP_TRY(push_hidden_cols(a, in));
  KHIP_TRY(push_stream_time(a, b, in, sctx));
  // UTF8 keys → stable key ids; their hashes only for the global-atomic engine's slot hashing
  if (a->desc.key_type == KHIP_KEY_UTF8) KHIP_TRY(key_ids(a, in, a->engine == 1, true));
  KHIP_TRY(push_key_partitions(a, in));
  int64_t tot[NPART] = {0};
  KHIP_TRY(push_engine(a, in, sctx, tot));
  return push_finish(a, in, sctx, tot, stats);
}

khip_status khip_stream_time_scan(khip_agg* a, const khip_batch* b, int64_t seed, int64_t* out, int64_t* out_max) {
  clear_error();
  if (!a || !b || !out_max || (b->n_rows > 0 && (!out || !b->ts))) return fail(KHIP_E_INVALID, "null argument");
  if (b->n_rows < 0) return fail(KHIP_E_INVALID, "batch shape");
  DeviceGuard g(a->device);
  const int64_t n = b->n_rows;
  *out_max = seed < -1 ? -1 : seed;
  if (n == 0) return KHIP_OK;
  BatchIn in;
  KHIP_TRY(stage_ts_valid(a, b, in));
  int64_t* dst = out;
  if (b->mem == KHIP_MEM_HOST) {
    KHIP_TRY(a->st_col.ensure((size_t)n * 8));
    dst = a->st_col.as<int64_t>();
  }
  KHIP_TRY(a->st_seen.ensure(8));
  int64_t* last = a->st_seen.as<int64_t>();
  KHIP_TRY(stream_time_column(a, in.ts, in.kv, in.rv, nullptr, n, seed < -1 ? -1 : seed, dst, last));
  if (b->mem == KHIP_MEM_HOST) KHIP_TRY_HIP(hipMemcpyAsync(out, dst, (size_t)n * 8, hipMemcpyDeviceToHost, a->stream));
  KHIP_TRY_HIP(hipMemcpyAsync(out_max, last, 8, hipMemcpyDeviceToHost, a->stream));
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  return KHIP_OK;
}

khip_status khip_agg_lost_windows(khip_agg* a, const khip_batch* b, int64_t seed, int64_t* ranges, int64_t capacity,
                                  int64_t* n_ranges) {
  clear_error();
  if (!a || !b || !n_ranges || (b->n_rows > 0 && !b->ts)) return fail(KHIP_E_INVALID, "null argument");
  if (b->n_rows < 0) return fail(KHIP_E_INVALID, "batch shape");
  if (!a->windowed || a->engine == 2 || a->desc.emit != KHIP_EMIT_FINAL)
    return fail(KHIP_E_INVALID, "lost windows: an EMIT FINAL TUMBLING / HOPPING aggregation");
  DeviceGuard g(a->device);
  const int64_t n = b->n_rows;
  *n_ranges = 0;
  if (n == 0) return KHIP_OK;
  BatchIn in;
  KHIP_TRY(stage_ts_valid(a, b, in));
  const int64_t sd = seed < -1 ? -1 : seed;
  KHIP_TRY(emit_final_lost(a, in.ts, in.kv, in.rv, n, sd));
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  const std::vector<int64_t> keep = a->lost;  // (the handle's own last push)
  KHIP_TRY(finish_lost_seed(a, in.ts, in.kv, in.rv, n, sd));
  std::vector<int64_t> got;
  got.swap(a->lost);
  a->lost = keep;
  *n_ranges = (int64_t)got.size() / 2;
  if (*n_ranges > capacity || (*n_ranges > 0 && !ranges)) return fail(KHIP_E_BUFFER, "ranges capacity");
  std::copy(got.begin(), got.end(), ranges);
  return KHIP_OK;
}

khip_status khip_agg_supplied_close(khip_agg* a, int64_t st_before, int64_t st_after, const int64_t* ranges,
                                    int64_t n_ranges) {
  clear_error();
  if (!a || n_ranges < 0 || (n_ranges > 0 && !ranges)) return fail(KHIP_E_INVALID, "null argument");
  if (a->desc.time_domain != KHIP_TIME_SUPPLIED) return fail(KHIP_E_INVALID, "handle not KHIP_TIME_SUPPLIED");
  if (st_after < st_before) return fail(KHIP_E_INVALID, "stream time after the batch below the one before");
  std::vector<std::pair<int64_t, int64_t>> r((size_t)n_ranges);
  for (int64_t k = 0; k < n_ranges; k++) {
    if (ranges[2 * k] > ranges[2 * k + 1]) return fail(KHIP_E_INVALID, "lost range with lo > hi");
    r[k] = {ranges[2 * k], ranges[2 * k + 1]};
  }
  a->sup_lost = merge_ranges(std::move(r));
  a->sup_before = st_before < -1 ? -1 : st_before;
  a->sup_after = st_after < -1 ? -1 : st_after;
  a->sup_set = true;
  return KHIP_OK;
}

// No row of the table has expired (retention) yet: every group counted in occ is visible.  The
// partitioned engine purges its closed store after every push; its live rows satisfy
// ws + size > (stream time before the last push) - grace, so they are all visible while that
// bound is at or above the first visible window start.  The atomic engine keeps every row.
static bool no_expired_live(const khip_agg* a) {
  if (a->engine == 2) return true;  // the session store drops expired sessions at every push
  if (a->desc.time_domain == KHIP_TIME_PARTITION && a->windowed) {  // no task has expired a window
    for (int64_t t : a->pst_host)
      if (partition_vis_from(a, t) != INT64_MIN) return false;
    return true;
  }
  const int64_t vf = visible_from(a);
  if (vf == INT64_MIN) return true;
  if (a->engine != 0 || a->st_before < 0) return false;
  return vf <= a->st_before - a->grace - a->desc.size_ms + 1;
}

static khip_status compact_rows(khip_agg* a, const khip_having* h, std::vector<uint64_t>* rows, int64_t* count,
                                const HavingDev* pull = nullptr) {
  HavingDev hd{};
  if (pull) hd = *pull;
  if (a->windowed && !hd.fin && a->engine != 2) {  // the store: expired windows are gone (retention)
    hd.vis = 1;
    hd.vis_from = visible_from(a);
  }
  hd.session = a->engine == 2;
  KHIP_TRY(partition_bounds(a, hd));  // PARTITION: each row's retention / EMIT FINAL bounds are its task's
  if (h) {
    if (h->agg_index < 0 || h->agg_index >= a->desc.n_aggs) return fail(KHIP_E_INVALID, "having agg index");
    if (h->op < KHIP_OP_GT || h->op > KHIP_OP_NE) return fail(KHIP_E_INVALID, "having op");
    if (agg_is_offset(a->aggs[h->agg_index].kind))  // (decode_words does not know the offset kinds)
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a LATEST / EARLIEST_BY_OFFSET aggregate");
    if (agg_is_topk(a->aggs[h->agg_index].kind))  // (nor the TOPK kinds: an ARRAY has no comparison)
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a TOPK / TOPKDISTINCT aggregate (an ARRAY)");
    if (agg_is_var(a->aggs[h->agg_index].kind))  // (nor the STDDEV kinds: decoded on the host from several words)
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a STDDEV_SAMP / STDDEV_SAMPLE aggregate");
    if (agg_is_pair(a->aggs[h->agg_index].kind))  // (nor CORRELATION, for the same reason)
      return fail(KHIP_E_UNSUPPORTED, "HAVING on a CORRELATION aggregate");
    hd.active = 1;
    hd.op = h->op;
    hd.a = a->outs[h->agg_index];
    hd.i64 = h->i64;
    hd.f64 = h->f64;
  }
  if (a->engine == 0) {
    KHIP_TRY(part_compact(a, hd, rows, count));
    if (rows && *count > a->occ) return fail(KHIP_E_STATE, "group count bookkeeping mismatch");
    return KHIP_OK;
  }
  // global-atomic table, or the SESSION store (a flat row array)
  const uint64_t* src = a->engine == 2 ? a->sess.rows.as<uint64_t>() : a->table.as<uint64_t>();
  const int64_t nsrc = a->engine == 2 ? a->sess.n : a->cap;
  DevBuf ctr, out;
  KHIP_TRY(ctr.ensure(8));
  KHIP_TRY_HIP(hipMemsetAsync(ctr.p, 0, 8, a->stream));
  const int grid = grid_for(std::max<int64_t>(nsrc, 1), 256, 4096);
  if (rows) KHIP_TRY(out.ensure((size_t)std::max<int64_t>(a->occ, 1) * a->sw * 8));
  if (nsrc)
    hipLaunchKernelGGL(k_compact, dim3(grid), dim3(256), 0, a->stream, src, nsrc, a->sw, hd,
                       rows ? out.as<uint64_t>() : nullptr, std::max<int64_t>(a->occ, 1), ctr.as<unsigned long long>());
  KHIP_TRY_HIP(hipGetLastError());
  int64_t n = 0;
  KHIP_TRY_HIP(hipMemcpyAsync(&n, ctr.p, 8, hipMemcpyDeviceToHost, a->stream));
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  *count = n;
  if (rows && n > a->occ) return fail(KHIP_E_STATE, "group count bookkeeping mismatch");
  if (rows) {
    rows->resize((size_t)n * a->sw);
    if (n) KHIP_TRY_HIP(hipMemcpy(rows->data(), out.p, (size_t)n * a->sw * 8, hipMemcpyDeviceToHost));
  }
  ctr.release();
  out.release();
  return KHIP_OK;
}

khip_status khip_agg_count_rows(khip_agg* a, const khip_having* h, int64_t* n) {
  clear_error();
  if (!a || !n) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  // every row while none has expired: the group count every engine maintains, no table scan
  if (!h && no_expired_live(a)) {
    *n = a->occ;
    return KHIP_OK;
  }
  // the query's own HAVING: counts maintained by the aggregate kernel, no table scan
  if (h && a->engine == 0 && a->desc.has_having && h->agg_index == a->desc.having.agg_index &&
      h->op == a->desc.having.op && h->i64 == a->desc.having.i64 &&
      (h->f64 == a->desc.having.f64 || (h->f64 != h->f64 && a->desc.having.f64 != a->desc.having.f64)) &&
      no_expired_live(a) && part_having_count(a, n))
    return KHIP_OK;
  return compact_rows(a, h, nullptr, n);
}

// The host copy of a UTF8 handle's arena: an id's key length (an inline id's is in the id).
static khip_status arena_host(khip_agg* a, std::vector<uint8_t>* arena) {
  arena->resize(a->dict.arena_used);
  if (a->dict.arena_used)
    KHIP_TRY_HIP(hipMemcpy(arena->data(), a->dict.arena.p, a->dict.arena_used, hipMemcpyDeviceToHost));
  return KHIP_OK;
}
static int64_t kid_len(const std::vector<uint8_t>& arena, int64_t kid) {
  return kid_inline(kid) ? (kid >> 57) & 31 : *(const int64_t*)(arena.data() + kid + 8);
}

khip_status khip_agg_snapshot_size(khip_agg* a, int64_t* n_rows, int64_t* key_bytes) {
  clear_error();
  if (!a) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  if (n_rows) {
    *n_rows = a->occ;
    if (!no_expired_live(a)) KHIP_TRY(compact_rows(a, nullptr, nullptr, n_rows));
  }
  if (key_bytes) {
    if (a->desc.key_type == KHIP_KEY_UTF8) {
      std::vector<uint64_t> rows;
      int64_t n = 0;
      KHIP_TRY(compact_rows(a, nullptr, &rows, &n));
      std::vector<uint8_t> arena;
      KHIP_TRY(arena_host(a, &arena));
      int64_t kb = 0;
      for (int64_t r = 0; r < n; r++) kb += kid_len(arena, (int64_t)rows[r * a->sw]);
      *key_bytes = kb;
    } else {
      *key_bytes = 0;
    }
  }
  return KHIP_OK;
}

// Sort compacted rows by (key, window start) and write them to the caller's snapshot buffers
// (ResultTransformer map() + WindowBoundsPopulator).
static khip_status emit_snapshot(khip_agg* a, const std::vector<uint64_t>& rows, int64_t n, khip_snapshot* out,
                                 const std::vector<uint8_t>* tomb_in = nullptr, uint8_t* tomb_out = nullptr) {
  const int sw = a->sw;
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8;
  // UTF8: each row's key bytes — its arena entry, or its inline id's digits (decoded once per row)
  std::vector<uint8_t> arena, inl;
  std::vector<const uint8_t*> kp;
  std::vector<int64_t> kl;
  if (utf8) {
    KHIP_TRY(arena_host(a, &arena));
    int64_t ni = 0;
    for (int64_t r = 0; r < n; r++) ni += kid_inline((int64_t)rows[r * sw]) ? 1 : 0;
    inl.resize((size_t)ni * KEY_INLINE_MAX);
    kp.resize(n);
    kl.resize(n);
    ni = 0;
    for (int64_t r = 0; r < n; r++) {
      const int64_t kid = (int64_t)rows[r * sw];
      if (kid_inline(kid)) {
        uint8_t* o = inl.data() + ni++ * KEY_INLINE_MAX;
        kl[r] = kid_inline_bytes(kid, o);
        kp[r] = o;
      } else {
        kl[r] = *(const int64_t*)(arena.data() + kid + 8);
        kp[r] = arena.data() + kid + 16;
      }
    }
  }
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  const bool session = a->engine == 2;
  std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    const int64_t kx = (int64_t)rows[x * sw], ky = (int64_t)rows[y * sw];
    if (kx != ky) {
      if (!utf8) return kx < ky;
      const int64_t lx = kl[x], ly = kl[y];
      const int c = memcmp(kp[x], kp[y], (size_t)std::min(lx, ly));
      if (c) return c < 0;
      if (lx != ly) return lx < ly;
    }
    if (session && tomb_in && (*tomb_in)[x] != (*tomb_in)[y]) return (*tomb_in)[x] > (*tomb_in)[y];  // deletes first
    if (rows[x * sw + 1] != rows[y * sw + 1]) return (int64_t)rows[x * sw + 1] < (int64_t)rows[y * sw + 1];
    return (int64_t)rows[x * sw + 2] < (int64_t)rows[y * sw + 2];
  });
  if (n > out->capacity) {
    out->n_rows = n;
    return fail(KHIP_E_BUFFER, "snapshot capacity too small");
  }
  int64_t kb = 0;
  if (utf8 && out->key_offsets) out->key_offsets[0] = 0;
  for (int64_t r = 0; r < n; r++) {
    const uint64_t* s = &rows[order[r] * sw];
    const int64_t key = (int64_t)s[0], ws = (int64_t)s[1];
    if (tomb_out) tomb_out[r] = tomb_in ? (*tomb_in)[order[r]] : 0;
    if (utf8) {
      const int64_t len = kl[order[r]];
      if (kb + len > out->key_bytes_capacity) return fail(KHIP_E_BUFFER, "snapshot key bytes capacity too small");
      if (out->key_bytes && len) memcpy(out->key_bytes + kb, kp[order[r]], (size_t)len);
      kb += len;
      if (out->key_offsets) out->key_offsets[r + 1] = kb;
    } else if (out->key_i64) {
      out->key_i64[r] = key;
    }
    if (out->window_start) out->window_start[r] = a->windowed ? ws : 0;
    if (out->window_end) out->window_end[r] = a->windowed ? (session ? (int64_t)s[2] : ws + a->desc.size_ms) : 0;
    if (out->rowtime) out->rowtime[r] = (int64_t)s[2];
    for (int i = 0; i < a->desc.n_aggs; i++) {
      const AggOut& o = a->outs[i];
      if (o.kind == KHIP_AGG_TOPK || o.kind == KHIP_AGG_TOPKDISTINCT) {
        // the ARRAY layout of khip_snapshot: L = k elements per row, the list first (descending:
        // the slots' order), then null slots.  TOPK: the column's non-null count says how many
        // slots are values (a Long.MIN_VALUE has the empty slot's key); TOPKDISTINCT: the leading
        // slots that are not empty, then Long.MIN_VALUE if its flag word is set and there is room.
        const int L = a->agg_k[i];
        int len = 0;
        if (o.kind == KHIP_AGG_TOPK) len = (int)std::min<int64_t>((int64_t)s[o.w_cnt], L);
        else
          while (len < L && (int64_t)s[o.w_val + len] != INT64_MIN) len++;
        const bool tail_min = a->out_flag[i] >= 0 && s[a->out_flag[i]] != 0 && len < L;
        for (int j = 0; j < L; j++) {
          const bool has = j < len || (tail_min && j == len);
          const int64_t key = j < len ? (int64_t)s[o.w_val + j] : INT64_MIN;
          const int64_t at = r * L + j;
          if (out->agg_values && out->agg_values[i]) {
            if (o.type == KHIP_TYPE_INT32) ((int32_t*)out->agg_values[i])[at] = has ? (int32_t)key : 0;
            else if (o.type == KHIP_TYPE_INT64) ((int64_t*)out->agg_values[i])[at] = has ? key : 0;
            else ((double*)out->agg_values[i])[at] = has ? f64_from_order_key(key) : 0.0;
          }
          if (out->agg_null && out->agg_null[i]) out->agg_null[i][at] = has ? 0 : 1;
        }
        continue;
      }
      if (a->out_off[i] >= 0 && a->offs.a[a->out_off[i]].n) {
        // the N forms of LATEST / EARLIEST_BY_OFFSET: the same layout, oldest first.  len = the
        // leading non-empty slots; EARLIEST's slots are already oldest first, LATEST's newest first
        // (element e is value word len - 1 - e).  The values are the argument's bits; null byte 2 =
        // a NULL element (KEEP_NULLS), 1 = past the end.
        const OffSpec& f = a->offs.a[a->out_off[i]];
        const int L = f.n;
        int len = 0;
        while (len < L && (int64_t)s[f.w_seq + len] != INT64_MIN) len++;
        const uint64_t mask = f.w_null >= 0 ? s[f.w_null] : 0ULL;
        for (int e = 0; e < L; e++) {
          const int j = f.earliest ? e : len - 1 - e;
          const bool has = e < len, nul = has && ((mask >> j) & 1ULL);
          const uint64_t bits = has && !nul ? s[f.w_val + j] : 0ULL;
          const int64_t at = r * L + e;
          if (out->agg_values && out->agg_values[i]) {
            if (o.type == KHIP_TYPE_INT32) ((int32_t*)out->agg_values[i])[at] = (int32_t)(int64_t)bits;
            else ((uint64_t*)out->agg_values[i])[at] = bits;  // INT64, or DOUBLE bits (NaN payloads, -0.0)
          }
          if (out->agg_null && out->agg_null[i]) out->agg_null[i][at] = !has ? 1 : (nul ? 2 : 0);
        }
        continue;
      }
      int64_t iv = 0;
      double dv = 0.0;
      bool isnull = false;
      switch (o.kind) {
        case KHIP_AGG_COUNT_STAR:
        case KHIP_AGG_COUNT: iv = (int64_t)s[o.w_val]; break;
        case KHIP_AGG_SUM:
          if (o.type == KHIP_TYPE_DOUBLE) memcpy(&dv, &s[o.w_val], 8);
          else iv = (int64_t)s[o.w_val];
          break;
        case KHIP_AGG_MIN:
        case KHIP_AGG_MAX:
          if ((int64_t)s[o.w_cnt] == 0) isnull = true;
          else if (o.type == KHIP_TYPE_DOUBLE) dv = f64_from_order_key((int64_t)s[o.w_val]);
          else iv = (int64_t)s[o.w_val];
          break;
        case KHIP_AGG_LATEST_BY_OFFSET:
        case KHIP_AGG_EARLIEST_BY_OFFSET: {  // NULL: no record yet, or the winning row's NULL (KEEP_NULLS)
          const OffSpec& f = a->offs.a[a->out_off[i]];
          const int64_t none = o.kind == KHIP_AGG_LATEST_BY_OFFSET ? INT64_MIN : INT64_MAX;
          if ((int64_t)s[f.w_seq] == none || (f.w_null >= 0 && s[f.w_null] != 0)) isnull = true;
          else if (o.type == KHIP_TYPE_DOUBLE) memcpy(&dv, &s[f.w_val], 8);  // the bits: NaN payloads, -0.0
          else iv = (int64_t)s[f.w_val];
          break;
        }
        case KHIP_AGG_STDDEV_SAMP:
        case KHIP_AGG_STDDEV_SAMPLE: {  // never NULL: 0.0 below two records (map :171-174)
          const khip_agg::VarWords& v = a->out_var[i];
          const bool big = o.type == KHIP_TYPE_INT64;
          dv = variance_result(o.kind == KHIP_AGG_STDDEV_SAMPLE, big, (int64_t)s[o.w_cnt], s[o.w_val],
                               big ? s[v.w_hi] : 0, &s[v.w_sq], big ? 4 : 2);
          break;
        }
        case KHIP_AGG_CORRELATION: {  // never NULL: NaN below two pairs or for a constant argument (map :127-133)
          const khip_agg::PairWords& v = a->out_pair[i];
          dv = correlation_result(o.type == KHIP_TYPE_INT64, s[v.w_n], &s[v.w_sx], &s[v.w_sy], &s[v.w_sxx], &s[v.w_syy],
                                  &s[v.w_sxy]);
          break;
        }
        case KHIP_AGG_AVG: {
          const int64_t c = (int64_t)s[o.w_cnt];
          if (c == 0) dv = 0.0;
          else if (o.type == KHIP_TYPE_DOUBLE) { double sum; memcpy(&sum, &s[o.w_val], 8); dv = sum / (double)c; }
          else if (o.type == KHIP_TYPE_INT32) dv = (double)(int32_t)s[o.w_val] / (double)c;
          else dv = (double)(int64_t)s[o.w_val] / (double)c;
          break;
        }
      }
      int32_t rt;
      khip_agg_result_type(&a->desc, i, &rt);
      if (out->agg_values && out->agg_values[i]) {
        if (rt == KHIP_TYPE_INT32) ((int32_t*)out->agg_values[i])[r] = isnull ? 0 : (int32_t)iv;
        else if (rt == KHIP_TYPE_INT64) ((int64_t*)out->agg_values[i])[r] = isnull ? 0 : iv;
        else ((double*)out->agg_values[i])[r] = isnull ? 0.0 : dv;
      }
      if (out->agg_null && out->agg_null[i]) out->agg_null[i][r] = isnull ? 1 : 0;
    }
  }
  out->n_rows = n;
  out->key_bytes_len = kb;
  return KHIP_OK;
}

khip_status khip_agg_snapshot(khip_agg* a, const khip_having* h, khip_snapshot* out) {
  clear_error();
  if (!a || !out) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  std::vector<uint64_t> rows;
  int64_t n = 0;
  KHIP_TRY(compact_rows(a, h, &rows, &n));
  return emit_snapshot(a, rows, n, out);
}

khip_status khip_agg_get(khip_agg* a, const khip_pull* q, const khip_having* h, khip_snapshot* out) {
  clear_error();
  if (!a || !q || !out) return fail(KHIP_E_INVALID, "null argument");
  if (q->n_keys < 0 || (q->n_keys > 0 && a->desc.key_type == KHIP_KEY_INT64 && !q->keys))
    return fail(KHIP_E_INVALID, "pull keys");
  const bool utf8 = a->desc.key_type == KHIP_KEY_UTF8;
  if (q->n_keys > 0 && utf8 && (!q->key_offsets || !q->key_bytes || q->key_offsets[0] != 0))
    return fail(KHIP_E_INVALID, "pull UTF8 keys need key_offsets (from 0) and key_bytes");
  DeviceGuard g(a->device);
  HavingDev pd{};
  pd.pull = 1;
  pd.pull_windowed = a->windowed;
  pd.ws_lo = q->ws_lo;
  pd.ws_hi = q->ws_hi;
  pd.we_lo = q->we_lo;
  pd.we_hi = q->we_hi;
  pd.size_ms = a->desc.size_ms;
  DevBuf dkeys;
  std::vector<int64_t> k;  // outlives the copy: compact_rows synchronises the stream
  if (q->n_keys > 0 && utf8) {
    // key bytes → dictionary ids on the device (read-only probe; digit keys: their inline ids);
    // unseen keys match nothing
    const int64_t nk = q->n_keys, nb = q->key_offsets[nk];
    k.assign((size_t)nk, -1);
    {
      DevBuf doff, dbytes, dkid;
      KHIP_TRY(doff.ensure((size_t)(nk + 1) * 8));
      KHIP_TRY(dbytes.ensure((size_t)std::max<int64_t>(nb, 1)));
      KHIP_TRY(dkid.ensure((size_t)nk * 8));
      KHIP_TRY_HIP(hipMemcpyAsync(doff.p, q->key_offsets, (size_t)(nk + 1) * 8, hipMemcpyHostToDevice, a->stream));
      if (nb) KHIP_TRY_HIP(hipMemcpyAsync(dbytes.p, q->key_bytes, (size_t)nb, hipMemcpyHostToDevice, a->stream));
      KHIP_TRY(dict_find(a->dict, a->stream, doff.as<int64_t>(), dbytes.as<uint8_t>(), nk, dkid.as<int64_t>()));
      KHIP_TRY_HIP(hipMemcpyAsync(k.data(), dkid.p, (size_t)nk * 8, hipMemcpyDeviceToHost, a->stream));
      KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
    }
    std::sort(k.begin(), k.end());
    k.erase(std::unique(k.begin(), k.end()), k.end());
    if (k.size() > 1 && k[0] == -1) k.erase(k.begin());  // -1 (unseen) never matches a row
    KHIP_TRY(dkeys.ensure(k.size() * 8));
    KHIP_TRY_HIP(hipMemcpyAsync(dkeys.p, k.data(), k.size() * 8, hipMemcpyHostToDevice, a->stream));
    pd.keys = dkeys.as<int64_t>();
    pd.n_keys = (int64_t)k.size();
  } else if (q->n_keys > 0) {
    k.assign(q->keys, q->keys + q->n_keys);
    std::sort(k.begin(), k.end());
    k.erase(std::unique(k.begin(), k.end()), k.end());
    KHIP_TRY(dkeys.ensure(k.size() * 8));
    KHIP_TRY_HIP(hipMemcpyAsync(dkeys.p, k.data(), k.size() * 8, hipMemcpyHostToDevice, a->stream));
    pd.keys = dkeys.as<int64_t>();
    pd.n_keys = (int64_t)k.size();
  }
  if (pd.n_keys > 0) pd.host_keys = k.data();
  std::vector<uint64_t> rows;
  int64_t n = 0;
  KHIP_TRY(compact_rows(a, h, &rows, &n, &pd));
  return emit_snapshot(a, rows, n, out);
}

// The rows the last push emitted (khip_agg_changes), computed once per push on first request.
static khip_status compute_changes(khip_agg* a) {
  if (a->chg_ready) return KHIP_OK;
  a->chg_rows.clear();
  a->chg_tomb.clear();
  a->chg_n = 0;
  if (a->desc.emit == KHIP_EMIT_FINAL && a->engine == 2) {
    // the sessions the push closed (sess_push: k_sess_apply / k_sess_keep)
    KHIP_TRY(sess_changes(a, &a->chg_rows, &a->chg_tomb, &a->chg_n));
  } else if (a->desc.emit == KHIP_EMIT_FINAL) {
    // windows closed by the push and still visible when they closed, passing HAVING
    HavingDev fd{};
    fd.fin = 1;
    fd.fin_c0 = a->st_before - a->grace;
    fd.fin_c1 = a->host_stream_time - a->grace;
    fd.fin_size = a->desc.size_ms;
    if (a->desc.time_domain == KHIP_TIME_PARTITION) {
      // per task (partition_bounds): a row closes when ITS partition's stream time passes its end;
      // a row whose key is not in the map closes nowhere
      fd.fin_c0 = fd.fin_c1 = 0;
      bool moved = false;
      for (size_t p = 0; p < a->pst_host.size(); p++) moved = moved || a->pst_host[p] > a->pst_prev_host[p];
      if (moved) fd.fin_c1 = 1;  // (only gates the compaction below)
    }
    DevBuf dl;
    if (!a->lost.empty()) {
      KHIP_TRY(dl.ensure(a->lost.size() * 8));
      KHIP_TRY_HIP(hipMemcpyAsync(dl.p, a->lost.data(), a->lost.size() * 8, hipMemcpyHostToDevice, a->stream));
      fd.lost = dl.as<int64_t>();
      fd.n_lost = (int32_t)(a->lost.size() / 2);
    }
    if (fd.fin_c1 > fd.fin_c0) {
      if (a->desc.time_domain == KHIP_TIME_PARTITION) fd.fin_c1 = 0;
      KHIP_TRY(compact_rows(a, a->desc.has_having ? &a->desc.having : nullptr, &a->chg_rows, &a->chg_n, &fd));
    }
    a->chg_tomb.assign((size_t)a->chg_n, 0);
  } else if (a->changelog && a->engine == 2) {
    KHIP_TRY(sess_changes(a, &a->chg_rows, &a->chg_tomb, &a->chg_n));
  } else if (a->changelog) {
    KHIP_TRY(part_changes(a, &a->chg_rows, &a->chg_tomb, &a->chg_n));
  } else {
    return fail(KHIP_E_STATE, "handle created without KHIP_FLAG_CHANGELOG (EMIT CHANGES)");
  }
  a->chg_ready = true;
  return KHIP_OK;
}

khip_status khip_agg_changes_size(khip_agg* a, int64_t* n_rows, int64_t* key_bytes) {
  clear_error();
  if (!a) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  KHIP_TRY(compute_changes(a));
  if (n_rows) *n_rows = a->chg_n;
  if (key_bytes) {
    int64_t kb = 0;
    if (a->desc.key_type == KHIP_KEY_UTF8 && a->chg_n) {
      std::vector<uint8_t> arena;
      KHIP_TRY(arena_host(a, &arena));
      for (int64_t r = 0; r < a->chg_n; r++) kb += kid_len(arena, (int64_t)a->chg_rows[r * a->sw]);
    }
    *key_bytes = kb;
  }
  return KHIP_OK;
}

khip_status khip_agg_changes(khip_agg* a, khip_snapshot* out, uint8_t* tombstone) {
  clear_error();
  if (!a || !out) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  KHIP_TRY(compute_changes(a));
  return emit_snapshot(a, a->chg_rows, a->chg_n, out, &a->chg_tomb, tombstone);
}

khip_status khip_agg_reset(khip_agg* a) {
  clear_error();
  if (!a) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  a->chg_ready = true;
  a->chg_n = 0;
  a->st_before = -1;
  a->lost.clear();
  if (a->engine == 0) {
    KHIP_TRY(part_reset(a));  // also the stream time
  } else if (a->engine == 2) {
    a->sess.n = 0;
    a->sess.nchg = 0;
    int64_t m1 = -1;
    KHIP_TRY_HIP(hipMemcpyAsync(a->stream_time.p, &m1, 8, hipMemcpyHostToDevice, a->stream));
  } else {
    hipLaunchKernelGGL(k_init_table, dim3(grid_for(a->cap * a->sw, 256)), dim3(256), 0, a->stream,
                       a->table.as<uint64_t>(), a->cap, a->sw, a->init);
    int64_t m1 = -1;
    KHIP_TRY_HIP(hipMemcpyAsync(a->stream_time.p, &m1, 8, hipMemcpyHostToDevice, a->stream));
    if (a->engine == 3) KHIP_TRY(tagg_reset(a));
  }
  if (a->desc.key_type == KHIP_KEY_UTF8) {
    KHIP_TRY(dict_clear(a->dict, a->stream));
  }
  if (a->desc.time_domain == KHIP_TIME_PARTITION) {
    KHIP_TRY_HIP(hipMemsetAsync(a->pst.p, 0xFF, (size_t)a->desc.n_partitions * 8, a->stream));
    a->pst_host.assign((size_t)a->desc.n_partitions, -1);
    a->pst_prev_host.assign((size_t)a->desc.n_partitions, -1);
    a->plost.clear();
    a->plost_off.clear();
    KHIP_TRY(pmap_clear(a));  // forget the keys' partitions (keeps the allocation)
  }
  // asynchronous on the handle's stream (every later call on the handle is ordered behind it)
  KHIP_TRY_HIP(hipGetLastError());
  a->occ = 0;
  a->host_stream_time = -1;
  a->seq_base = 0;
  return KHIP_OK;
}

khip_status khip_agg_sync(khip_agg* a) {
  if (!a) return fail(KHIP_E_INVALID, "null argument");
  DeviceGuard g(a->device);
  KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  return KHIP_OK;
}

khip_status khip_agg_kernel_times(khip_agg* a, khip_kernel_times* out, int32_t reset) {
  if (!a || !out) return fail(KHIP_E_INVALID, "null argument");
  if (!a->profile) return fail(KHIP_E_STATE, "handle created without KHIP_FLAG_PROFILE");
  *out = a->times;
  if (reset) a->times = khip_kernel_times{};
  return KHIP_OK;
}

khip_status khip_agg_stream(khip_agg* a, void** s) {
  if (!a || !s) return fail(KHIP_E_INVALID, "null argument");
  *s = (void*)a->stream;
  return KHIP_OK;
}

khip_status khip_agg_destroy(khip_agg* a) {
  if (!a) return KHIP_OK;
  DeviceGuard g(a->device);
  if (a->stream) hipStreamSynchronize(a->stream);
  DevBuf* bufs[] = {&a->table, &a->blockmax, &a->blockprefix, &a->partials, &a->resume, &a->counters,
                    &a->stream_time, &a->st_keys, &a->st_ts, &a->st_kv, &a->st_rv, &a->st_koff,
                    &a->st_kbytes, &a->kid, &a->khash, &a->chg, &a->lostbuf, &a->lostctr,
                    &a->pst, &a->pst2, &a->st_col, &a->st_agg, &a->st_seen, &a->st_part, &a->seqbuf,
                    &a->nseqbuf};
  for (DevBuf* b : bufs) b->release();
  for (int c = 0; c < MAX_COLS; c++) {
    a->st_cols[c].release();
    a->st_cval[c].release();
  }
  dict_release(a->dict);
  pmap_release(a);
  tagg_release(a);
  part_release(a);
  sess_release(a);
  for (int e = 0; e < 8; e++)
    if (a->ev[e]) hipEventDestroy(a->ev[e]);
  if (a->stream) hipStreamDestroy(a->stream);
  delete a;
  return KHIP_OK;
}

}  // extern "C"
