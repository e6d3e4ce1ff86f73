// khip_agg_c1.hip — the windowed COUNT(*) pipeline of the partitioned engine (C2's query:
// `SELECT k, COUNT(*) ... WINDOW TUMBLING ... GROUP BY k [HAVING ...]`).
//
// Same contract as part_push's general path (khip_agg_part.hip) — per record (SURVEY §8.0,
// Kafka Streams' KStreamWindowAggregate as called from S/StreamAggregateBuilder.java:287-294):
// stream time, TimeWindows.windowsFor, late drop, store update, row time = max ts — but the input
// is read once, and every record moves as 8 bytes:
//
//   k_c1_scatter  keys, ts, validity: every record → (key - kb, ts - T0), two int32s; invalid
//                 records (null key / row, ts < 0) as sentinels; each 4096-record step leaves as
//                 one run in bucket order (B coarse buckets: top bits of the key hash; the
//                 step-run layout: no histogram pass ahead of it).  A tile (16 steps) leaves, per
//                 bucket, each run's place within the tile's share of the bucket (u16, the prefix
//                 over the tile's steps, formed in LDS) and the tile's total; per step the largest
//                 and smallest accepted ts, per tile the counters and the key range.
//                 Optimistic: no record is assumed late.
//   k_c1_runpos   one workgroup per bucket: the exclusive scan of the bucket's tile totals (each
//                 tile's base in the bucket) and the bucket's total.  A run's place in its
//                 bucket = tile base + place within the tile (run_pos): two levels, no scan over
//                 the [bucket][step] counts.
//   k_c1_check    one workgroup: stream time before each 4096-record step (exclusive prefix
//                 max), and the push is ACCEPTED only if no step can hold a late record (the
//                 general path's `fast` test per step), every ts fits ts - T0 in 31 bits and the
//                 keys fit 32 bits above the base kb; otherwise nothing was written and the host
//                 runs the general path (or the same push with kb = the key minimum).
//                 Also the bucket bases (from the bucket totals), the window range, the
//                 group-identity width, the refine's chunk list and, when accepted, the push's
//                 statistics (the tiles' counters summed: no k_part_stats launch).
//   k_c1_chunks   one thread per refine chunk: its first step run and run count (two searches,
//                 each over the tile bases and then the tile's steps)
//   k_c1_refine   per 8K-record chunk of a bucket, read from its step runs: sentinels dropped,
//                 keys rebased to the key minimum, records counting-sorted by their partition
//                 inside the bucket (LDS), written bucket-contiguously; the chunk's per-partition
//                 offsets (u16) go to a segment table
//   k_c1_merge    persistent workgroups, one partition per item: the partition's records are its
//                 segments of the bucket's chunks (an LDS table of prefix | (base - prefix) << 32
//                 per segment, the base relative to the bucket's first record: a lane looks its
//                 AU records up together, c1_seg_lookup, and loads them from the bucket's uniform
//                 base + a 32-bit offset); (key - kmin, window) → a 32-bit identity when
//                 it fits (no key hash on the record path), LDS identity CAS + u32 row-time max +
//                 u32 count, claimed entries listed (the write-out walks the list, not the table);
//                 a last chunk of one or two live slot rows runs a variant that issues nothing
//                 for the other rows; a partition without resident rows skips the count pass;
//                 resident rows merged, closed rows evicted, HAVING counts and changelog flags
//                 maintained exactly as k_part_merge_c1 does (k_part_commit publishes)
//
// Algorithmic bytes per record: 16 + 8 (scatter) + 8 + 8 (refine) + 8 (merge read)
// + the table rows written (32 B per group) — against 16 + 24 + 16 + 8 + rows for the general
// path (DESIGN.md §(d)).
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "khip_part.hpp"

namespace khip {

constexpr int C1_TILE = 65536;   // records per hist / scatter tile (the general path's tile)
constexpr int C1_NT = 512;       // workgroup size of every kernel here
constexpr int C1_CH = 8192;      // refine chunk (records), 16 per thread
// Record loads of the refines and merges: plain loads.  Nontemporal ones (rounds 3-5) re-fetched
// the lines two neighbouring runs or segments share and cost C2 1.94 -> 1.88 ms / step, C5's
// value refine 921 -> 839 us (profiles/r05/ab/record_loads_temporal.txt).
template <class T>
__device__ __forceinline__ T c1_ld(const T* p) {
  return *p;
}
constexpr int C1_SEGMAX = 512;   // chunks of one bucket the merge can hold (4M records)
constexpr int C1_SEGB = 7;       // the merge's segment lookup: one entry per 32, 64 or 128 records of an
constexpr int C1_SEGOF = 512;    // item (the finest that fits 512 entries; past 64K records: binary search)
constexpr uint32_t C1_SENT = 0x80000000u;  // low word of a sentinel record (ts - T0 never is)

__device__ __forceinline__ int bits_of(uint64_t v) { return v ? 64 - __clzll((long long)v) : 0; }

// A c1info word another kernel produced (atomics / stores of the scatters, stores of
// k_c1_check): read with a device-coherent vector load, never through the scalar cache.
__device__ __forceinline__ int64_t ci_ld(const int64_t* ci, int k) {
  const uint64_t v = (uint64_t)__hip_atomic_load(&ci[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // uniform: back into scalar registers
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ------------------------------------------------------------------ step-run layout
// The scatters write no bucket-contiguous output (that needs every tile's bucket counts first: a
// histogram pass over the keys): each step of S records leaves as ONE contiguous run of S records
// in bucket order at out[gs * S]; its per-bucket counts / offsets are held in LDS for the tile's
// SPT steps and leave per bucket at the tile's end (flush_run_counts): roff[b][gs], the bucket's
// offset inside step gs's run; rloc[b][gs], the run's place within the tile's share of the bucket
// (the exclusive prefix of the counts over the tile's steps); ttot[b][tile], the tile's total.
// k_c1_runpos scans each bucket's tile totals (tbase[b][0 .. nT], the last the bucket's total), and
// run_pos gives a (bucket, step) run's place in the bucket's order; the refine reads a bucket's
// chunk from its step runs.  The key range, the time base and the bucket counts are all learned in
// the one read of the input.
template <int U, int NT, class R, bool W>
__device__ __forceinline__ uint32_t stage_step_runs(const R (&rec)[U], const uint32_t (&t32)[U], const uint32_t (&bin)[U],
                                                const bool (&ok)[U], int nb, uint32_t* cnt, uint32_t* sbase, int* wsum,
                                                R* sp, uint32_t* lt32, R* __restrict__ out, uint32_t* __restrict__ outT,
                                                int64_t gs, uint32_t* lrc, uint16_t* lro) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t rank[U];
#pragma unroll
  for (int u = 0; u < U; u++) rank[u] = ok[u] ? atomicAdd(&cnt[bin[u]], 1u) : 0u;
  lds_barrier();
  const uint32_t c = t < nb ? cnt[t] : 0u;
  uint32_t incl = c;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(incl, off, 64);
    if (lane >= off) incl += y;
  }
  if (lane == 63) wsum[wave] = (int)incl;
  lds_barrier();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; k++) {
    before += k < wave ? (uint32_t)wsum[k] : 0u;
    tot += (uint32_t)wsum[k];
  }
  if (t < nb) {
    sbase[t] = before + incl - c;
    lrc[t] = c;  // the step's row of the tile's run counts / offsets (flush_run_counts)
    lro[t] = (uint16_t)(before + incl - c);
    cnt[t] = 0u;
  }
  lds_barrier();
#pragma unroll
  for (int u = 0; u < U; u++)
    if (ok[u]) {
      const uint32_t i = sbase[bin[u]] + rank[u];
      sp[i] = rec[u];
      if (W) lt32[i] = t32[u];
    }
  lds_barrier();
  R* o = out + gs * (int64_t)(U * NT);
  for (uint32_t j = t; j < tot; j += NT) o[j] = sp[j];
  if (W) {
    uint32_t* oT = outT + gs * (int64_t)(U * NT);
    for (uint32_t j = t; j < tot; j += NT) oT[j] = lt32[j];
  }
  // the next step's first barrier (after its rank atomics) orders these LDS reads before any
  // rewrite of sbase / the stage
  return tot;
}

// The step's staged key offsets (key - kb, kbits wide, above bit 32 of the record's first word)
// → the workgroup's LDS minimum / maximum (one atomic pair per wave); registers only for the step.
template <int NT, class R>
__device__ __forceinline__ void step_krange(const R* sp, uint32_t tot, uint32_t kmask, uint32_t* lkr) {
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
  for (uint32_t j = threadIdx.x; j < tot; j += NT) {
    uint64_t w;
    if constexpr (sizeof(R) == 16) w = ((const ulonglong2*)sp)[j].x;
    else w = (uint64_t)((const int64_t*)sp)[j];
    const uint32_t kr = (uint32_t)(w >> 32) & kmask;
    mn = kr < mn ? kr : mn;
    mx = kr > mx ? kr : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx >= mn) {
    atomicMin(&lkr[0], mn);
    atomicMax(&lkr[1], mx);
  }
}

// LDS of a step-run scatter: per bucket its step count and staged base, the staged records (and
// their ts words when W).
__host__ __device__ constexpr size_t run_stage_lds(int nb, int S, int rec_bytes, bool w) {
  return (size_t)nb * 8 + (size_t)S * rec_bytes + (w ? (size_t)S * 4 : 0);
}
// ... then the tile's run counts u32[spt][nb] and offsets u16[spt][nb], written out per bucket at
// the end of the tile
__host__ __device__ constexpr size_t run_cnt_lds(int nb, int spt) { return (size_t)nb * spt * 6; }

// The tile's SPT run places / offsets of bucket b leave as whole 16-byte stores (rloc[b][t * SPT ..],
// roff[b][t * SPT ..]: 32 + 32 B for SPT = 16) instead of 2-byte stores per step and bucket, which
// the memory side turned into 32-byte partial writes (C2: ~250 MB a push).  A run's place is the
// sum of the bucket's counts over the tile's earlier steps: at most C1_TILE less one step, a u16.
// Steps past the input (the last tile's) are empty runs at the end of the tile's share.  Thread b
// wrote row entries lrc[st][b] itself.
template <int SPT, int NT>
__device__ __forceinline__ void flush_run_counts(const uint32_t* lrc, const uint16_t* lro, int B, int st_last, int64_t t,
                                                 int64_t nT, uint16_t* __restrict__ rloc, uint16_t* __restrict__ roff,
                                                 uint32_t* __restrict__ ttot) {
  static_assert(SPT % 8 == 0, "whole 16-byte stores");
  static_assert(C1_TILE - C1_TILE / SPT < 65536, "a run's place within its tile fits a u16");
  const int64_t nSt = nT * SPT;
  for (int b = threadIdx.x; b < B; b += NT) {
    uint16_t* rl = rloc + (int64_t)b * nSt + t * SPT;
    uint16_t* ro = roff + (int64_t)b * nSt + t * SPT;
    uint32_t acc = 0u;
#pragma unroll
    for (int q = 0; q < SPT / 8; q++) {
      uint32_t v[4], w[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int s0 = 8 * q + 2 * k;
        const uint32_t p0 = acc;
        acc += s0 <= st_last ? lrc[s0 * B + b] : 0u;
        const uint32_t p1 = acc;
        acc += s0 + 1 <= st_last ? lrc[(s0 + 1) * B + b] : 0u;
        v[k] = p0 | p1 << 16;
        const uint32_t lo = s0 <= st_last ? lro[s0 * B + b] : 0u, hi = s0 + 1 <= st_last ? lro[(s0 + 1) * B + b] : 0u;
        w[k] = lo | hi << 16;
      }
      *(uint4*)(rl + 8 * q) = make_uint4(v[0], v[1], v[2], v[3]);
      *(uint4*)(ro + 8 * q) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    ttot[(int64_t)b * nT + t] = acc;
  }
}

// A (bucket, step) run's place in its bucket's order: the tile's base (tb: the bucket's row of
// k_c1_runpos's scan, nT + 1 entries) + the run's place within the tile (rl: the bucket's row of
// rloc).  s = nSt: the bucket's total, the end of its last run.  sh = log2 of the steps per tile.
__device__ __forceinline__ int64_t run_pos(const uint32_t* __restrict__ tb, const uint16_t* __restrict__ rl, int64_t nSt,
                                           int sh, int64_t s) {
  return (int64_t)tb[s >> sh] + (s < nSt ? (int64_t)rl[s] : 0);
}

// The time base, the key base and the tile's key range — shared by both scatters.  T0: the stream
// time before the push, else the first ts (k_c1_check's 31-bit ts test is relative to it).  kb:
// the host's base (the last push's key minimum less a margin), else keys[0] − half the key field;
// the records hold (key − kb), and k_c1_check rebases them to the push's key minimum (CI_KSHIFT)
// or declines when some key falls outside the field.
__device__ __forceinline__ void run_bases(const int64_t* __restrict__ keys, const int64_t* __restrict__ ts, int64_t n,
                                          const int64_t* __restrict__ stream_time, int64_t kb_in, int has_kb,
                                          int kfield, int64_t* ci, int64_t* T0, int64_t* kb) {
  const int64_t st0 = *stream_time;
  const int64_t t0 = n > 0 ? ts[0] : 0;
  *T0 = st0 >= 0 ? st0 : (t0 > 0 ? t0 : 0);
  *kb = has_kb ? kb_in : (int64_t)((uint64_t)keys[0] - (1ULL << (kfield - 1)));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ci[CI_T0] = *T0;
    ci[CI_KBASE] = *kb;
  }
}

// The workgroup's key range → CI_KMIN / CI_KMAX atomics (kb + the staged offsets' extremes), and
// CI_KFAIL when some key fell outside the record's key field above kb (thread 0, after the loop).
__device__ __forceinline__ void run_krange(const uint32_t* lkr, int kfail, int64_t kb, int64_t* ci) {
  if (lkr[1] >= lkr[0]) {
    atomicMin((long long*)&ci[CI_KMIN], (long long)((uint64_t)kb + lkr[0]));
    atomicMax((long long*)&ci[CI_KMAX], (long long)((uint64_t)kb + lkr[1]));
  }
  if (kfail) atomicOr((unsigned long long*)&ci[CI_KFAIL], 1ULL);
}

// ------------------------------------------------------------------ k_c1_scatter
// Records of tile t → step runs.  8-byte record: (key - kb) << 32 | (uint32)(ts - T0); invalid
// records keep their key word (their bucket is the key's) with the sentinel low word.
// WIDE (the key range does not fit 32 bits): the record is the 64-bit key hash (key = its inverse)
// and ts - T0 goes to a parallel u32 array (srecT), staged beside it.
template <int U, int NT, bool WIDE, bool ST>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_c1_scatter(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ ts, const uint8_t* __restrict__ kv,
    const uint8_t* __restrict__ rv, int64_t n, int64_t nT, int log2B, uint16_t* __restrict__ rloc,
    uint16_t* __restrict__ roff, uint32_t* __restrict__ ttot, uint64_t* __restrict__ srec, int64_t* __restrict__ tilestat,
    int64_t* __restrict__ tpart, int64_t* __restrict__ ci, const int64_t* __restrict__ st_at,
    uint32_t* __restrict__ srecT, int64_t size, int64_t adv, FastDiv fd, int64_t grace,
    const int64_t* __restrict__ stream_time, int64_t kb_in, int has_kb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int wsum[NT / 64];
  __shared__ unsigned long long lc[4];
  __shared__ int lt[2][2];  // [step parity][max | min] of the step's accepted ts - T0 (LDS atomics)
  __shared__ int lfail, lkfail;
  __shared__ uint32_t lkr[2];  // min / max of the staged key offsets (not WIDE)
  constexpr int S = U * NT;
  constexpr int SPT = C1_TILE / S;
  const int B = 1 << log2B;
  const int64_t t = tile_of(blockIdx.x, nT);
  uint32_t* cnt = (uint32_t*)smem;
  uint32_t* sbase = cnt + B;
  int64_t* sp = (int64_t*)(smem + (size_t)B * 8);
  uint32_t* lt32 = (uint32_t*)(sp + S);  // WIDE: the staged ts - T0
  uint32_t* lrc = (uint32_t*)(smem + run_stage_lds(B, S, 8, WIDE));
  uint16_t* lro = (uint16_t*)(lrc + SPT * B);
  for (int b = threadIdx.x; b < B; b += NT) cnt[b] = 0u;
  if (threadIdx.x < 4) lc[threadIdx.x] = 0;
  if (threadIdx.x < 2) {
    lt[threadIdx.x][0] = INT32_MIN;
    lt[threadIdx.x][1] = INT32_MAX;
  }
  if (threadIdx.x == 0) {
    lfail = lkfail = 0;
    lkr[0] = 0xFFFFFFFFu;
    lkr[1] = 0u;
  }
  int64_t T0, kb;
  run_bases(keys, ts, n, stream_time, kb_in, has_kb, 32, ci, &T0, &kb);
  const int shift = log2B == 0 ? 64 : 64 - log2B;
  const uint32_t bmask = (uint32_t)(B - 1);
  const int64_t base = t * C1_TILE;
  const int64_t end = base + C1_TILE < n ? base + C1_TILE : n;
  int c_acc = 0, c_nk = 0, c_nr = 0, c_bt = 0;  // < 2^16 per tile
  uint32_t kor = 0u;
  int64_t x[U], k[U];
  auto load_step = [&](int64_t i0, int64_t (&dx)[U], int64_t (&dk)[U]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      int64_t i = i0 + (int64_t)u * NT;
      i = i < end ? i : end - 1;
      dx[u] = ts[i];
      dk[u] = keys[i];
    }
  };
  // Thread 0 folds each step's accepted-ts range (LDS slots lt[st & 1], reset for step st + 2)
  // into the tile's late-record summary for k_c1_check: the stream-time maximum, the smallest ts,
  // the largest stream time every step stays below (bound: the step's earliest window still
  // open, S/StreamAggregateBuilder.java:272-277) and whether the tile's own running maximum
  // already passes a step's bound.  The check then needs only the stream time carried INTO the
  // tile: carry <= bound (and ok) <=> no record of the tile is late.
  int64_t t_rmax = -1, t_min = INT64_MAX, t_bound = INT64_MAX;
  bool t_ok = true;
  auto publish = [&](int64_t, int st) {
    const int mx = lt[st & 1][0], mn = lt[st & 1][1];
    if (mx != INT32_MIN) {
      const int64_t smx = T0 + mx, smn = T0 + mn;
      t_rmax = smx > t_rmax ? smx : t_rmax;
      t_min = smn < t_min ? smn : t_min;
      const int64_t fw = first_window_start_fd(smn, size, adv, fd) + size;
      const int64_t b = grace > ((int64_t)1 << 61) ? INT64_MAX : fw + grace - 1;
      t_bound = b < t_bound ? b : t_bound;
      t_ok = t_ok && t_rmax <= b;
    }
    lt[st & 1][0] = INT32_MIN;
    lt[st & 1][1] = INT32_MAX;
  };
  lds_barrier();
  int64_t s0 = base;
  int st_last = -1;
  if (s0 < end) load_step(s0 + threadIdx.x, x, k);
  for (int st = 0; s0 < end; s0 += S, st++) {  // uniform across the block: barriers inside
    st_last = st;
    const int64_t i0 = s0 + threadIdx.x;
    bool ok[U];
    uint32_t bin[U], t32[U];
    int64_t rec[U];
    // this step's accepted ts range, relative to T0 (k_c1_check's late test): 32-bit, every
    // accepted ts - T0 and stream time - T0 fits (else tfail declines the push)
    int tmx = INT32_MIN, tmn = INT32_MAX;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = i0 + (int64_t)u * NT;
      ok[u] = i < end;
      const bool kok = bit_get(kv, ok[u] ? i : base), rok = bit_get(rv, ok[u] ? i : base);
      const bool valid = ok[u] && kok && rok && x[u] >= 0;
      c_nk += ok[u] && !kok;
      c_nr += ok[u] && kok && !rok;
      c_bt += ok[u] && kok && rok && x[u] < 0;
      c_acc += valid;
      const int64_t sx = ST ? st_at[ok[u] ? i : base] : x[u];  // ABI 5 domains: the given stream time
      const int64_t d = x[u] - T0;
      if (valid && (d <= (int64_t)INT32_MIN || d > (int64_t)INT32_MAX)) {  // rare: an LDS flag, not a loop-carried mask
        lfail = 1;
#ifdef KHIP_TUNING
        if (ci[CI_N - 1] == 1 && (threadIdx.x & 63) == 0) printf("[c1 scatter] t %ld i %ld x %ld T0 %ld\n", (long)t, (long)i, (long)x[u], (long)T0);
#endif
      }
      if constexpr (ST) {
        const int64_t ds = sx - T0;
        if (valid && (ds <= (int64_t)INT32_MIN || ds > (int64_t)INT32_MAX)) lfail = 1;
        tmx = valid && (int)ds > tmx ? (int)ds : tmx;
      } else {
        tmx = valid && (int)d > tmx ? (int)d : tmx;
      }
      tmn = valid && (int)d < tmn ? (int)d : tmn;
      const uint64_t hk = key_hash(k[u]);
      bin[u] = stage_bin(hk, shift, bmask);
      t32[u] = valid ? (uint32_t)d : C1_SENT;
      const uint64_t kd = (uint64_t)k[u] - (uint64_t)kb;
      if (!WIDE) kor |= ok[u] ? (uint32_t)(kd >> 32) : 0u;  // nonzero: a key outside the field above kb
      rec[u] = WIDE ? (int64_t)hk : (int64_t)((kd << 32) | (uint64_t)t32[u]);
    }
    // the next step's loads go into x / k (dead now) and stay in flight through this step's stage
    if (s0 + S < end) load_step(i0 + S, x, k);
    const uint32_t tot = stage_step_runs<U, NT, int64_t, WIDE>(rec, t32, bin, ok, B, cnt, sbase, wsum, sp, lt32,
                                                               (int64_t*)srec, srecT, t * SPT + st, lrc + st * B,
                                                               lro + st * B);
    if (!WIDE) step_krange<NT, int64_t>(sp, tot, 0xFFFFFFFFu, lkr);
    // the step's ts range: the wave's first (one LDS atomic per wave, not 64 to one address),
    // after the stage so that its registers are free; published by thread 0 one step later
    // (after the next stage's barriers), the last step's after the loop
    for (int off = 32; off > 0; off >>= 1) {
      const int a = __shfl_xor(tmx, off, 64), b = __shfl_xor(tmn, off, 64);
      tmx = a > tmx ? a : tmx;
      tmn = b < tmn ? b : tmn;
    }
    if ((threadIdx.x & 63) == 0 && tmx != INT32_MIN) {
      atomicMax(&lt[st & 1][0], tmx);
      atomicMin(&lt[st & 1][1], tmn);
    }
    if (threadIdx.x == 0 && st > 0) publish(s0 - S, st - 1);
  }
  flush_run_counts<SPT, NT>(lrc, lro, B, st_last, t, nT, rloc, roff, ttot);
  if (!WIDE && kor) lkfail = 1;
  __syncthreads();
  if (threadIdx.x == 0 && s0 > base) publish(s0 - S, st_last);
  if (!WIDE && threadIdx.x == 0) run_krange(lkr, lkfail, kb, ci);
  c_acc = wave_sum(c_acc);
  c_nk = wave_sum(c_nk);
  c_nr = wave_sum(c_nr);
  c_bt = wave_sum(c_bt);
  if ((threadIdx.x & 63) == 0) {
    if (c_acc) atomicAdd(&lc[0], (unsigned long long)c_acc);
    if (c_nk) atomicAdd(&lc[1], (unsigned long long)c_nk);
    if (c_nr) atomicAdd(&lc[2], (unsigned long long)c_nr);
    if (c_bt) atomicAdd(&lc[3], (unsigned long long)c_bt);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* tp = tpart + t * T_NPART;
    tp[T_ACCEPTED] = (int64_t)lc[0];
    tp[T_NULL_KEY] = (int64_t)lc[1];
    tp[T_NULL_ROW] = (int64_t)lc[2];
    tp[T_BAD_TS] = (int64_t)lc[3];
    tp[T_APPLIED] = (int64_t)lc[0];  // TUMBLING: one window per accepted record, none late (checked)
    tp[T_LATE] = 0;
    if (lfail) atomicOr((unsigned long long*)&ci[CI_TFAIL], 1ULL);
    int64_t* ts4 = tilestat + t * 4;
    ts4[0] = t_rmax;
    ts4[1] = t_min;
    ts4[2] = t_bound;
    ts4[3] = t_ok ? 1 : 0;
  }
}

// The exact key range of a push (the host's fallback when a key fell outside the key field; keys
// every `stride` words):
// out[0] = max of ~key (= ~min), out[1] = max of key (both start at INT64_MIN).
__global__ __launch_bounds__(256) void k_c1_krange(const int64_t* __restrict__ keys, int64_t stride, int64_t n,
                                                   long long* __restrict__ out) {
  int64_t mx = INT64_MIN, mxn = INT64_MIN;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = keys[i * stride];
    mx = k > mx ? k : mx;
    mxn = ~k > mxn ? ~k : mxn;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t a = __shfl_xor(mx, off, 64), b = __shfl_xor(mxn, off, 64);
    mx = a > mx ? a : mx;
    mxn = b > mxn ? b : mxn;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&out[0], (long long)mxn);
    atomicMax(&out[1], (long long)mx);
  }
}

// Each tile's base in its bucket and each bucket's total: workgroup b scans bucket b's nT tile
// totals (exclusive, bucket-relative) into tbase[b][0 .. nT), the total into tbase[b][nT].  No
// workgroup waits for another.
__global__ __launch_bounds__(1024) void k_c1_runpos(const uint32_t* __restrict__ ttot, int64_t nT,
                                                    uint32_t* __restrict__ tbase) {
  __shared__ uint32_t wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t* in = ttot + (int64_t)blockIdx.x * nT;
  uint32_t* out = tbase + (int64_t)blockIdx.x * (nT + 1);
  uint32_t carry = 0u;
  for (int64_t t0 = 0; t0 < nT; t0 += 1024) {  // uniform across the block: barriers inside
    const int64_t t = t0 + threadIdx.x;
    const uint32_t c = t < nT ? in[t] : 0u;
    uint32_t incl = c;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, tot = 0u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      before += k < wave ? wsum[k] : 0u;
      tot += wsum[k];
    }
    if (t < nT) out[t] = carry + before + incl - c;
    carry += tot;
    __syncthreads();  // wsum is rewritten by the next round
  }
  if (threadIdx.x == 0) out[nT] = carry;
}

// Refine work item w → its bucket (cstart), its first step s0 and run count R (cinfo[2w],
// [2w + 1]): one thread per item, binary searches over cstart and the bucket's run positions —
// first the tile (over the nT tile bases), then the step inside it (over its 2^sh places) — so a
// refine workgroup starts with one round of table loads, not the searches.  Positions are relative
// to the bucket's first record.  Empty runs share their position with the next run: s0 is the
// LAST step starting at or before the chunk, the end the FIRST step starting at or past its end.
__global__ __launch_bounds__(256) void k_c1_chunks(const int* __restrict__ cstart, int B,
                                                   const uint32_t* __restrict__ tbase, const uint16_t* __restrict__ rloc,
                                                   int64_t nT, int sh, int ch, const int64_t* __restrict__ ci,
                                                   uint32_t* __restrict__ cinfo) {
  if (ci_ld(ci, CI_GATE) == 0) return;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (int)ci_ld(ci, CI_NCHUNK)) return;
  int a = 0, e = B;  // the last bucket with cstart[b] <= w, in [a, e)
  while (e - a > 1) {
    const int m = (a + e) >> 1;
    if (cstart[m] <= w) a = m;
    else e = m;
  }
  const int b = a;
  const int64_t nSt = nT << sh, spt = (int64_t)1 << sh;
  const uint32_t* tb = tbase + (int64_t)b * (nT + 1);
  const uint16_t* rl = rloc + (int64_t)b * nSt;
  const int64_t lo = (int64_t)(w - cstart[b]) * ch, blen = (int64_t)tb[nT];
  const int64_t hi = blen - lo < ch ? blen : lo + ch;
  // s0 (sa): the last step whose run starts at or before lo.  The end: the first step after s0
  // whose run starts at or past the chunk's end (or nSt), one past sl, the last step starting
  // before it.  The two searches advance together, so their loads overlap: first the tiles (tb[0]
  // = 0 passes both tests), then the 2^sh steps of each one's tile (whose first place is 0).
  int64_t t0 = 0, e0 = nT, t1 = 0, e1 = nT;
  while (e0 - t0 > 1 || e1 - t1 > 1) {
    const int64_t m0 = (t0 + e0) >> 1, m1 = (t1 + e1) >> 1;  // (a finished search reloads its answer)
    const int64_t p0 = (int64_t)tb[m0], p1 = (int64_t)tb[m1];
    if (e0 - t0 > 1) {
      if (p0 <= lo) t0 = m0;
      else e0 = m0;
    }
    if (e1 - t1 > 1) {
      if (p1 < hi) t1 = m1;
      else e1 = m1;
    }
  }
  const int64_t b0 = (int64_t)tb[t0], b1 = (int64_t)tb[t1];
  int64_t sa = t0 << sh, sl = t1 << sh;
  for (int64_t half = spt >> 1; half > 0; half >>= 1) {
    const int64_t q0 = b0 + (int64_t)rl[sa + half], q1 = b1 + (int64_t)rl[sl + half];
    if (q0 <= lo) sa += half;
    if (q1 < hi) sl += half;
  }
  cinfo[2 * w] = (uint32_t)sa;
  cinfo[2 * w + 1] = (uint32_t)(sl + 1 - sa);
}

// The chunk's source positions: map[j] = where the chunk's record j lies in the step runs (u32 per
// record, in the refine's not yet used stage).  One thread per run of the chunk (cinfo): one round
// of loads of its position / end / step offset, then the run's slice of the map.  lo: the chunk's
// first record, relative to the bucket's (as the run positions are).
__device__ __forceinline__ void chunk_map(const uint32_t* __restrict__ tb, const uint16_t* __restrict__ rl,
                                          const uint16_t* __restrict__ ro, int64_t nSt, int sh,
                                          const uint32_t* __restrict__ cinfo, int w, int64_t S, int64_t lo, int len,
                                          uint32_t* map) {
  const int64_t s0 = cinfo[2 * w];
  const int R = (int)cinfo[2 * w + 1];
  for (int k = threadIdx.x; k < R; k += blockDim.x) {
    const int64_t s = s0 + k, p = run_pos(tb, rl, nSt, sh, s), pe = run_pos(tb, rl, nSt, sh, s + 1);
    const int64_t a = p > lo ? p : lo, e = pe < lo + len ? pe : lo + len;
    const uint32_t src = (uint32_t)(s * S + (int64_t)ro[s] + (a - p));
    for (int64_t x = a; x < e; x++) map[x - lo] = src + (uint32_t)(x - a);
  }
  __syncthreads();
}

// ------------------------------------------------------------------ k_c1_check
// One workgroup.  Accept the push when no scatter step (4096 consecutive records) can hold a late
// record: the step's earliest window outlives the largest stream time the step reaches,
// max(stream time before the step, the step's max ts) - grace (the general path's per-tile `fast`
// test at step granularity; S/StreamAggregateBuilder.java:272-277 for the grace).
// Accepted: publish the stream time, the window range (k_part_wrange's rules, resident rows
// included), the identity width and the refine's chunk list (cstart); reset the counters the
// merge and commit use, and write the push's statistics (the tiles' counters tpart, summed:
// ctr[CTR_TILE ..], what k_part_stats computes on the general path).  Declined: nothing persistent
// is touched.  Either way the bucket bases bb[0 .. B] (scratch of this push) from the bucket
// totals tbase[b][nT] (k_c1_runpos).
__global__ __launch_bounds__(1024) void k_c1_check(
    const int64_t* __restrict__ tilestat, const int64_t* __restrict__ tpart, int64_t nT, int64_t size, int64_t adv,
    FastDiv fd, int64_t grace, int64_t close0, int fresh, int log2B, int log2P, int wide, int ch, int kbmax, int pbits,
    const uint32_t* __restrict__ tbase, int64_t* __restrict__ bb, int* __restrict__ cstart,
    int64_t* __restrict__ ci, int64_t* __restrict__ stream_time, int64_t* __restrict__ res,
    unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ closed_ctr, unsigned long long closed_n) {
  __shared__ int64_t wmx[16];
  __shared__ int64_t red[2][16];
  __shared__ unsigned long long lsum[T_NPART];  // the tiles' counters, summed
  __shared__ int lslow;
  __shared__ int64_t wtot[8];  // per wave of the first B threads: the buckets' records,
  __shared__ int wnch[8], wmxc[8];  // chunks and largest chunk count
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) lslow = 0;
  if (threadIdx.x < T_NPART) lsum[threadIdx.x] = 0ULL;
  // thread b < B: bucket b's total (k_c1_runpos), in flight during the tile loops
  const int B = 1 << log2B;
  const uint32_t btot = (int)threadIdx.x < B ? tbase[(int64_t)threadIdx.x * (nT + 1) + nT] : 0u;
  const int64_t st0 = *stream_time;
  // thread j owns tiles [j K, (j + 1) K): their stream-time maximum, the block's exclusive prefix
  // of those (the stream time carried into each tile), then each tile's summary (k_c1_scatter)
  const int64_t K = (nT + 1023) / 1024;
  const int64_t g0 = threadIdx.x * K, g1 = g0 + K < nT ? g0 + K : nT;
  int64_t m = -1;
  for (int64_t g = g0; g < g1; g++) m = tilestat[4 * g] > m ? tilestat[4 * g] : m;
  const int64_t incl = wave_incl_max(m);
  if (lane == 63) wmx[wave] = incl;
  __syncthreads();
  int64_t pre = st0;
  for (int w = 0; w < wave; w++) pre = wmx[w] > pre ? wmx[w] : pre;
  const int64_t excl = __shfl_up(incl, 1, 64);
  int64_t run = lane == 0 ? pre : (excl > pre ? excl : pre);  // stream time before tile g0
  int64_t gmn = INT64_MAX, gmx = -1;
  int64_t tsum[T_NPART] = {};  // the tiles' counters (k_c1_scatter), summed
  bool slow = false;
  for (int64_t g = g0; g < g1; g++) {
    const int64_t* t4 = tilestat + 4 * g;
    const int64_t mx = t4[0], mn = t4[1];
    if (mn != INT64_MAX) {
      slow |= t4[3] == 0 || run > t4[2];  // a record of the tile may be late
      gmn = mn < gmn ? mn : gmn;
    }
    run = mx > run ? mx : run;
    gmx = mx > gmx ? mx : gmx;
#pragma unroll
    for (int k = 0; k < T_NPART; k++) tsum[k] += tpart[g * T_NPART + k];
  }
  if (slow) lslow = 1;
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t a = __shfl_xor(gmn, off, 64), b = __shfl_xor(gmx, off, 64);
    gmn = a < gmn ? a : gmn;
    gmx = b > gmx ? b : gmx;
  }
#pragma unroll
  for (int k = 0; k < T_NPART; k++) tsum[k] = wave_sum(tsum[k]);
  if (lane == 0) {
    red[0][wave] = gmn;
    red[1][wave] = gmx;
#pragma unroll
    for (int k = 0; k < T_NPART; k++)
      if (tsum[k]) atomicAdd(&lsum[k], (unsigned long long)tsum[k]);
  }
  // the buckets' totals → bucket bases, chunks per bucket → cstart: exclusive prefixes over the
  // first B threads (B <= 512: waves 0 .. 7), each writing its own bucket's; the largest bucket's
  // chunk count
  const int nch = (int)((btot + (uint32_t)ch - 1u) / (uint32_t)ch);  // (btot < 2^31: no wrap)
  int64_t itot = (int64_t)btot;
  int inch = nch, mnch = nch;
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t y = __shfl_up(itot, off, 64);
    const int z = __shfl_up(inch, off, 64), q = __shfl_xor(mnch, off, 64);
    if (lane >= off) {
      itot += y;
      inch += z;
    }
    mnch = q > mnch ? q : mnch;
  }
  if (lane == 63 && wave < 8) {
    wtot[wave] = itot;
    wnch[wave] = inch;
    wmxc[wave] = mnch;
  }
  __syncthreads();
  if ((int)threadIdx.x < B) {
    int64_t bt = 0;
    int bn = 0;
    for (int w = 0; w < wave; w++) {
      bt += wtot[w];
      bn += wnch[w];
    }
    bb[threadIdx.x] = bt + itot - (int64_t)btot;
    cstart[threadIdx.x] = bn + inch - nch;
  }
  if (threadIdx.x) return;
  for (int w = 0; w < 16; w++) {
    gmn = red[0][w] < gmn ? red[0][w] : gmn;
    gmx = red[1][w] > gmx ? red[1][w] : gmx;
  }
  int acc = 0, mxc = 0;
  int64_t base = 0;
  for (int w = 0; w < 8; w++) {  // (waves past the B threads hold zeros)
    base += wtot[w];
    acc += wnch[w];
    mxc = wmxc[w] > mxc ? wmxc[w] : mxc;
  }
  bb[B] = base;
  cstart[B] = acc;
  const int64_t kmin = ci_ld(ci, CI_KMIN), kmax = ci_ld(ci, CI_KMAX);
  const bool tfail = ci_ld(ci, CI_TFAIL) != 0, kfail = ci_ld(ci, CI_KFAIL) != 0;
  ci[CI_KMIN] = INT64_MAX;  // ready for the next push's atomics
  ci[CI_KMAX] = INT64_MIN;
  ci[CI_TFAIL] = 0;
  ci[CI_KFAIL] = 0;
  // (wide records: the scatter tracks no key range)
  bool ok = !lslow && !tfail && mxc <= C1_SEGMAX && (wide || kmax >= kmin);
#ifdef KHIP_TUNING
  if (ci[CI_N - 1] == 1)  // debug (tuning build, KHIP_C1_DEBUG=1): the decision's inputs
    printf("[c1 check] tfail %d slow %d mxc %d kmin %ld kmax %ld gmn %ld gmx %ld T0 %ld st0 %ld nT %ld\n", (int)tfail,
           (int)lslow, mxc, (long)kmin, (long)kmax, (long)gmn, (long)gmx, (long)ci[CI_T0], (long)st0, (long)nT);
#endif
  // compact records: every key within the key field above the push's base kb (the scatters wrote
  // key - kb; kfail: some key was not — the host then learns the true range and re-runs the push
  // with kb = kmin, or with wide records), and the range within 32 key bits (value records 31)
  const uint64_t krange = kmax >= kmin ? (uint64_t)kmax - (uint64_t)kmin : 0;
  const bool fits = !wide && !kfail && krange < ((1ULL << kbmax) - 1);
  const int64_t kb = ci_ld(ci, CI_KBASE);
  ci[CI_FITS] = fits ? 1 : 0;
  ci[CI_REASON] = ok && !wide && kfail ? 2 : (ok && !wide && !fits ? 1 : 0);
  ci[CI_KMINC] = kmin;
  ci[CI_KSHIFT] = (int64_t)((uint64_t)kmin - (uint64_t)kb);
  ok = ok && (wide || fits);
  // window range of this push's records and of the live resident rows (k_part_wrange)
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  if (gmx >= 0) {
    const int64_t l = gmn - size + adv;
    lo = (int64_t)fast_udiv((uint64_t)(l > 0 ? l : 0), fd);
    hi = (int64_t)fast_udiv((uint64_t)gmx, fd);
  }
  if (!fresh) {
    int64_t rlo = res[0];
    const int64_t rhi = res[1];
    if (close0 != INT64_MIN && rlo != INT64_MAX) {  // live: ws > close0 - size
      const int64_t c = close0 - size;
      const int64_t lb = c >= 0 ? (int64_t)fast_udiv((uint64_t)c, fd) + 1 : 0;
      rlo = rlo > lb ? rlo : lb;
    }
    lo = rlo < lo ? rlo : lo;
    hi = rhi > hi ? rhi : hi;
  }
  const bool none = lo > hi;  // nothing live, nothing new
  if (none) lo = hi = 0;
  ok = ok && (uint64_t)(hi - lo) < (wide ? ((uint64_t)1 << log2P) - 1 : (pbits ? 0x7FFFFFFEull : 0xFFFFFFFEull));
  const int wbits = bits_of((uint64_t)(hi - lo)), kbits = bits_of(krange);
  ci[CI_GATE] = ok ? 1 : 0;
  if (!ok) return;
  ci[CI_WBASE] = lo;
  ci[CI_WHI] = hi - lo;
  ci[CI_WBITS] = wbits;
  ci[CI_KBITS] = kbits;
  ci[CI_KRANGE] = (int64_t)krange;
  ci[CI_ID32] = !wide && kbits + wbits + pbits <= 31 ? 1 : 0;  // pbits: the pane flag
  ci[CI_WIDE] = wide;
  ci[CI_TMIN] = gmx >= 0 ? gmn : 0;
  ci[CI_TMAX] = gmx;
  ci[CI_NCHUNK] = acc;
  *stream_time = gmx > st0 ? gmx : st0;
  res[0] = none ? INT64_MAX : lo;
  res[1] = none ? INT64_MIN : hi;
  ctr[CTR_ADDED] = ctr[CTR_FAILED] = ctr[CTR_NEED] = 0ULL;
  for (int k = 0; k < T_NPART; k++) ctr[CTR_TILE + k] = lsum[k];
  if (closed_ctr) *closed_ctr = closed_n;
}

// ------------------------------------------------------------------ k_c1_refine
// Work item w = chunk c of bucket b (cstart): its records are counting-sorted by partition
// inside the bucket (F = 2^fbits bins) in LDS and written back to the same positions of the
// output; seg[w][f] (u16) = partition f's first record in the chunk, seg[w][F] = valid records.
// WIDE: records are key hashes (srcA / srec) with ts - T0 in parallel u32 arrays (srcAT / srecT);
// the two are staged one after the other through the same LDS.
template <int U, int NT, bool WIDE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_c1_refine(
    const uint64_t* __restrict__ srcA, const int64_t* __restrict__ bb, const int* __restrict__ cstart, int log2B,
    int log2P, int fbits, uint64_t* __restrict__ srec, uint16_t* __restrict__ seg, const int64_t* __restrict__ ci,
    const uint32_t* __restrict__ srcAT, uint32_t* __restrict__ srecT, const uint32_t* __restrict__ tbase,
    const uint16_t* __restrict__ rloc, const uint16_t* __restrict__ roff, int64_t nT, int sh, int64_t S,
    const uint32_t* __restrict__ cinfo) {
  if (ci_ld(ci, CI_GATE) == 0) return;
  const int w = blockIdx.x;
  if (w >= (int)ci_ld(ci, CI_NCHUNK)) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int lb, lnv;
  __shared__ int wsum[NT / 64];
  static_assert(U * NT == C1_CH, "refine chunk");
  const int F = 1 << fbits, B = 1 << log2B;
  uint32_t* cnt = (uint32_t*)smem;
  uint32_t* sbase = cnt + F;
  uint64_t* stage = (uint64_t*)(smem + (size_t)F * 8);
  for (int f = threadIdx.x; f < F; f += NT) cnt[f] = 0u;
  if (threadIdx.x == 0) lb = -1;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += NT)
    if (cstart[b] <= w && w < cstart[b + 1]) lb = b;
  __syncthreads();
  const int b = lb;
  if (b < 0) return;  // (cannot happen: w < cstart[B])
  const int64_t lo = bb[b] + (int64_t)(w - cstart[b]) * C1_CH;
  const int64_t bend = bb[b + 1];
  const int len = (int)(bend - lo < C1_CH ? bend - lo : C1_CH);
  const int64_t kmin = ci_ld(ci, CI_KMINC);
  const uint64_t kshift = WIDE ? 0 : (uint64_t)ci_ld(ci, CI_KSHIFT) << 32;  // records hold key - kb
  const int shift = 64 - log2P;
  // where the chunk's records lie in the step runs (a map in the not yet used stage)
  const int64_t nSt = nT << sh;
  chunk_map(tbase + (int64_t)b * (nT + 1), rloc + (int64_t)b * nSt, roff + (int64_t)b * nSt, nSt, sh, cinfo, w, S,
            lo - bb[b], len, (uint32_t*)stage);
  uint64_t r[U];
  uint32_t f[U], rank[U], t32[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = threadIdx.x + u * NT;
    const uint32_t src = ((const uint32_t*)stage)[j < len ? j : len - 1];
    r[u] = c1_ld(srcA + src) - kshift;
    if constexpr (WIDE) t32[u] = c1_ld(srcAT + src);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = threadIdx.x + u * NT;
    const bool v = j < len && (WIDE ? t32[u] : (uint32_t)r[u]) != C1_SENT;
    f[u] = WIDE ? (uint32_t)(r[u] >> shift) & (uint32_t)(F - 1)
                : (uint32_t)(key_hash(kmin + (int64_t)(r[u] >> 32)) >> shift) & (uint32_t)(F - 1);
    rank[u] = v ? atomicAdd(&cnt[f[u]], 1u) : 0xFFFFFFFFu;
  }
  __syncthreads();
  // exclusive scan of the F counts (F <= NT)
  {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t c = t < F ? cnt[t] : 0u;
    uint32_t incl = c;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = (int)incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
      before += k < wave ? (uint32_t)wsum[k] : 0u;
      tot += (uint32_t)wsum[k];
    }
    if (t < F) {
      sbase[t] = before + incl - c;
      seg[(int64_t)w * (F + 1) + t] = (uint16_t)(before + incl - c);
    }
    if (t == 0) {
      seg[(int64_t)w * (F + 1) + F] = (uint16_t)tot;
      lnv = (int)tot;
    }
  }
  __syncthreads();
  const int nv = lnv;
#pragma unroll
  for (int u = 0; u < U; u++)
    if (rank[u] != 0xFFFFFFFFu) stage[sbase[f[u]] + rank[u]] = r[u];
  __syncthreads();
  for (int j = threadIdx.x; j < nv; j += NT) srec[lo + j] = stage[j];
  if constexpr (WIDE) {  // the ts words through the same LDS
    __syncthreads();
    uint32_t* stage32 = (uint32_t*)stage;
#pragma unroll
    for (int u = 0; u < U; u++)
      if (rank[u] != 0xFFFFFFFFu) stage32[sbase[f[u]] + rank[u]] = t32[u];
    __syncthreads();
    for (int j = threadIdx.x; j < nv; j += NT) srecT[lo + j] = stage32[j];
  }
}

// KHIP_AGG_PROBE (tuning build): wall-clock time per merge phase summed over the persistent
// workgroups (thread 0's view): 0 item start + eviction, 1 records, 2 pane fold, 3 mark + count
// + reserve, 4 write-out.  dbg == nullptr in every other run.
#ifdef KHIP_TUNING
#define C1M_T(k)                                                                        \
  do {                                                                                  \
    if (dbg && threadIdx.x == 0) {                                                      \
      const unsigned long long now_ = wall_clock64();                                   \
      atomicAdd(&dbg[(k)], now_ - t_last);                                              \
      t_last = now_;                                                                    \
    }                                                                                   \
  } while (0)
#define C1M_T0 unsigned long long t_last = dbg ? wall_clock64() : 0ULL
#else  // the release build carries no probe (its registers would cost the merge)
#define C1M_T(k) \
  do {           \
  } while (0)
#define C1M_T0 (void)dbg
#endif

// ------------------------------------------------------------------ k_c1_merge
struct C1Q {
  int32_t log2P, fbits, log2H, sw, hv_active, hv_op, hmax;
  int64_t size, adv, cmax, hv_i64;
  FastDiv fd;
  FastDiv32 fd32;
  uint8_t* chg;  // changelog: per-row-slot emission flags (CHG_*), or null
};

__device__ __forceinline__ bool c1q_having(const C1Q& q, uint64_t c) {
  const int64_t v = (int64_t)c;
  switch (q.hv_op) {
    case KHIP_OP_GT: return v > q.hv_i64;
    case KHIP_OP_GE: return v >= q.hv_i64;
    case KHIP_OP_LT: return v < q.hv_i64;
    case KHIP_OP_LE: return v <= q.hv_i64;
    case KHIP_OP_EQ: return v == q.hv_i64;
    case KHIP_OP_NE: return v != q.hv_i64;
  }
  return true;
}

// identity → 32-bit hash (slot = its top log2H bits; sub-pass = bits of a remix)
template <class ID>
__device__ __forceinline__ uint32_t c1_hash(ID id) {
  if constexpr (sizeof(ID) == 4) return (uint32_t)id * 0x9E3779B1u;
  else return ((uint32_t)id * 0x9E3779B1u) ^ ((uint32_t)(id >> 32) * 0x85EBCA77u);
}
__device__ __forceinline__ uint32_t c1_sub(uint32_t h, int sbits) {
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return (h >> 12) & ((1u << sbits) - 1u);
}

template <class ID>
__device__ __forceinline__ int c1_find_id(const KLDS ID* ids, ID id, uint32_t e, int H) {
  for (int probe = 0; probe < H; probe++) {
    const ID v = ids[e];
    if (v == id) return (int)e;
    if (v == (ID)~(ID)0) return -1;
    e = (e + 1) & (uint32_t)(H - 1);
  }
  return -1;
}

// Closed rows leave a partition for the closed store ONCE per push, on the first pass: every item
// of that pass moves its closed resident rows, the items that fail included (their retries read
// the same source region, which keeps the rows until the partition commits).  Later passes only
// skip closed rows: not counted, no slots, no HAVING count.
constexpr unsigned long long C1_NOSLOT = ~0ULL;
// n slots of the closed store (an item's thread 0).  The host sizes the store for every live row,
// so a reservation that ends past the capacity is a bug: it gets no slots (nothing is written)
// and the push fails (fail bit 4, C1_FATAL in need).
__device__ __forceinline__ unsigned long long c1_reserve_closed(unsigned long long* closed_n, unsigned long long n,
                                                                unsigned long long cap, uint8_t* failp,
                                                                unsigned long long* need) {
  if (!n) return 0ULL;
  const unsigned long long b = atomicAdd(closed_n, n);
  if (b + n <= cap) return b;
  *failp |= 4;
  atomicOr(need, C1_FATAL);
  return C1_NOSLOT;
}

// Segment lookup of a lane's AU records at once: record li = min(l0 + thread + u NT, rn - 1) of
// the item whose segment table is in LDS lies at at[u] = base(segment) + li, in 32-bit arithmetic
// (an item has fewer than 2^31 records, a bucket at most C1_SEGMAX x C1_CH).  An entry is
// prefix | (base - prefix) << 32 and sg2[nseg] holds the total, so a record's segment is the last
// one whose prefix is <= li.  Staged, so the LDS round trips of the AU records overlap: every
// block → segment read then one wait, every entry pair then one wait, then ONE loop in which all
// still-unresolved records step on together (uniform exit through a ballot, every read
// unconditional).  Items past C1_SEGOF << segb records search the prefixes instead, the AU
// searches in step.  rn, nseg and segb are wave-uniform; rn >= 1.
typedef uint64_t c1_sgpair __attribute__((ext_vector_type(2), aligned(8)));  // two neighbouring entries
template <int AU, int NT>
__device__ __forceinline__ void c1_seg_lookup(const KLDS uint64_t* sg2, const KLDS uint16_t* segof, uint32_t l0,
                                              uint32_t rn, int nseg, int segb, uint32_t (&at)[AU]) {
  uint32_t li[AU];
#pragma unroll
  for (int u = 0; u < AU; u++) {
    const uint32_t i = l0 + threadIdx.x + (uint32_t)(u * NT);
    li[u] = i < rn ? i : rn - 1u;
  }
  if (rn <= ((uint32_t)C1_SEGOF << segb)) {  // from the block's segment, a step or two on
    int lo[AU];
    uint32_t ba[AU];  // base - prefix of segment lo
    uint64_t sb[AU];  // entry lo + 1
#pragma unroll
    for (int u = 0; u < AU; u++) lo[u] = (int)segof[li[u] >> segb];
#pragma unroll
    for (int u = 0; u < AU; u++) {  // entries lo and lo + 1 in one read (ds_read2_b64)
      const c1_sgpair pr = *(const KLDS c1_sgpair*)(sg2 + lo[u]);
      ba[u] = (uint32_t)(pr.x >> 32);
      sb[u] = pr.y;
    }
    for (;;) {  // (sg2[nseg] = the total > li: no step leaves the table)
      bool any = false;
#pragma unroll
      for (int u = 0; u < AU; u++) any |= (uint32_t)sb[u] <= li[u];
      if (!__ballot(any)) break;
      for (int u = 0; u < AU; u++) {  // (unrolled with the loop above; a pragma here only warns)
        const bool on = (uint32_t)sb[u] <= li[u];
        lo[u] += on ? 1 : 0;
        ba[u] = on ? (uint32_t)(sb[u] >> 32) : ba[u];
        sb[u] = sg2[lo[u] + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < AU; u++) at[u] = ba[u] + li[u];
  } else {
    // the last segment whose prefix is <= li: sg2[lo] <= li < sg2[hi] holds throughout (a search
    // that has converged reads mid = lo and stays)
    uint32_t lo[AU], hi[AU];
#pragma unroll
    for (int u = 0; u < AU; u++) {
      lo[u] = 0u;
      hi[u] = (uint32_t)nseg;
    }
    for (int span = nseg; span > 1; span = (span + 1) >> 1) {  // the widest interval left: uniform
      uint32_t pm[AU];
#pragma unroll
      for (int u = 0; u < AU; u++) pm[u] = (uint32_t)sg2[(lo[u] + hi[u]) >> 1];
#pragma unroll
      for (int u = 0; u < AU; u++) {
        const uint32_t mid = (lo[u] + hi[u]) >> 1;
        const bool up = pm[u] <= li[u];
        lo[u] = up ? mid : lo[u];
        hi[u] = up ? hi[u] : mid;
      }
    }
#pragma unroll
    for (int u = 0; u < AU; u++) at[u] = (uint32_t)(sg2[lo[u]] >> 32) + li[u];
  }
}

// Work item: p (work == nullptr: item w is partition w) or work[w] = p | sbits << 16 | sub << 20
// (a retry with 2^sbits sub-passes).  LDS: ids ID[H + 64] | rt u32[H + 64] | ct u32[H + 64] |
// list u16[H] | segment entries u64[SEGMAX + 4] (prefix | (base in the bucket - prefix) << 32) |
// bucket bases and chunk starts | block → segment u16[SEGOF].
template <int NT, int AU, class ID, bool WIDE>
__global__ __launch_bounds__(NT, 4) void k_c1_merge(
    C1Q q, const uint32_t* __restrict__ work, int64_t nwork, const int64_t* __restrict__ bb,
    const int* __restrict__ cstart, const uint16_t* __restrict__ seg, const uint64_t* __restrict__ srec, int first,
    uint64_t* __restrict__ buf0, uint64_t* __restrict__ buf1, const uint8_t* __restrict__ sel,
    const int64_t* __restrict__ cnt, unsigned long long* __restrict__ newcnt, uint8_t* __restrict__ fail,
    unsigned long long* __restrict__ need, int64_t close0, uint64_t* __restrict__ closed,
    unsigned long long* __restrict__ closed_n, unsigned long long closed_cap, const int64_t* __restrict__ ci,
    unsigned long long* __restrict__ hnew,
    unsigned long long* __restrict__ hclosed, uint32_t* __restrict__ prn, const uint32_t* __restrict__ srecT,
    unsigned long long* __restrict__ dbg) {
  if (ci_ld(ci, CI_GATE) == 0) return;
  if ((ci_ld(ci, CI_WIDE) != 0) != WIDE) return;                            // the other record format's
  if (!WIDE && (ci_ld(ci, CI_ID32) != 0) != (sizeof(ID) == 4)) return;     // the other identity width's
  static_assert(!WIDE || sizeof(ID) == 8, "wide records use 64-bit identities");
  constexpr int NW = NT / 64;
  constexpr ID EMPTY = (ID)~(ID)0;
  const int log2H = q.log2H;
  const int H = 1 << log2H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  KLDS ID* ids = (KLDS ID*)(KLDS char*)smem;
  KLDS uint32_t* rt = (KLDS uint32_t*)((KLDS char*)smem + (size_t)(H + 64) * sizeof(ID));
  KLDS uint32_t* ct = rt + (H + 64);
  KLDS uint16_t* list = (KLDS uint16_t*)(ct + (H + 64));
  // segment k: prefix of the lengths | (base - prefix) << 32, so a lookup reads k and k + 1 at once
  KLDS uint64_t* sg2 = (KLDS uint64_t*)((KLDS char*)list + (((size_t)H * 2 + 15) & ~(size_t)15));
  KLDS int64_t* lbb = (KLDS int64_t*)(sg2 + C1_SEGMAX + 4);  // [B + 1] bucket bases
  KLDS int32_t* lcs = (KLDS int32_t*)(lbb + (1 << (q.log2P - q.fbits)) + 1);  // [B + 1] chunk starts
  KLDS uint16_t* segof = (KLDS uint16_t*)(lcs + (1 << (q.log2P - q.fbits)) + 2);  // [C1_SEGOF] block → segment
  __shared__ int lovf, nnew;
  __shared__ int wsum[NW], csum[NW];
  __shared__ unsigned long long lbase, cbase;
  const int F = 1 << q.fbits;
  const int64_t wbase = ci_ld(ci, CI_WBASE), whi = ci_ld(ci, CI_WHI), T0 = ci_ld(ci, CI_T0), tmin = ci_ld(ci, CI_TMIN);
  const int wbits = (int)ci_ld(ci, CI_WBITS);
  const int64_t kmin = ci_ld(ci, CI_KMINC);
  const uint64_t krange = (uint64_t)ci_ld(ci, CI_KRANGE);
  const int32_t tmin32 = (int32_t)(tmin - T0);
  const int64_t wstart = wbase * q.adv;  // the first window's start: every record ts >= it
  const bool r32 = ci_ld(ci, CI_TMAX) - wstart < ((int64_t)1 << 32);
  const uint32_t tsh32 = (uint32_t)(T0 - wstart);  // ts - wstart = (uint32) t32 + tsh32
  const bool evict = close0 != INT64_MIN;
  C1M_T0;
  const uint32_t dummy = (uint32_t)H + (uint32_t)lane;
  for (int i = threadIdx.x; i < H + 64; i += NT) {
    ids[i] = EMPTY;
    rt[i] = 0u;
    ct[i] = 0u;
  }
  if (threadIdx.x == 0) {
    lovf = 0;
    nnew = 0;
  }
  // identity of a resident row (false: no record of this push can match it) and its sub-pass hash
  auto row_id = [&](const uint64_t* row, ID* id, uint32_t* h) -> bool {
    const int64_t wi = (int64_t)fast_udiv((uint64_t)row[1], q.fd) - wbase;
    if constexpr (WIDE) {  // (key hash without its partition bits) << log2P | window
      if (wi < 0 || wi > whi) {
        *h = (uint32_t)(key_hash((int64_t)row[0]) >> 32) ^ (uint32_t)row[1];
        return false;
      }
      *id = (ID)((key_hash((int64_t)row[0]) << q.log2P) | (uint64_t)wi);
      *h = c1_hash<ID>(*id);
      return true;
    }
    const uint64_t krel = (uint64_t)((int64_t)row[0] - kmin);
    if (krel > krange || wi < 0 || wi > whi) {
      *h = (uint32_t)(key_hash((int64_t)row[0]) >> 32) ^ (uint32_t)row[1];
      return false;
    }
    if constexpr (sizeof(ID) == 4) *id = (ID)(((uint32_t)krel << wbits) | (uint32_t)wi);
    else *id = (ID)((krel << 32) | (uint64_t)wi);
    *h = c1_hash<ID>(*id);
    return true;
  };
  // item w's descriptor, and its segments in LDS (prefix of their lengths, each one's base in the
  // bucket: record li = srec[bb0 + base(s) + li - prefix(s)]).  fetch issues the global loads
  // only (the raw words stay in registers, nothing waits on them): it runs for item w + grid at
  // the start of item w, so the
  // loads are in flight through w's records.  prep (the whole workgroup, barriers inside) turns
  // them into the LDS segment table once w's records are in the table.
  struct Pre {
    uint32_t p;
    int sbits, sub;
    int64_t nrow;
    uint32_t selw;
    // seg[k0][f] | seg[k0][f + 1] << 16 and the same of k0 + 1 (the bucket's segment count and base
    // are read again by prep: nothing of them is held through the item's records)
    uint32_t s0, s1;
  };
  // the segments of partition p's bucket: their count, the first one's index, the bucket's base
  auto bucket = [&](uint32_t p, int& cs, int64_t& bb0) -> int {
    const int b = (int)(p >> q.fbits);
    cs = lcs[b];
    bb0 = lbb[b];
    const int nseg = lcs[b + 1] - cs;
    return nseg < 0 || nseg > C1_SEGMAX ? 0 : nseg;  // (k_c1_check guarantees 0 <= nseg <= SEGMAX)
  };
  struct It {
    uint32_t p;
    int sbits, sub, nseg, segb;  // segb: log2 of the records per segment-lookup block
    uint32_t rn;                 // records (< 2^31)
    uint32_t bb0;                // the bucket's first record in srec (k_c1_check: a sum of u32 totals);
                                 // the segment bases are relative to it
    int64_t nrow;
    bool isel;
  };
  auto fetch = [&](int64_t w, Pre& r) {
    uint32_t p;
    int sbits = 0, sub = 0;
    if (work) {
      const uint32_t x = work[w];
      p = x & 0xFFFFu;
      sbits = (x >> 16) & 0xF;
      sub = (int)(x >> 20);
    } else {
      p = (uint32_t)w;
    }
    p = __builtin_amdgcn_readfirstlane(p);
    const int f = (int)(p & (uint32_t)(F - 1));
    int cs;
    int64_t bb0;
    const int nseg = bucket(p, cs, bb0);
    r.p = p;
    r.sbits = sbits;
    r.sub = sub;
    r.nrow = cnt[p];
    r.selw = ((const uint32_t*)sel)[p >> 2];
    const int k0 = threadIdx.x * 2;
    r.s0 = r.s1 = 0u;
    if (k0 < nseg) {
      const uint16_t* sg = seg + (int64_t)(cs + k0) * (F + 1) + f;
      r.s0 = (uint32_t)sg[0] | (uint32_t)sg[1] << 16;
    }
    if (k0 + 1 < nseg) {
      const uint16_t* sg = seg + (int64_t)(cs + k0 + 1) * (F + 1) + f;
      r.s1 = (uint32_t)sg[0] | (uint32_t)sg[1] << 16;
    }
  };
  auto prep = [&](const Pre& r, It& it) {
    int cs;
    int64_t bb0;
    const int nseg = bucket(r.p, cs, bb0);
    it.p = r.p;
    it.sbits = r.sbits;
    it.sub = r.sub;
    it.nrow = r.nrow;
    it.isel = ((r.selw >> (8 * (r.p & 3))) & 0xFFu) != 0;
    const int k0 = threadIdx.x * 2;
    const uint32_t s00 = r.s0 & 0xFFFFu, s10 = r.s1 & 0xFFFFu;
    const int len0 = k0 < nseg ? (int)(r.s0 >> 16) - (int)s00 : 0;
    const int len1 = k0 + 1 < nseg ? (int)(r.s1 >> 16) - (int)s10 : 0;
    const uint32_t base0 = (uint32_t)(k0 * C1_CH) + s00;  // relative to the bucket's first record
    const uint32_t base1 = (uint32_t)((k0 + 1) * C1_CH) + s10;
    const int s = len0 + len1;
    int incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    lds_barrier();
    int before = 0;
    int tot = 0;
    for (int k = 0; k < NW; k++) {
      before += k < wave ? wsum[k] : 0;
      tot += wsum[k];
    }
    const int ex = before + incl - s;
    // the finest lookup block that covers the item in C1_SEGOF entries (segments hold C1_CH / F
    // records on average: 32-record blocks make the lookup a read and at most a step or two)
    const int segb = tot <= (C1_SEGOF << 5) ? 5 : (tot <= (C1_SEGOF << 6) ? 6 : C1_SEGB);
    const int bm = (1 << segb) - 1;
    if (k0 < nseg) sg2[k0] = (uint32_t)ex | (uint64_t)(base0 - (uint32_t)ex) << 32;
    if (k0 + 1 < nseg) sg2[k0 + 1] = (uint32_t)(ex + len0) | (uint64_t)(base1 - (uint32_t)(ex + len0)) << 32;
    // segment lookup: block j (records [j << segb, (j + 1) << segb)) starts in segment segof[j]
    for (int bj = (ex + bm) >> segb, be = (ex + len0 + bm) >> segb; bj < be && bj < C1_SEGOF; bj++)
      segof[bj] = (uint16_t)k0;
    for (int bj = (ex + len0 + bm) >> segb, be = (ex + s + bm) >> segb; bj < be && bj < C1_SEGOF; bj++)
      segof[bj] = (uint16_t)(k0 + 1);
    if (k0 < nseg && k0 + 2 >= nseg) sg2[nseg] = (uint32_t)(ex + s);  // the total
    if (nseg == 0 && threadIdx.x == 0) sg2[0] = 0u;
    lds_barrier();
    // (the same in every lane: held in scalar registers, so the record loop's control flow is
    // uniform and the bucket's base is a scalar address)
    it.rn = __builtin_amdgcn_readfirstlane((uint32_t)sg2[nseg]);
    it.segb = __builtin_amdgcn_readfirstlane(segb);
    it.nseg = __builtin_amdgcn_readfirstlane(nseg);
    it.bb0 = __builtin_amdgcn_readfirstlane((uint32_t)bb0);
  };
  uint64_t ra[AU], rb[AU];
  uint32_t ta[AU], tb[AU];  // WIDE: the records' ts words
  // records li = l0 + thread + u NT of the item whose segments are in LDS (indices clamped to the
  // last record: every load is unconditional, so the waits stay counted).  A record's address is
  // the bucket's base (uniform) plus a 32-bit byte offset.
  auto load = [&](uint64_t (&x)[AU], uint32_t (&tx)[AU], uint32_t l0, const It& t) {
    uint32_t at[AU];
    c1_seg_lookup<AU, NT>(sg2, segof, l0, t.rn, t.nseg, t.segb, at);
    const char* sb = (const char*)(srec + t.bb0);
#pragma unroll
    for (int u = 0; u < AU; u++) x[u] = c1_ld((const uint64_t*)(sb + (uint64_t)(uint32_t)(at[u] << 3)));
    if constexpr (WIDE) {
      const char* sbT = (const char*)(srecT + t.bb0);
#pragma unroll
      for (int u = 0; u < AU; u++) tx[u] = c1_ld((const uint32_t*)(sbT + (uint64_t)(uint32_t)(at[u] << 2)));
    }
  };
  // the item's first two chunks (register sets A and B): a chunk is always two chunks ahead of
  // the one being applied
  auto load01 = [&](const It& x) {
    if (x.rn > 0) load(ra, ta, 0u, x);
    if (x.rn > (uint32_t)(AU * NT)) load(rb, tb, (uint32_t)(AU * NT), x);
  };
  // the bucket table (chunk starts, bucket bases) in LDS for every descriptor
  for (int k = threadIdx.x; k <= (1 << (q.log2P - q.fbits)); k += NT) {
    lcs[k] = cstart[k];
    lbb[k] = bb[k];
  }
  lds_barrier();
  // the first item, and its first chunks in flight; each item prepares the next one (segments and
  // first chunks) as soon as its own records are in the table, so those loads overlap its
  // resident-row, count and write-out phases
  Pre pr{};
  It nx{};
  if (blockIdx.x < nwork) {
    fetch(blockIdx.x, pr);
    prep(pr, nx);
    load01(nx);
  }
  for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const It it = nx;
    const uint32_t p = it.p;
    const int sbits = it.sbits, sub = it.sub;
    const uint32_t rn = it.rn;
    const int64_t nrow = it.nrow;
    const bool isel = it.isel;
    const int64_t wn = w + gridDim.x;
    if (wn < nwork) fetch(wn, pr);
    if (first && threadIdx.x == 0) prn[p] = rn;
    if (rn == 0 && first) {  // untouched partition: nothing to rewrite
      if (wn < nwork) {
        prep(pr, nx);
        load01(nx);
      }
      continue;
    }
    const uint64_t* src = (isel ? buf1 : buf0) + (uint64_t)p * q.cmax * q.sw;
    // (closed resident rows leave for the closed store in the write-out, phase 4: one pass over the
    // resident rows there, the closed store's slots reserved with the region's)
    // An item that fails on the first pass moves them here instead (count, reserve, copy), since
    // its retries skip them.
    auto evict_failed = [&]() {
      if (!first || !evict || nrow == 0) return;  // (uniform)
      auto mine_closed = [&](const uint64_t* row) -> bool {
        if ((int64_t)row[1] + q.size > close0) return false;
        if (!sbits) return true;
        ID id;
        uint32_t h;
        row_id(row, &id, &h);
        return (int)c1_sub(h, sbits) == sub;
      };
      int n_cl = 0;
      for (int64_t r = threadIdx.x; r < nrow; r += NT) n_cl += mine_closed(src + r * q.sw) ? 1 : 0;
      const int wave_cl = (int)wave_sum(n_cl);
      if (lane == 0) csum[wave] = wave_cl;
      lds_barrier();
      int cl_before = 0, cl_total = 0;
      for (int k = 0; k < NW; k++) {
        if (k < wave) cl_before += csum[k];
        cl_total += csum[k];
      }
      if (threadIdx.x == 0)
        cbase = c1_reserve_closed(closed_n, (unsigned long long)cl_total, closed_cap, &fail[p], need);
      lds_barrier();
      const unsigned long long cb = cbase;
      if (cl_total == 0 || cb == C1_NOSLOT) return;
      uint64_t ccur = cb + (uint64_t)cl_before;
      const uint64_t lt = (1ULL << lane) - 1;
      int nhc = 0;
      for (int64_t r0 = wave * 64; r0 < nrow; r0 += NT) {
        const int64_t r = r0 + lane;
        const uint64_t* row = src + (r < nrow ? r : 0) * q.sw;
        const bool cl = r < nrow && mine_closed(row);
        const uint64_t bc = __ballot(cl);
        if (cl) {
          uint64_t* cd = closed + (ccur + __popcll(bc & lt)) * q.sw;
          for (int k = 0; k < q.sw; k++) cd[k] = row[k];
          nhc += q.hv_active && c1q_having(q, row[3]) ? 1 : 0;
        }
        ccur += __popcll(bc);
      }
      if (q.hv_active) {
        nhc = (int)wave_sum(nhc);
        if (lane == 0 && nhc) atomicAdd(hclosed, (unsigned long long)nhc);
      }
    };
    C1M_T(0);
    // 1. records → delta entries, two register sets (chunk c + 1 in flight while c is applied;
    //    chunk 0 was loaded with the item's segments)
    // R32: the push's record times relative to the first window's start fit 32 bits (a 32-bit
    // window division instead of the 64-bit one)
    // The record set's next chunk is loaded into the same registers right after its identities'
    // CASes are issued (prefetch): the chunk's segment lookups and the table-full flag then return
    // with the CASes (LDS returns in order), not behind this chunk's plane atomics, and the loads
    // have a whole chunk to land.  Returns false when the table is (about to be) full.
    auto apply = [&](const uint64_t (&xr)[AU], const uint32_t (&txr)[AU], uint32_t l0, auto R32, auto NUc,
                     auto&& prefetch) -> bool {
      constexpr int NU = decltype(NUc)::value;  // live slot rows: AU, or a last chunk's 1 or 2
      ID id[NU];
      uint32_t e[NU], tr[NU];
      bool pend[NU], claimed[NU];
#pragma unroll
      for (int u = 0; u < NU; u++) {
        const uint32_t li = l0 + threadIdx.x + (uint32_t)(u * NT);
        const uint64_t v = xr[u];
        const int32_t t32 = WIDE ? (int32_t)txr[u] : (int32_t)(uint32_t)v;
        const uint64_t krel = v >> 32;
        uint64_t wi;
        if constexpr (decltype(R32)::value) wi = fast_udiv32((uint32_t)t32 + tsh32, q.fd32);
        else wi = fast_udiv((uint64_t)(T0 + (int64_t)t32), q.fd) - (uint64_t)wbase;
        ID x;
        if constexpr (WIDE) x = (ID)((v << q.log2P) | wi);  // v = the key hash
        else if constexpr (sizeof(ID) == 4) x = (ID)(((uint32_t)krel << wbits) | (uint32_t)wi);
        else x = (ID)((krel << 32) | wi);
        const uint32_t h = c1_hash<ID>(x);
        bool act = li < rn;
        if (sbits) act = act && (int)c1_sub(h, sbits) == sub;
        id[u] = act ? x : EMPTY;
        e[u] = act ? h >> (32 - log2H) : dummy;
        tr[u] = (uint32_t)(t32 - tmin32) + 1u;
      }
      ID old[NU];
#pragma unroll
      for (int u = 0; u < NU; u++) {
        old[u] = EMPTY;
        __hip_atomic_compare_exchange_strong(&ids[e[u]], &old[u], id[u], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      const int fullv = *(volatile KLDS int*)&lovf;
      prefetch();
      const int full = __builtin_amdgcn_readfirstlane(fullv);  // (one LDS word: the same in every lane)
#pragma unroll
      for (int u = 0; u < NU; u++) {
        claimed[u] = id[u] != EMPTY && old[u] == EMPTY;
        pend[u] = old[u] != EMPTY && old[u] != id[u];
      }
      for (int probes = 1;; probes++) {  // collisions: every pending record probes on together
        bool anyp = false;
#pragma unroll
        for (int u = 0; u < NU; u++) anyp |= pend[u];
        if (!__ballot(anyp)) break;
        if (probes >= H) {
          lovf = 1;
#pragma unroll
          for (int u = 0; u < NU; u++)
            if (pend[u]) id[u] = EMPTY;
          break;
        }
#pragma unroll
        for (int u = 0; u < NU; u++) {
          if (!pend[u]) continue;
          e[u] = (e[u] + 1) & (uint32_t)(H - 1);
          ID o2 = EMPTY;
          __hip_atomic_compare_exchange_strong(&ids[e[u]], &o2, id[u], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
          claimed[u] = o2 == EMPTY;
          pend[u] = o2 != EMPTY && o2 != id[u];
        }
      }
      int nnow;
      {
        bool cl[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) cl[u] = claimed[u] && id[u] != EMPTY;
        nnow = mg_list_append_n<NU>(cl, e, list, &nnew);
      }
#pragma unroll
      for (int u = 0; u < NU; u++) {
        if (id[u] == EMPTY) continue;
        __hip_atomic_fetch_max(&rt[e[u]], tr[u], WG_RLX);
        __hip_atomic_fetch_add(&ct[e[u]], 1u, WG_RLX);
      }
      return !full && nnow <= q.hmax;
    };
    constexpr uint32_t CR = (uint32_t)(AU * NT);  // records per chunk
    const uint32_t nch = (rn + CR - 1u) / CR;
    // The last chunk has nu = ceil((rn - l0) / NT) live slot rows (records u NT + thread of the
    // chunk, nu uniform like rn).  With nu = 1 or 2 it is applied after the loop by a variant that
    // issues nothing for the rows u >= nu: no identity, CAS, probe, append or plane atomic.  (Its
    // prefetch stays the full load, dead rows clamped to the last record: sized loads were
    // measured and cost more than they saved, profiles/c1_merge_tail.)  nu >= 3 takes the full code.
    constexpr int TAILNU = AU - 1 < 2 ? AU - 1 : 2;  // the largest nu with a variant of its own
    const uint32_t tail_r = rn - (nch - 1u) * CR;    // (rn > 0) records of the last chunk
    const uint32_t tnu =
        rn > 0 && tail_r <= (uint32_t)(TAILNU * NT) ? (tail_r + (uint32_t)(NT - 1)) / (uint32_t)NT : (uint32_t)AU;
    const uint32_t nfc = tnu < (uint32_t)AU ? nch - 1u : nch;
    using FullNU = std::integral_constant<int, AU>;
    if (rn > 0) {  // chunks 0 and 1 are in flight (load01); each set is reloaded as it is applied
      bool go = true;
      for (uint32_t c = 0; c < nfc; c += 2) {
        auto pa = [&] { if (c + 2 < nch) load(ra, ta, (c + 2) * CR, it); };
        const bool ga = r32 ? apply(ra, ta, c * CR, std::true_type{}, FullNU{}, pa)
                            : apply(ra, ta, c * CR, std::false_type{}, FullNU{}, pa);
        if (!ga) go = false;
        if (!ga || c + 1 >= nfc) break;
        auto pb = [&] { if (c + 3 < nch) load(rb, tb, (c + 3) * CR, it); };
        const bool gb = r32 ? apply(rb, tb, (c + 1) * CR, std::true_type{}, FullNU{}, pb)
                            : apply(rb, tb, (c + 1) * CR, std::false_type{}, FullNU{}, pb);
        if (!gb) {
          go = false;
          break;
        }
      }
      if (go && nfc < nch) {  // the short last chunk, from the set that holds it
        auto tail = [&](const uint64_t (&xr)[AU], const uint32_t (&txr)[AU], auto NUc) {
          auto none = [] {};
          if (r32) apply(xr, txr, nfc * CR, std::true_type{}, NUc, none);
          else apply(xr, txr, nfc * CR, std::false_type{}, NUc, none);
        };
        using N1 = std::integral_constant<int, 1>;
        using N2 = std::integral_constant<int, TAILNU>;
        if (nfc & 1u) {
          if (tnu == 1u) tail(rb, tb, N1{});
          else tail(rb, tb, N2{});
        } else {
          if (tnu == 1u) tail(ra, ta, N1{});
          else tail(ra, ta, N2{});
        }
      }
    }
    lds_barrier();
    // the item's records are in the table (its segments are no longer read).  Every thread takes
    // the list's length and the overflow flag now: the barriers of the next item's prep then
    // separate these reads from thread 0's reset, and the item's closing barrier the reset from
    // the next item's appends.  (The workgroup's last item resets nothing: nothing reads it.)
    const int nnew_r = __builtin_amdgcn_readfirstlane(nnew);
    const int lovf_r = __builtin_amdgcn_readfirstlane(lovf);
    // the next item's segments and first chunks
    if (wn < nwork) {
      prep(pr, nx);
      if (threadIdx.x == 0) {
        lovf = 0;
        nnew = 0;
      }
      load01(nx);
    }
    C1M_T(1);
    const int nl = nnew_r < H ? nnew_r : H;
    if (lovf_r || nnew_r > q.hmax) {  // more groups than the table takes: retried with 2x sub-passes
      if (threadIdx.x == 0) fail[p] |= 1;
      for (int i = threadIdx.x; i < nl; i += NT) {
        const uint32_t e = list[i];
        ids[e] = EMPTY;
        rt[e] = 0u;
        ct[e] = 0u;
      }
      evict_failed();
      lds_barrier();  // the table is clear for the next item
      continue;
    }
    // 2. resident rows: mark the delta entries they absorb; count live and closed rows
    int n_mine = 0, n_cl = 0;
    for (int64_t r = threadIdx.x; r < nrow; r += NT) {
      const uint64_t* row = src + r * q.sw;
      ID id;
      uint32_t h;
      const bool has = row_id(row, &id, &h);
      if (sbits && (int)c1_sub(h, sbits) != sub) continue;
      if (evict && (int64_t)row[1] + q.size <= close0) {
        n_cl += first ? 1 : 0;  // (a later pass: the first one moved it)
        continue;
      }
      if (has) {
        const int e = c1_find_id<ID>(ids, id, h >> (32 - log2H), H);
        if (e >= 0) rt[e] |= RT_MATCHED;  // one resident row per identity: a plain store
      }
      n_mine++;
    }
    if (nrow > 0) lds_barrier();  // the marks before the list walk reads them (uniform: nrow is the item's)
    // the wave's share of the list: new (unmatched) entries
    const int per = ((nl + NW - 1) / NW + 63) & ~63;
    const int lb0 = wave * per, lb1 = lb0 + per < nl ? lb0 + per : nl;
    // 3. per-wave row counts → the partition's region range (one atomic per work item), and the
    //    closed store's slots for its closed rows
    int wave_before = 0, total = 0, cl_before = 0, cl_total = 0;
    unsigned long long lb, cb;  // the item's base in the region and in the closed store
    if (nrow == 0) {
      // no resident rows (uniform): nothing is matched, so every listed entry is a new row and the
      // counts are known without walking the list: the wave's rows are its share, the waves
      // before it hold min(lb0, nl), no row is closed (no closed-store slots)
      total = nl;
      wave_before = lb0 < nl ? lb0 : nl;
      cb = 0ULL;
      if (work) {  // a retry's sub-passes share the region: thread 0 reserves, everyone reads
        if (threadIdx.x == 0) lbase = total ? atomicAdd(&newcnt[p], (unsigned long long)total) : 0ULL;
        lds_barrier();
        lb = lbase;
      } else {
        lb = 0ULL;
        if (threadIdx.x == 0) newcnt[p] = (unsigned long long)total;
      }
    } else {
      int nnw = 0;
      for (int k = lb0; k < lb1; k += 64) {
        const int i = k + lane;
        const uint32_t e = i < lb1 ? list[i] : dummy;
        const bool isnew = i < lb1 && !(rt[e] & RT_MATCHED);
        nnw += (int)__popcll(__ballot(isnew));
      }
      const int wave_rows = (int)wave_sum(n_mine) + nnw;
      const int wave_cl = (int)wave_sum(n_cl);
      if (lane == 0) {
        wsum[wave] = wave_rows;
        csum[wave] = wave_cl;
      }
      lds_barrier();
      for (int k = 0; k < NW; k++) {
        if (k < wave) wave_before += wsum[k], cl_before += csum[k];
        total += wsum[k];
        cl_total += csum[k];
      }
      if (threadIdx.x == 0) {
        if (work) lbase = total ? atomicAdd(&newcnt[p], (unsigned long long)total) : 0ULL;
        else {
          lbase = 0;
          newcnt[p] = (unsigned long long)total;
        }
        // (an item that does not fit its region reserves with its own copy, evict_failed)
        cbase = (int64_t)(lbase + total) <= q.cmax
                    ? c1_reserve_closed(closed_n, (unsigned long long)cl_total, closed_cap, &fail[p], need)
                    : 0ULL;
      }
      lds_barrier();
      lb = lbase;
      cb = cbase;
    }
    if ((int64_t)(lb + total) > q.cmax) {
      if (threadIdx.x == 0) {
        fail[p] |= 2;
        atomicMax(need, (unsigned long long)(lb + total));
      }
      for (int i = threadIdx.x; i < nl; i += NT) {
        const uint32_t e = list[i];
        ids[e] = EMPTY;
        rt[e] = 0u;
        ct[e] = 0u;
      }
      evict_failed();
      lds_barrier();  // the table is clear for the next item
      continue;
    }
    C1M_T(3);
    // 4. write: resident rows (merged), then the wave's new entries (ballot ranks: consecutive rows)
    uint64_t* dst0 = (isel ? buf0 : buf1) + (uint64_t)p * q.cmax * q.sw;
    uint64_t cur = lb + (uint64_t)wave_before;
    uint64_t ccur = cb + (uint64_t)cl_before;
    const bool cmove = first && cb != C1_NOSLOT;  // closed rows are copied (else only dropped)
    const uint64_t lt = (1ULL << lane) - 1;
    int nh = 0, nhc = 0;
    for (int64_t r0 = wave * 64; r0 < nrow; r0 += NT) {
      const int64_t r = r0 + lane;
      const uint64_t* row = src + (r < nrow ? r : 0) * q.sw;
      bool live = r < nrow, cl = false;
      int e = -1;
      if (live) {
        ID id;
        uint32_t h;
        const bool has = row_id(row, &id, &h);
        if (sbits) live = (int)c1_sub(h, sbits) == sub;
        cl = live && evict && (int64_t)row[1] + q.size <= close0;
        live = live && !cl;
        if (live && has) e = c1_find_id<ID>(ids, id, h >> (32 - log2H), H);
      }
      const uint64_t bc = __ballot(cl);
      if (cl && cmove) {
        uint64_t* cd = closed + (ccur + __popcll(bc & lt)) * q.sw;
        for (int k = 0; k < q.sw; k++) cd[k] = row[k];
        nhc += q.hv_active && c1q_having(q, row[3]) ? 1 : 0;
      }
      ccur += __popcll(bc);
      const uint64_t bl = __ballot(live);
      if (live) {
        const uint64_t ri = cur + __popcll(bl & lt);
        uint64_t* dst = dst0 + ri * q.sw;
        uint64_t w2 = row[2], c = row[3];
        if (e >= 0) {
          const int64_t t = tmin + (int64_t)(rt[e] & ~RT_MATCHED) - 1;
          w2 = t > (int64_t)w2 ? (uint64_t)t : w2;
          c += ct[e];
        }
        *(longlong2*)dst = make_longlong2((int64_t)row[0], (int64_t)row[1]);
        *(longlong2*)(dst + 2) = make_longlong2((int64_t)w2, (int64_t)c);
        const bool now = !q.hv_active || c1q_having(q, c);
        nh += q.hv_active && now ? 1 : 0;
        if (q.chg)
          q.chg[(uint64_t)p * q.cmax + ri] =
              e >= 0 ? (uint8_t)(CHG_TOUCHED | (!q.hv_active || c1q_having(q, row[3]) ? CHG_OLD : 0) | (now ? CHG_NEW : 0))
                     : (uint8_t)0;
      }
      cur += __popcll(bl);
    }
    if (nrow > 0) lds_barrier();  // every wave's resident rows have read their entries: the list walk clears them
    const uint32_t wmask = wbits ? (1u << wbits) - 1u : 0u;
    for (int k = lb0; k < lb1; k += 64) {
      const int i = k + lane;
      const uint32_t e = i < lb1 ? list[i] : dummy;
      const uint32_t rv = rt[e];
      const bool used = i < lb1;
      const bool isnew = used && !(rv & RT_MATCHED);
      const uint64_t bl = __ballot(isnew);
      if (isnew) {
        const uint64_t ri = cur + __popcll(bl & lt);
        uint64_t* dst = dst0 + ri * q.sw;
        const ID id = ids[e];
        int64_t key, wi;
        if constexpr (WIDE) {  // the partition's bits above the identity's key-hash bits
          wi = (int64_t)((uint64_t)id & (((uint64_t)1 << q.log2P) - 1));
          key = key_of_hash(((uint64_t)p << (64 - q.log2P)) | ((uint64_t)id >> q.log2P));
        } else if constexpr (sizeof(ID) == 4) {
          key = kmin + (int64_t)((uint32_t)id >> wbits);
          wi = (int64_t)((uint32_t)id & wmask);
        } else {
          key = kmin + (int64_t)((uint64_t)id >> 32);
          wi = (int64_t)((uint64_t)id & 0xFFFFFFFFull);
        }
        const uint32_t c = ct[e];
        *(longlong2*)dst = make_longlong2(key, (wbase + wi) * q.adv);
        *(longlong2*)(dst + 2) = make_longlong2(tmin + (int64_t)rv - 1, (int64_t)c);
        const bool now = !q.hv_active || c1q_having(q, c);
        nh += q.hv_active && now ? 1 : 0;
        if (q.chg) q.chg[(uint64_t)p * q.cmax + ri] = (uint8_t)(CHG_TOUCHED | (now ? CHG_NEW : 0));
      }
      if (used) {  // every listed (used) entry leaves cleared for the next item
        ids[e] = EMPTY;
        rt[e] = 0u;
        ct[e] = 0u;
      }
      cur += __popcll(bl);
    }
    if (q.hv_active) {
      nh = (int)wave_sum(nh);
      nhc = (int)wave_sum(nhc);
      if (lane == 0 && nh) atomicAdd(&hnew[p], (unsigned long long)nh);
      if (lane == 0 && nhc) atomicAdd(hclosed, (unsigned long long)nhc);
    }
    lds_barrier();  // the table is clear for the next item (its list length was reset after prep)
    C1M_T(4);
  }
}

// ------------------------------------------------------------------ value records (c1v)
// The same pipeline for a query whose aggregates all read ONE argument column (COUNT(col), SUM,
// AVG, MIN, MAX, with or without COUNT(*)): records are 16 bytes, {(key - kmin) << 32 |
// (uint32)(ts - T0), bit 63 = the argument is not NULL; the argument's bits (INT sign-extended,
// BIGINT, DOUBLE raw)}, so the key range must fit 31 bits.  HOPPING windows whose size is a
// multiple of the advance go through panes: a record updates ONE entry, its pane (key, ts /
// advance), and after the records every pane is folded into its F windows — F updates per pane,
// not per record.  TUMBLING is the F = 1 case (the pane is the window).
constexpr int C1V_CH = 4096;  // refine chunk of 16-byte records (64 KB of LDS stage)
constexpr int C1V_MAXW = 8;   // row words (key, ws, rowtime + at most 5 state words)

typedef uint64_t c1v_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ulonglong2 ld_nt2(const ulonglong2* p) {  // 16-byte load (c1_ld)
  const c1v_u2 v = c1_ld((const c1v_u2*)p);
  return make_ulonglong2(v.x, v.y);
}

struct C1VCol {
  const void* data;
  const uint8_t* valid;
  int32_t type;
};


// Records of tile t → step runs, as k_c1_scatter, 16 bytes each (key - kb in 31 bits, the
// argument's non-null flag in bit 63).  HOP: the windows
// applied per accepted record (windowsFor's count) for the batch statistics.
template <int U, int NT, bool ST, bool ROWS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_c1v_scatter(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ ts, const uint8_t* __restrict__ kv,
    const uint8_t* __restrict__ rv, C1VCol vc, RowsIn ri, int64_t n, int64_t nT, int log2B, uint16_t* __restrict__ rloc,
    uint16_t* __restrict__ roff, uint32_t* __restrict__ ttot, ulonglong2* __restrict__ srec, int64_t* __restrict__ tilestat,
    int64_t* __restrict__ tpart, int64_t* __restrict__ ci, const int64_t* __restrict__ st_at, int64_t size, int64_t adv,
    FastDiv fd, int hop, int64_t grace, const int64_t* __restrict__ stream_time, int64_t kb_in, int has_kb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int wsum[NT / 64];
  __shared__ unsigned long long lc[5];
  __shared__ int lt[2][2];
  __shared__ int lfail, lkfail;
  __shared__ uint32_t lkr[2];  // min / max of the staged key offsets
  constexpr int S = U * NT;
  constexpr int SPT = C1_TILE / S;
  const int B = 1 << log2B;
  const int64_t t = tile_of(blockIdx.x, nT);
  uint32_t* cnt = (uint32_t*)smem;
  uint32_t* sbase = cnt + B;
  ulonglong2* sp = (ulonglong2*)(smem + (size_t)B * 8);  // B >= 32: 16-byte aligned
  uint32_t* lrc = (uint32_t*)(smem + run_stage_lds(B, S, 16, false));
  uint16_t* lro = (uint16_t*)(lrc + SPT * B);
  for (int b = threadIdx.x; b < B; b += NT) cnt[b] = 0u;
  if (threadIdx.x < 5) lc[threadIdx.x] = 0;
  if (threadIdx.x < 2) {
    lt[threadIdx.x][0] = INT32_MIN;
    lt[threadIdx.x][1] = INT32_MAX;
  }
  if (threadIdx.x == 0) {
    lfail = lkfail = 0;
    lkr[0] = 0xFFFFFFFFu;
    lkr[1] = 0u;
  }
  int64_t T0, kb;
  if constexpr (ROWS) run_bases((const int64_t*)ri.rows, (const int64_t*)ri.rows + 1, n, stream_time, kb_in, has_kb, 31, ci, &T0, &kb);
  else run_bases(keys, ts, n, stream_time, kb_in, has_kb, 31, ci, &T0, &kb);
  const int shift = log2B == 0 ? 64 : 64 - log2B;
  const uint32_t bmask = (uint32_t)(B - 1);
  const int64_t base = t * C1_TILE;
  const int64_t end = base + C1_TILE < n ? base + C1_TILE : n;
  int c_acc = 0, c_nk = 0, c_nr = 0, c_bt = 0, c_app = 0;
  uint32_t kor = 0u;
  int64_t x[U], k[U], v[U];
  uint32_t vm[ROWS ? U : 1];  // ROWS: the rows' validity words (low half)
  int64_t rst[ROWS && ST ? U : 1];  // ROWS && ST: the rows' stream-time words (KHIP_SHUFFLE_STREAM_TIME)
  auto load_step = [&](int64_t i0) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      int64_t i = i0 + (int64_t)u * NT;
      i = i < end ? i : end - 1;
      if constexpr (ROWS) {
        const uint64_t* r = ri.rows + i * (int64_t)ri.rw;
        if (ri.rw == 4 && ri.vword == 2) {  // [key, ts, argument, validity]: two 16-byte loads
          const ulonglong2 a = ((const ulonglong2*)r)[0], b = ((const ulonglong2*)r)[1];
          k[u] = (int64_t)a.x;
          x[u] = (int64_t)a.y;
          v[u] = (int64_t)b.x;
          vm[u] = (uint32_t)b.y;
        } else {
          k[u] = (int64_t)r[0];
          x[u] = (int64_t)r[1];
          v[u] = (int64_t)r[ri.vword];
          vm[u] = (uint32_t)r[ri.rw - 1];
        }
        if constexpr (ST) rst[u] = (int64_t)r[ri.rw - 2];
      } else {
        x[u] = ts[i];
        k[u] = keys[i];
        v[u] = vc.type == KHIP_TYPE_INT32 ? (int64_t)((const int32_t*)vc.data)[i] : ((const int64_t*)vc.data)[i];
      }
    }
  };
  int64_t t_rmax = -1, t_min = INT64_MAX, t_bound = INT64_MAX;  // the tile's summary (k_c1_scatter)
  bool t_ok = true;
  auto publish = [&](int64_t, int st) {
    const int mx = lt[st & 1][0], mn = lt[st & 1][1];
    if (mx != INT32_MIN) {
      const int64_t smx = T0 + mx, smn = T0 + mn;
      t_rmax = smx > t_rmax ? smx : t_rmax;
      t_min = smn < t_min ? smn : t_min;
      const int64_t fw = first_window_start_fd(smn, size, adv, fd) + size;
      const int64_t b = grace > ((int64_t)1 << 61) ? INT64_MAX : fw + grace - 1;
      t_bound = b < t_bound ? b : t_bound;
      t_ok = t_ok && t_rmax <= b;
    }
    lt[st & 1][0] = INT32_MIN;
    lt[st & 1][1] = INT32_MAX;
  };
  lds_barrier();
  int64_t s0 = base;
  int st_last = -1;
  if (s0 < end) load_step(s0 + threadIdx.x);
  for (int st = 0; s0 < end; s0 += S, st++) {
    st_last = st;
    const int64_t i0 = s0 + threadIdx.x;
    bool ok[U];
    uint32_t bin[U];
    ulonglong2 rec[U];
    int tmx = INT32_MIN, tmn = INT32_MAX;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = i0 + (int64_t)u * NT;
      ok[u] = i < end;
      const int64_t ii = ok[u] ? i : base;
      const bool kok = ROWS || bit_get(kv, ii), rok = ROWS || bit_get(rv, ii);
      const bool vok = ROWS ? ((vm[ROWS ? u : 0] >> ri.vbit) & 1u) != 0 : bit_get(vc.valid, ii);
      const bool valid = ok[u] && kok && rok && x[u] >= 0;
      c_nk += ok[u] && !kok;
      c_nr += ok[u] && kok && !rok;
      c_bt += ok[u] && kok && rok && x[u] < 0;
      c_acc += valid;
      const int64_t d = x[u] - T0;
      if (valid && (d <= (int64_t)INT32_MIN || d > (int64_t)INT32_MAX)) {  // rare: an LDS flag, not a loop-carried mask
        lfail = 1;
#ifdef KHIP_TUNING
        if (ci[CI_N - 1] == 1 && (threadIdx.x & 63) == 0) printf("[c1 scatter] t %ld i %ld x %ld T0 %ld\n", (long)t, (long)i, (long)x[u], (long)T0);
#endif
      }
      if constexpr (ST) {
        const int64_t ds = (ROWS ? rst[ROWS ? u : 0] : st_at[ii]) - T0;
        if (valid && (ds <= (int64_t)INT32_MIN || ds > (int64_t)INT32_MAX)) lfail = 1;
        tmx = valid && (int)ds > tmx ? (int)ds : tmx;
      } else {
        tmx = valid && (int)d > tmx ? (int)d : tmx;
      }
      tmn = valid && (int)d < tmn ? (int)d : tmn;
      if (hop && valid) {  // windowsFor: starts in (ts - size, ts], multiples of adv, >= 0
        const int64_t lo = x[u] - size + adv;
        c_app += (int)((int64_t)fast_udiv((uint64_t)x[u], fd) - (int64_t)fast_udiv((uint64_t)(lo > 0 ? lo : 0), fd) + 1);
      }
      bin[u] = stage_bin(key_hash(k[u]), shift, bmask);
      const uint64_t kd = (uint64_t)k[u] - (uint64_t)kb;
      kor |= ok[u] ? (uint32_t)(kd >> 31) : 0u;  // nonzero: a key outside the 31-bit field above kb
      const uint64_t w0 = ((kd & 0x7FFFFFFFull) << 32) | (uint64_t)(valid ? (uint32_t)d : C1_SENT);
      rec[u] = make_ulonglong2(w0 | (vok ? (1ULL << 63) : 0ULL), (uint64_t)v[u]);
    }
    if (s0 + S < end) load_step(i0 + S);
    uint32_t t32u[U];  // (no ts words: 16-byte records carry the ts)
    const uint32_t tot = stage_step_runs<U, NT, ulonglong2, false>(rec, t32u, bin, ok, B, cnt, sbase, wsum, sp, nullptr,
                                                                   srec, nullptr, t * SPT + st, lrc + st * B,
                                                                   lro + st * B);
    step_krange<NT, ulonglong2>(sp, tot, 0x7FFFFFFFu, lkr);
    for (int off = 32; off > 0; off >>= 1) {
      const int a = __shfl_xor(tmx, off, 64), b = __shfl_xor(tmn, off, 64);
      tmx = a > tmx ? a : tmx;
      tmn = b < tmn ? b : tmn;
    }
    if ((threadIdx.x & 63) == 0 && tmx != INT32_MIN) {
      atomicMax(&lt[st & 1][0], tmx);
      atomicMin(&lt[st & 1][1], tmn);
    }
    if (threadIdx.x == 0 && st > 0) publish(s0 - S, st - 1);
  }
  flush_run_counts<SPT, NT>(lrc, lro, B, st_last, t, nT, rloc, roff, ttot);
  if (kor) lkfail = 1;
  __syncthreads();
  if (threadIdx.x == 0 && s0 > base) publish(s0 - S, st_last);
  if (threadIdx.x == 0) run_krange(lkr, lkfail, kb, ci);
  c_acc = wave_sum(c_acc);
  c_nk = wave_sum(c_nk);
  c_nr = wave_sum(c_nr);
  c_bt = wave_sum(c_bt);
  c_app = wave_sum(c_app);
  if ((threadIdx.x & 63) == 0) {
    if (c_acc) atomicAdd(&lc[0], (unsigned long long)c_acc);
    if (c_nk) atomicAdd(&lc[1], (unsigned long long)c_nk);
    if (c_nr) atomicAdd(&lc[2], (unsigned long long)c_nr);
    if (c_bt) atomicAdd(&lc[3], (unsigned long long)c_bt);
    if (c_app) atomicAdd(&lc[4], (unsigned long long)c_app);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* tp = tpart + t * T_NPART;
    tp[T_ACCEPTED] = (int64_t)lc[0];
    tp[T_NULL_KEY] = (int64_t)lc[1];
    tp[T_NULL_ROW] = (int64_t)lc[2];
    tp[T_BAD_TS] = (int64_t)lc[3];
    tp[T_APPLIED] = hop ? (int64_t)lc[4] : (int64_t)lc[0];  // none late (checked)
    tp[T_LATE] = 0;
    if (lfail) atomicOr((unsigned long long*)&ci[CI_TFAIL], 1ULL);
    int64_t* ts4 = tilestat + t * 4;
    ts4[0] = t_rmax;
    ts4[1] = t_min;
    ts4[2] = t_bound;
    ts4[3] = t_ok ? 1 : 0;
  }
}

// Chunk w of its bucket (C1V_CH records): sentinels dropped, counting-sorted by partition,
// written back in place; the segment table as k_c1_refine's.
template <int U, int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_c1v_refine(
    const ulonglong2* __restrict__ srcA, const int64_t* __restrict__ bb, const int* __restrict__ cstart, int log2B,
    int log2P, int fbits, ulonglong2* __restrict__ srec, uint16_t* __restrict__ seg, const int64_t* __restrict__ ci,
    const uint32_t* __restrict__ tbase, const uint16_t* __restrict__ rloc, const uint16_t* __restrict__ roff,
    int64_t nT, int sh, int64_t S, const uint32_t* __restrict__ cinfo) {
  if (ci_ld(ci, CI_GATE) == 0) return;
  const int w = blockIdx.x;
  if (w >= (int)ci_ld(ci, CI_NCHUNK)) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int lb, lnv;
  __shared__ int wsum[NT / 64];
  constexpr int CH = U * NT;
  static_assert(CH == C1V_CH, "refine chunk");
  const int F = 1 << fbits, B = 1 << log2B;
  uint32_t* cnt = (uint32_t*)smem;
  uint32_t* sbase = cnt + F;
  ulonglong2* stage = (ulonglong2*)(smem + (((size_t)F * 8 + 15) & ~(size_t)15));
  for (int f = threadIdx.x; f < F; f += NT) cnt[f] = 0u;
  if (threadIdx.x == 0) lb = -1;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += NT)
    if (cstart[b] <= w && w < cstart[b + 1]) lb = b;
  __syncthreads();
  const int b = lb;
  if (b < 0) return;
  const int64_t lo = bb[b] + (int64_t)(w - cstart[b]) * CH;
  const int64_t bend = bb[b + 1];
  const int len = (int)(bend - lo < CH ? bend - lo : CH);
  const int64_t kmin = ci_ld(ci, CI_KMINC);
  const uint64_t kshift = (uint64_t)ci_ld(ci, CI_KSHIFT) << 32;  // records hold key - kb
  const int shift = 64 - log2P;
  // where the chunk's records lie in the step runs (a map in the not yet used stage)
  const int64_t nSt = nT << sh;
  chunk_map(tbase + (int64_t)b * (nT + 1), rloc + (int64_t)b * nSt, roff + (int64_t)b * nSt, nSt, sh, cinfo, w, S,
            lo - bb[b], len, (uint32_t*)stage);
  ulonglong2 r[U];
  uint32_t f[U], rank[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = threadIdx.x + u * NT;
    const uint32_t src = ((const uint32_t*)stage)[j < len ? j : len - 1];
    r[u] = ld_nt2(srcA + src);
    r[u].x -= kshift;
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = threadIdx.x + u * NT;
    const bool v = j < len && (uint32_t)r[u].x != C1_SENT;
    f[u] = (uint32_t)(key_hash(kmin + (int64_t)((r[u].x >> 32) & 0x7FFFFFFFull)) >> shift) & (uint32_t)(F - 1);
    rank[u] = v ? atomicAdd(&cnt[f[u]], 1u) : 0xFFFFFFFFu;
  }
  __syncthreads();
  {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t c = t < F ? cnt[t] : 0u;
    uint32_t incl = c;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = (int)incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
      before += k < wave ? (uint32_t)wsum[k] : 0u;
      tot += (uint32_t)wsum[k];
    }
    if (t < F) {
      sbase[t] = before + incl - c;
      seg[(int64_t)w * (F + 1) + t] = (uint16_t)(before + incl - c);
    }
    if (t == 0) {
      seg[(int64_t)w * (F + 1) + F] = (uint16_t)tot;
      lnv = (int)tot;
    }
  }
  __syncthreads();
  const int nv = lnv;
#pragma unroll
  for (int u = 0; u < U; u++)
    if (rank[u] != 0xFFFFFFFFu) stage[sbase[f[u]] + rank[u]] = r[u];
  __syncthreads();
  for (int j = threadIdx.x; j < nv; j += NT) srec[lo + j] = stage[j];
}

// Merge parameters of the value pipeline.  LDS: ids ID[H + 64] | 8-byte planes (sum, min, max,
// present ones) | u32 planes (row time, COUNT(*), non-null count) | list u16[H] | segment prefix
// | segment bases | bucket bases | chunk starts (byte offsets below, from c1v_layout).
struct C1VQ {
  int32_t log2P, fbits, log2H, sw, hmax, f64, fan;
  int32_t off_sum, off_min, off_max, off_rt, off_star, off_cnt, off_list, off_spre;
  int32_t word_op[C1V_MAXW];  // kind of the update op writing row word k (-1: none)
  int64_t size, adv, cmax;
  FastDiv fd;
  FastDiv32 fd32;
  uint64_t init[C1V_MAXW];
  HavingDev having;
  uint8_t* chg;
};

template <class T>
__device__ __forceinline__ KLDS T* c1v_plane(char* smem, int off) {
  return (KLDS T*)((KLDS char*)smem + off);
}

// Plane masks: a merge instantiation specialised for the planes a query has (PM != 0, the
// benchmarks' shapes), or PM = 0 reading them from the parameters (every other shape).
constexpr int PM_STAR = 1, PM_CNT = 2, PM_SUM = 4, PM_MIN = 8, PM_MAX = 16, PM_F64 = 32, PM_SPEC = 64;
constexpr int PM_C5 = PM_SPEC | PM_SUM;                                   // SUM(BIGINT)
constexpr int PM_C3 = PM_SPEC | PM_CNT | PM_SUM | PM_MIN | PM_MAX | PM_F64;  // SUM/AVG/MIN/MAX(DOUBLE)
template <int PM>
struct C1VP {
  const C1VQ& q;
  __device__ __forceinline__ bool star() const { return PM ? (PM & PM_STAR) != 0 : q.off_star >= 0; }
  __device__ __forceinline__ bool cnt() const { return PM ? (PM & PM_CNT) != 0 : q.off_cnt >= 0; }
  __device__ __forceinline__ bool sum() const { return PM ? (PM & PM_SUM) != 0 : q.off_sum >= 0; }
  __device__ __forceinline__ bool mn() const { return PM ? (PM & PM_MIN) != 0 : q.off_min >= 0; }
  __device__ __forceinline__ bool mx() const { return PM ? (PM & PM_MAX) != 0 : q.off_max >= 0; }
  __device__ __forceinline__ bool f64() const { return PM ? (PM & PM_F64) != 0 : q.f64 != 0; }
};

// Row word k (k >= 3) of a (key, window) combined with delta entry e: the word's update op
// applied to the entry's plane.
template <int PM>
__device__ __forceinline__ uint64_t c1v_word(const C1VQ& q, char* smem, int e, int k, uint64_t w) {
  const C1VP<PM> v{q};
  switch (q.word_op[k]) {
    case OP_INC: return v.star() ? w + c1v_plane<uint32_t>(smem, q.off_star)[e] : w;
    case OP_INC_VALID: return v.cnt() ? w + c1v_plane<uint32_t>(smem, q.off_cnt)[e] : w;
    case OP_ADD_I64: return v.sum() && !v.f64() ? w + c1v_plane<uint64_t>(smem, q.off_sum)[e] : w;
    case OP_ADD_F64:
      if (v.sum() && v.f64()) {
        double a, b = c1v_plane<double>(smem, q.off_sum)[e];
        __builtin_memcpy(&a, &w, 8);
        a += b;
        __builtin_memcpy(&w, &a, 8);
      }
      return w;
    case OP_MIN:
      if (v.mn()) {
        const int64_t m = c1v_plane<int64_t>(smem, q.off_min)[e];
        if (m < (int64_t)w) w = (uint64_t)m;
      }
      return w;
    case OP_MAX:
      if (v.mx()) {
        const int64_t m = c1v_plane<int64_t>(smem, q.off_max)[e];
        if (m > (int64_t)w) w = (uint64_t)m;
      }
      return w;
    default: return w;
  }
}

// Write one row word by word (no row array in registers: the write-out runs while the next
// item's record chunks are in flight), from the resident row (src) or, src == nullptr, from the
// initial words + key / window start / row time; e >= 0: combined with delta entry e (rtabs =
// its row time).  *was / *now: the HAVING before and after.
template <int PM>
__device__ __forceinline__ void c1v_emit(const C1VQ& q, char* smem, uint64_t* __restrict__ dst,
                                         const uint64_t* __restrict__ src, int e, int64_t key, int64_t ws, int64_t rtabs,
                                         bool* was, bool* now) {
  const int hv = q.having.a.w_val, hc = q.having.a.w_cnt;
  uint64_t ov = 0, oc = 0, nv = 0, nc = 0;
#pragma unroll
  for (int k = 0; k < C1V_MAXW; k++) {
    if (k >= q.sw) break;
    uint64_t w = src ? src[k] : (k == 0 ? (uint64_t)key : k == 1 ? (uint64_t)ws : k == 2 ? (uint64_t)rtabs : q.init[k]);
    if (k == hv) ov = w;
    if (k == hc) oc = w;
    if (e >= 0) {
      if (k == 2 && src) w = rtabs > (int64_t)w ? (uint64_t)rtabs : w;
      if (k >= 3) w = c1v_word<PM>(q, smem, e, k, w);
    }
    if (k == hv) nv = w;
    if (k == hc) nc = w;
    dst[k] = w;
  }
  *was = q.having.active ? having_ok_words(ov, oc, q.having) : true;
  *now = q.having.active ? having_ok_words(nv, nc, q.having) : true;
}

// Clear delta entry e for the next item.
template <int PM>
__device__ __forceinline__ void c1v_clear(const C1VQ& q, char* smem, int e) {
  const C1VP<PM> v{q};
  c1v_plane<uint32_t>(smem, q.off_rt)[e] = 0u;
  if (v.star()) c1v_plane<uint32_t>(smem, q.off_star)[e] = 0u;
  if (v.cnt()) c1v_plane<uint32_t>(smem, q.off_cnt)[e] = 0u;
  if (v.sum()) c1v_plane<uint64_t>(smem, q.off_sum)[e] = 0ULL;
  if (v.mn()) c1v_plane<int64_t>(smem, q.off_min)[e] = INT64_MAX;
  if (v.mx()) c1v_plane<int64_t>(smem, q.off_max)[e] = INT64_MIN;
}

// One (record or pane) contribution into delta entry e: row time, then the update planes.
// cv: the argument's non-null count (a record: 0 / 1), sum its bits (sum), mn / mx its order keys.
template <int PM>
__device__ __forceinline__ void c1v_add(const C1VQ& q, char* smem, uint32_t e, uint32_t tr, uint32_t cs, uint32_t cv,
                                        uint64_t sum, int64_t mn, int64_t mx) {
  const C1VP<PM> v{q};
  KLDS uint32_t* prt = &c1v_plane<uint32_t>(smem, q.off_rt)[e];
  __hip_atomic_fetch_max(prt, tr, WG_RLX);
  if (v.star() && cs) __hip_atomic_fetch_add(&c1v_plane<uint32_t>(smem, q.off_star)[e], cs, WG_RLX);
  if (cv) {
    if (v.cnt()) __hip_atomic_fetch_add(&c1v_plane<uint32_t>(smem, q.off_cnt)[e], cv, WG_RLX);
    if (v.sum()) {
      if (v.f64()) {
        double d;
        __builtin_memcpy(&d, &sum, 8);
        __hip_atomic_fetch_add(&c1v_plane<double>(smem, q.off_sum)[e], d, WG_RLX);
      } else {
        __hip_atomic_fetch_add(&c1v_plane<uint64_t>(smem, q.off_sum)[e], sum, WG_RLX);
      }
    }
    if (v.mn()) {
      KLDS int64_t* pm = &c1v_plane<int64_t>(smem, q.off_min)[e];
      __hip_atomic_fetch_min(pm, mn, WG_RLX);
    }
    if (v.mx()) {
      KLDS int64_t* pm = &c1v_plane<int64_t>(smem, q.off_max)[e];
      __hip_atomic_fetch_max(pm, mx, WG_RLX);
    }
  }
}

// identity of (krel, relative window or pane index): u32 krel << (wbits + PB) | pane << wbits | wi,
// u64 krel << 32 | pane << 31 | wi
template <class ID, bool PANES>
__device__ __forceinline__ ID c1v_id(uint64_t krel, uint64_t wi, bool pane, int wbits) {
  if constexpr (sizeof(ID) == 4)
    return (ID)(((uint32_t)krel << (wbits + (PANES ? 1 : 0))) | ((PANES && pane) ? (1u << wbits) : 0u) | (uint32_t)wi);
  else
    return (ID)((krel << 32) | ((PANES && pane) ? (1ULL << 31) : 0ULL) | wi);
}
template <class ID, bool PANES>
__device__ __forceinline__ bool c1v_is_pane(ID id, int wbits) {
  if constexpr (!PANES) return false;
  if constexpr (sizeof(ID) == 4) return ((uint32_t)id >> wbits) & 1u;
  else return ((uint64_t)id >> 31) & 1ULL;
}

// WPE: waves per SIMD the register budget allows (4: <= 128 VGPRs, two workgroups per CU; 2:
// <= 256, one)
template <int NT, int AU, class ID, bool PANES, int WPE, int PM>
__global__ __launch_bounds__(NT, WPE) void k_c1v_merge(
    const C1VQ* __restrict__ qp, const uint32_t* __restrict__ work, int64_t nwork, const int64_t* __restrict__ bb,
    const int* __restrict__ cstart, const uint16_t* __restrict__ seg, const ulonglong2* __restrict__ srec, int first,
    uint64_t* __restrict__ buf0, uint64_t* __restrict__ buf1, const uint8_t* __restrict__ sel,
    const int64_t* __restrict__ cnt, unsigned long long* __restrict__ newcnt, uint8_t* __restrict__ fail,
    unsigned long long* __restrict__ need, int64_t close0, uint64_t* __restrict__ closed,
    unsigned long long* __restrict__ closed_n, unsigned long long closed_cap, const int64_t* __restrict__ ci,
    unsigned long long* __restrict__ hnew,
    unsigned long long* __restrict__ hclosed, uint32_t* __restrict__ prn, unsigned long long* __restrict__ dbg) {
  if (ci_ld(ci, CI_GATE) == 0) return;
  if ((ci_ld(ci, CI_ID32) != 0) != (sizeof(ID) == 4)) return;  // the other identity width's
  const C1VQ& q = *qp;  // in device memory: its fields are loaded where used (SGPR pressure)
  constexpr int NW = NT / 64;
  constexpr ID EMPTY = (ID)~(ID)0;
  const int log2H = q.log2H;
  const int H = 1 << log2H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  KLDS ID* ids = (KLDS ID*)(KLDS char*)smem;
  KLDS uint32_t* rt = c1v_plane<uint32_t>(smem, q.off_rt);
  KLDS uint16_t* list = c1v_plane<uint16_t>(smem, q.off_list);
  KLDS uint64_t* sg2 = c1v_plane<uint64_t>(smem, q.off_spre);  // as k_c1_merge's
  KLDS uint16_t* segof = (KLDS uint16_t*)(sg2 + C1_SEGMAX + 4);
  // the bucket tables (chunk starts, bucket bases) are read from memory per item (their 3 KB of
  // LDS let a 2^12-entry table of 32-bit identities fit two workgroups per CU)
  __shared__ int lovf, nnew;
  __shared__ int wsum[NW], csum[NW];
  __shared__ unsigned long long lbase, cbase;
  const int F = 1 << q.fbits;
  const int64_t wbase = ci_ld(ci, CI_WBASE), whi = ci_ld(ci, CI_WHI), T0 = ci_ld(ci, CI_T0), tmin = ci_ld(ci, CI_TMIN);
  const int wbits = (int)ci_ld(ci, CI_WBITS);
  const int64_t kmin = ci_ld(ci, CI_KMINC);
  const uint64_t krange = (uint64_t)ci_ld(ci, CI_KRANGE);
  const int32_t tmin32 = (int32_t)(tmin - T0);
  const int64_t wstart = wbase * q.adv;
  const bool r32 = ci_ld(ci, CI_TMAX) - wstart < ((int64_t)1 << 32);
  const uint32_t tsh32 = (uint32_t)(T0 - wstart);
  const bool evict = close0 != INT64_MIN;
  C1M_T0;
  const uint32_t dummy = (uint32_t)H + (uint32_t)lane;
  for (int i = threadIdx.x; i < H + 64; i += NT) {
    ids[i] = EMPTY;
    c1v_clear<PM>(q, smem, i);
  }
  if (threadIdx.x == 0) {
    lovf = 0;
    nnew = 0;
  }
  // identity and slot hash of a resident row (false: no record of this push can match it).
  // Sub-passes split a partition by KEY (subh): a pane and its windows stay in one sub-pass.
  auto row_id = [&](const uint64_t* row, ID* id, uint32_t* h) -> bool {
    const int64_t wi = (int64_t)fast_udiv((uint64_t)row[1], q.fd) - wbase;
    const uint64_t krel = (uint64_t)((int64_t)row[0] - kmin);
    if (krel > krange || wi < 0 || wi > whi) return false;
    *id = c1v_id<ID, PANES>(krel, (uint64_t)wi, false, wbits);
    *h = c1_hash<ID>(*id);
    return true;
  };
  auto subh = [&](int64_t key) -> uint32_t { return (uint32_t)(uint64_t)(key - kmin) * 0x9E3779B1u; };
  // probe for id from its home slot; claims it if absent (listed); -1 when the table is full
  auto claim = [&](ID id, bool act) -> int {
    uint32_t e = act ? c1_hash<ID>(id) >> (32 - log2H) : dummy;
    ID old = EMPTY;
    __hip_atomic_compare_exchange_strong(&ids[e], &old, act ? id : EMPTY, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
    bool got = act && old == EMPTY;
    bool pend = act && old != EMPTY && old != id;
    for (int probes = 1;; probes++) {
      if (!__ballot(pend)) break;
      if (probes >= H) {  // the table is full: the item is retried (claimed entries stay listed)
        if (pend) {
          lovf = 1;
          act = false;
        }
        pend = false;
        break;
      }
      if (pend) {
        e = (e + 1) & (uint32_t)(H - 1);
        ID o2 = EMPTY;
        __hip_atomic_compare_exchange_strong(&ids[e], &o2, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
        got = o2 == EMPTY;
        pend = o2 != EMPTY && o2 != id;
      }
    }
    mg_list_append(act && got, e, list, &nnew);
    return act ? (int)e : -1;
  };
  struct Pre {
    uint32_t p;
    int sbits, sub, nseg;
    int64_t nrow, bb0;
    uint32_t selw;
    uint16_t s00, s01, s10, s11;
  };
  struct It {
    uint32_t p;
    int sbits, sub, nseg, segb;  // segb: log2 of the records per segment-lookup block
    int64_t rn, nrow;
    bool isel;
  };
  auto fetch = [&](int64_t w, Pre& r) {
    uint32_t p;
    int sbits = 0, sub = 0;
    if (work) {
      const uint32_t x = work[w];
      p = x & 0xFFFFu;
      sbits = (x >> 16) & 0xF;
      sub = (int)(x >> 20);
    } else {
      p = (uint32_t)w;
    }
    p = __builtin_amdgcn_readfirstlane(p);
    const int b = (int)(p >> q.fbits), f = (int)(p & (uint32_t)(F - 1));
    const int cs = cstart[b];
    int nseg = cstart[b + 1] - cs;
    if (nseg < 0 || nseg > C1_SEGMAX) nseg = 0;
    r.p = p;
    r.sbits = sbits;
    r.sub = sub;
    r.nseg = nseg;
    r.nrow = cnt[p];
    r.selw = ((const uint32_t*)sel)[p >> 2];
    r.bb0 = bb[b];
    const int k0 = threadIdx.x * 2;
    r.s00 = r.s01 = r.s10 = r.s11 = 0;
    if (k0 < nseg) {
      const uint16_t* sg = seg + (int64_t)(cs + k0) * (F + 1) + f;
      r.s00 = sg[0];
      r.s01 = sg[1];
    }
    if (k0 + 1 < nseg) {
      const uint16_t* sg = seg + (int64_t)(cs + k0 + 1) * (F + 1) + f;
      r.s10 = sg[0];
      r.s11 = sg[1];
    }
  };
  auto prep = [&](const Pre& r, It& it) {
    const int nseg = r.nseg;
    it.p = r.p;
    it.sbits = r.sbits;
    it.sub = r.sub;
    it.nseg = nseg;
    it.nrow = r.nrow;
    it.isel = ((r.selw >> (8 * (r.p & 3))) & 0xFFu) != 0;
    const int k0 = threadIdx.x * 2;
    const int len0 = k0 < nseg ? (int)r.s01 - (int)r.s00 : 0;
    const int len1 = k0 + 1 < nseg ? (int)r.s11 - (int)r.s10 : 0;
    const int64_t base0 = r.bb0 + (int64_t)k0 * C1V_CH + r.s00;
    const int64_t base1 = r.bb0 + (int64_t)(k0 + 1) * C1V_CH + r.s10;
    const int s = len0 + len1;
    int incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    lds_barrier();
    int before = 0;
    int tot = 0;
    for (int k = 0; k < NW; k++) {
      before += k < wave ? wsum[k] : 0;
      tot += wsum[k];
    }
    const int ex = before + incl - s;
    // the finest lookup block that covers the item in C1_SEGOF entries (segments hold C1_CH / F
    // records on average: 32-record blocks make the lookup a read and at most a step or two)
    const int segb = tot <= (C1_SEGOF << 5) ? 5 : (tot <= (C1_SEGOF << 6) ? 6 : C1_SEGB);
    const int bm = (1 << segb) - 1;
    if (k0 < nseg) {
      sg2[k0] = (uint32_t)ex | (uint64_t)(uint32_t)(int32_t)(base0 - ex) << 32;
    }
    if (k0 + 1 < nseg) {
      sg2[k0 + 1] = (uint32_t)(ex + len0) | (uint64_t)(uint32_t)(int32_t)(base1 - (ex + len0)) << 32;
    }
    // segment lookup: block j (records [j << segb, (j + 1) << segb)) starts in segment segof[j]
    for (int bj = (ex + bm) >> segb, be = (ex + len0 + bm) >> segb; bj < be && bj < C1_SEGOF; bj++)
      segof[bj] = (uint16_t)k0;
    for (int bj = (ex + len0 + bm) >> segb, be = (ex + s + bm) >> segb; bj < be && bj < C1_SEGOF; bj++)
      segof[bj] = (uint16_t)(k0 + 1);
    if (k0 < nseg && k0 + 2 >= nseg) sg2[nseg] = (uint32_t)(ex + s);
    if (nseg == 0 && threadIdx.x == 0) sg2[0] = 0u;
    lds_barrier();
    it.rn = (uint32_t)sg2[nseg];
    it.segb = segb;
  };
  ulonglong2 ra[AU], rb[AU];
  auto load = [&](ulonglong2 (&x)[AU], int64_t l0, int64_t rn, int nseg, int segb) {
#pragma unroll
    for (int u = 0; u < AU; u++) {
      int64_t li = l0 + threadIdx.x + (int64_t)u * NT;
      li = li < rn ? li : rn - 1;
      int lo = 0;  // the last segment starting at or before li
      int64_t at;
      if (rn <= ((int64_t)C1_SEGOF << segb)) {  // from the block's segment, a step or two on
        lo = segof[li >> segb];
        uint64_t sa = sg2[lo], sb = sg2[lo + 1];
        while (lo + 1 < nseg && (int64_t)(uint32_t)sb <= li) {
          lo++;
          sa = sb;
          sb = sg2[lo + 1];
        }
        at = (int64_t)(int32_t)(sa >> 32) + li;
      } else {
        int hi = nseg;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if ((int64_t)(uint32_t)sg2[mid] <= li) lo = mid;
          else hi = mid;
        }
        at = (int64_t)(int32_t)(sg2[lo] >> 32) + li;
      }
      x[u] = ld_nt2(srec + at);
    }
  };
  auto load01 = [&](const It& x) {
    if (x.rn > 0) load(ra, 0, x.rn, x.nseg, x.segb);
    if (x.rn > (int64_t)AU * NT) load(rb, (int64_t)AU * NT, x.rn, x.nseg, x.segb);
  };
  lds_barrier();  // the table and flags initialised above
  Pre pr{};
  It nx{};
  if (blockIdx.x < nwork) {
    fetch(blockIdx.x, pr);
    prep(pr, nx);
    load01(nx);
  }
  for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const It it = nx;
    const uint32_t p = it.p;
    const int sbits = it.sbits, sub = it.sub, nseg = it.nseg, segb = it.segb;
    const int64_t rn = it.rn, nrow = it.nrow;
    const bool isel = it.isel;
    const int64_t wn = w + gridDim.x;
    if (wn < nwork) fetch(wn, pr);
    if (first && threadIdx.x == 0) prn[p] = (uint32_t)rn;
    if (rn == 0 && first) {
      if (wn < nwork) {
        prep(pr, nx);
        load01(nx);
      }
      continue;
    }
    const uint64_t* src = (isel ? buf1 : buf0) + (uint64_t)p * q.cmax * q.sw;
    // (closed resident rows leave for the closed store in the write-out, phase 4: one pass over the
    // resident rows there, the closed store's slots reserved with the region's)
    // An item that fails on the first pass moves them here instead (count, reserve, copy), since
    // its retries skip them (as k_c1_merge).
    auto evict_failed = [&]() {
      if (!first || !evict || nrow == 0) return;  // (uniform)
      auto mine_closed = [&](const uint64_t* row) -> bool {
        return (int64_t)row[1] + q.size <= close0 && (!sbits || (int)c1_sub(subh((int64_t)row[0]), sbits) == sub);
      };
      int n_cl = 0;
      for (int64_t r = threadIdx.x; r < nrow; r += NT) n_cl += mine_closed(src + r * q.sw) ? 1 : 0;
      const int wave_cl = (int)wave_sum(n_cl);
      if (lane == 0) csum[wave] = wave_cl;
      lds_barrier();
      int cl_before = 0, cl_total = 0;
      for (int k = 0; k < NW; k++) {
        if (k < wave) cl_before += csum[k];
        cl_total += csum[k];
      }
      if (threadIdx.x == 0)
        cbase = c1_reserve_closed(closed_n, (unsigned long long)cl_total, closed_cap, &fail[p], need);
      lds_barrier();
      const unsigned long long cb = cbase;
      if (cl_total == 0 || cb == C1_NOSLOT) return;
      uint64_t ccur = cb + (uint64_t)cl_before;
      const uint64_t lt = (1ULL << lane) - 1;
      int nhc = 0;
      for (int64_t r0 = wave * 64; r0 < nrow; r0 += NT) {
        const int64_t r = r0 + lane;
        const uint64_t* row = src + (r < nrow ? r : 0) * q.sw;
        const bool cl = r < nrow && mine_closed(row);
        const uint64_t bc = __ballot(cl);
        if (cl) {
          uint64_t* cd = closed + (ccur + __popcll(bc & lt)) * q.sw;
          for (int k = 0; k < q.sw; k++) cd[k] = row[k];
          nhc += having_ok_words(q.having.a.w_val >= 0 ? row[q.having.a.w_val] : 0,
                                 q.having.a.w_cnt >= 0 ? row[q.having.a.w_cnt] : 0, q.having) ? 1 : 0;
        }
        ccur += __popcll(bc);
      }
      if (q.having.active) {
        nhc = (int)wave_sum(nhc);
        if (lane == 0 && nhc) atomicAdd(hclosed, (unsigned long long)nhc);
      }
    };
    C1M_T(0);
    // 1. records → their pane (window) entries: the AU identities' CASes back to back, then the
    //    collisions probe on together (as k_c1_merge)
    //    The set's next chunk is loaded into the same registers right after the CASes are issued
    //    (prefetch; what the planes need is kept aside first), as k_c1_merge.
    auto apply = [&](const ulonglong2 (&xr)[AU], int64_t l0, auto R32, auto&& prefetch) -> bool {
      ID id[AU];
      uint32_t e[AU], trv[AU];
      uint64_t arg[AU];
      bool pend[AU], claimed[AU], nn[AU];
#pragma unroll
      for (int u = 0; u < AU; u++) {
        const int64_t li = l0 + threadIdx.x + (int64_t)u * NT;
        const uint64_t w0 = xr[u].x;
        trv[u] = (uint32_t)((int32_t)(uint32_t)w0 - tmin32) + 1u;
        nn[u] = (w0 >> 63) != 0;
        arg[u] = xr[u].y;
        const uint64_t krel = (w0 >> 32) & 0x7FFFFFFFull;
        uint64_t wi;
        if constexpr (decltype(R32)::value) wi = fast_udiv32((uint32_t)w0 + tsh32, q.fd32);
        else wi = fast_udiv((uint64_t)(T0 + (int64_t)(int32_t)(uint32_t)w0), q.fd) - (uint64_t)wbase;
        const ID x = c1v_id<ID, PANES>(krel, wi, PANES, wbits);
        bool act = li < rn;
        if (sbits) act = act && (int)c1_sub((uint32_t)krel * 0x9E3779B1u, sbits) == sub;
        id[u] = act ? x : EMPTY;
        e[u] = act ? c1_hash<ID>(x) >> (32 - log2H) : dummy;
      }
      ID old[AU];
#pragma unroll
      for (int u = 0; u < AU; u++) {
        old[u] = EMPTY;
        __hip_atomic_compare_exchange_strong(&ids[e[u]], &old[u], id[u], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      const int full = *(volatile KLDS int*)&lovf;
      prefetch();
#pragma unroll
      for (int u = 0; u < AU; u++) {
        claimed[u] = id[u] != EMPTY && old[u] == EMPTY;
        pend[u] = old[u] != EMPTY && old[u] != id[u];
      }
      for (int probes = 1;; probes++) {
        bool anyp = false;
#pragma unroll
        for (int u = 0; u < AU; u++) anyp |= pend[u];
        if (!__ballot(anyp)) break;
        if (probes >= H) {
          lovf = 1;
#pragma unroll
          for (int u = 0; u < AU; u++)
            if (pend[u]) id[u] = EMPTY;
          break;
        }
#pragma unroll
        for (int u = 0; u < AU; u++) {
          if (!pend[u]) continue;
          e[u] = (e[u] + 1) & (uint32_t)(H - 1);
          ID o2 = EMPTY;
          __hip_atomic_compare_exchange_strong(&ids[e[u]], &o2, id[u], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
          claimed[u] = o2 == EMPTY;
          pend[u] = o2 != EMPTY && o2 != id[u];
        }
      }
      int nnow;
      {
        bool cl[AU];
#pragma unroll
        for (int u = 0; u < AU; u++) cl[u] = claimed[u] && id[u] != EMPTY;
        nnow = mg_list_append_n<AU>(cl, e, list, &nnew);
      }
#pragma unroll
      for (int u = 0; u < AU; u++) {
        if (id[u] == EMPTY) continue;
        int64_t ok_ = (int64_t)arg[u];
        if (C1VP<PM>{q}.f64() && (C1VP<PM>{q}.mn() || C1VP<PM>{q}.mx())) {
          double d;
          __builtin_memcpy(&d, &arg[u], 8);
          ok_ = f64_order_key(d);
        }
        c1v_add<PM>(q, smem, e[u], trv[u], 1u, nn[u] ? 1u : 0u, arg[u], ok_, ok_);
      }
      return !full && nnow <= q.hmax;
    };
    const int64_t nch = (rn + (int64_t)AU * NT - 1) / ((int64_t)AU * NT);
    if (rn > 0 && PANES) {
      // HOPPING items run many chunks (C3: ~8): a straight-line body (a chunk past the end applies
      // nothing; its loads, clamped to the last record, read one line) whose wait for one register
      // set counts the other set's loads as in flight; the table-full check once per two chunks
      auto records = [&](auto R32) {
        for (int64_t c = 0; c < nch; c += 2) {
          const bool ga = apply(ra, c * AU * NT, R32, [&] { load(ra, (c + 2) * AU * NT, rn, nseg, segb); });
          const bool gb = apply(rb, (c + 1) * AU * NT, R32, [&] { load(rb, (c + 3) * AU * NT, rn, nseg, segb); });
          if (!ga || !gb) break;
        }
      };
      if (r32) records(std::true_type{});
      else records(std::false_type{});
    } else if (rn > 0) {
      for (int64_t c = 0; c < nch; c += 2) {
        auto pa = [&] { if (c + 2 < nch) load(ra, (c + 2) * AU * NT, rn, nseg, segb); };
        const bool ga = r32 ? apply(ra, c * AU * NT, std::true_type{}, pa) : apply(ra, c * AU * NT, std::false_type{}, pa);
        if (!ga || c + 1 >= nch) break;
        auto pb = [&] { if (c + 3 < nch) load(rb, (c + 3) * AU * NT, rn, nseg, segb); };
        const bool gb = r32 ? apply(rb, (c + 1) * AU * NT, std::true_type{}, pb)
                            : apply(rb, (c + 1) * AU * NT, std::false_type{}, pb);
        if (!gb) break;
      }
    }
    lds_barrier();
    if (wn < nwork) {
      prep(pr, nx);
      load01(nx);
    }
    C1M_T(1);
    // 1b. panes → their windows (the window entries are claimed as a record's would be)
    if (PANES && q.fan > 1 && !lovf && nnew <= q.hmax) {
      const int nn0 = nnew;
      lds_barrier();  // every thread has read nn0 before the fold lists windows
      for (int i0 = 0; i0 < nn0; i0 += NT) {  // uniform trip count: claim's ballots converge
        const int li = i0 + threadIdx.x;
        const int pe = li < nn0 ? (int)list[li] : 0;
        const ID pid = li < nn0 ? ids[pe] : EMPTY;
        const bool isp = li < nn0 && pid != EMPTY && c1v_is_pane<ID, PANES>(pid, wbits);
        uint64_t krel, pw;
        if constexpr (sizeof(ID) == 4) {
          krel = (uint64_t)((uint32_t)pid >> (wbits + 1));
          pw = (uint64_t)((uint32_t)pid & ((1u << wbits) - 1u));
          if (wbits == 0) pw = 0;
        } else {
          krel = (uint64_t)pid >> 32;
          pw = (uint64_t)pid & 0x7FFFFFFFull;
        }
        const uint32_t prt = isp ? rt[pe] : 0u;
        const C1VP<PM> pv{q};
        const uint32_t pcs = isp && pv.star() ? c1v_plane<uint32_t>(smem, q.off_star)[pe] : 0u;
        const uint32_t pcv = isp && pv.cnt() ? c1v_plane<uint32_t>(smem, q.off_cnt)[pe] : (isp ? 1u : 0u);
        const uint64_t psum = isp && pv.sum() ? c1v_plane<uint64_t>(smem, q.off_sum)[pe] : 0ULL;
        const int64_t pmn = isp && pv.mn() ? c1v_plane<int64_t>(smem, q.off_min)[pe] : INT64_MAX;
        const int64_t pmx = isp && pv.mx() ? c1v_plane<int64_t>(smem, q.off_max)[pe] : INT64_MIN;
        for (int j = 0; j < q.fan; j++) {
          // window pw - j (its start is >= 0: windowsFor never returns a negative start)
          const bool act = isp && (int64_t)pw - j + wbase >= 0 && (int64_t)pw - j >= 0;
          const int e = claim(c1v_id<ID, PANES>(krel, pw - (uint64_t)j, false, wbits), act);
          if (e >= 0) c1v_add<PM>(q, smem, (uint32_t)e, prt, pcs, pcv, psum, pmn, pmx);
        }
      }
      lds_barrier();
    }
    C1M_T(2);
    const int nl = nnew < H ? nnew : H;
    if (lovf || nnew > q.hmax) {
      if (threadIdx.x == 0) fail[p] |= 1;
      for (int i = threadIdx.x; i < nl; i += NT) {
        const uint32_t e = list[i];
        ids[e] = EMPTY;
        c1v_clear<PM>(q, smem, (int)e);
      }
      evict_failed();
      lds_barrier();
      if (threadIdx.x == 0) {
        lovf = 0;
        nnew = 0;
      }
      lds_barrier();
      continue;
    }
    // 2. resident rows: mark the delta entries they absorb; count live and closed rows
    int n_mine = 0, n_cl = 0;
    for (int64_t r = threadIdx.x; r < nrow; r += NT) {
      const uint64_t* row = src + r * q.sw;
      if (sbits && (int)c1_sub(subh((int64_t)row[0]), sbits) != sub) continue;
      if (evict && (int64_t)row[1] + q.size <= close0) {
        n_cl += first ? 1 : 0;  // (a later pass: the first one moved it)
        continue;
      }
      ID id;
      uint32_t h;
      const bool has = row_id(row, &id, &h);
      if (has) {
        const int e = c1_find_id<ID>(ids, id, h >> (32 - log2H), H);
        if (e >= 0) rt[e] |= RT_MATCHED;
      }
      n_mine++;
    }
    if (nrow > 0) lds_barrier();  // the marks before the list walk reads them (uniform: nrow is the item's)
    const int per = ((nl + NW - 1) / NW + 63) & ~63;
    const int lb0 = wave * per, lb1 = lb0 + per < nl ? lb0 + per : nl;
    int nnw = 0;
    for (int k = lb0; k < lb1; k += 64) {
      const int i = k + lane;
      const uint32_t e = i < lb1 ? list[i] : dummy;
      const bool isnew = i < lb1 && !(rt[e] & RT_MATCHED) && !c1v_is_pane<ID, PANES>(ids[e], wbits);
      nnw += (int)__popcll(__ballot(isnew));
    }
    // 3. the partition's region range, and the closed store's slots for its closed rows
    const int wave_rows = (int)wave_sum(n_mine) + nnw;
    const int wave_cl = (int)wave_sum(n_cl);
    if (lane == 0) {
      wsum[wave] = wave_rows;
      csum[wave] = wave_cl;
    }
    lds_barrier();
    int wave_before = 0, total = 0, cl_before = 0, cl_total = 0;
    for (int k = 0; k < NW; k++) {
      if (k < wave) wave_before += wsum[k], cl_before += csum[k];
      total += wsum[k];
      cl_total += csum[k];
    }
    if (threadIdx.x == 0) {
      if (work) lbase = total ? atomicAdd(&newcnt[p], (unsigned long long)total) : 0ULL;
      else {
        lbase = 0;
        newcnt[p] = (unsigned long long)total;
      }
      // (an item that does not fit its region reserves with its own copy, evict_failed)
      cbase = (int64_t)(lbase + total) <= q.cmax
                  ? c1_reserve_closed(closed_n, (unsigned long long)cl_total, closed_cap, &fail[p], need)
                  : 0ULL;
    }
    lds_barrier();
    if ((int64_t)(lbase + total) > q.cmax) {
      if (threadIdx.x == 0) {
        fail[p] |= 2;
        atomicMax(need, (unsigned long long)(lbase + total));
      }
      for (int i = threadIdx.x; i < nl; i += NT) {
        const uint32_t e = list[i];
        ids[e] = EMPTY;
        c1v_clear<PM>(q, smem, (int)e);
      }
      evict_failed();
      lds_barrier();
      if (threadIdx.x == 0) nnew = 0;
      lds_barrier();
      continue;
    }
    C1M_T(3);
    // 4. write: resident rows (merged; closed ones to the closed store), then the wave's new window
    //    entries
    uint64_t* dst0 = (isel ? buf0 : buf1) + (uint64_t)p * q.cmax * q.sw;
    uint64_t cur = lbase + (uint64_t)wave_before;
    uint64_t ccur = cbase + (uint64_t)cl_before;
    const bool cmove = first && cbase != C1_NOSLOT;  // closed rows are copied (else only dropped)
    const uint64_t lt = (1ULL << lane) - 1;
    int nh = 0, nhc = 0;
    for (int64_t r0 = wave * 64; r0 < nrow; r0 += NT) {
      const int64_t r = r0 + lane;
      const uint64_t* row = src + (r < nrow ? r : 0) * q.sw;
      const bool mine = r < nrow && (!sbits || (int)c1_sub(subh((int64_t)row[0]), sbits) == sub);
      const bool cl = mine && evict && (int64_t)row[1] + q.size <= close0;
      const bool live = mine && !cl;
      int e = -1;
      if (live) {
        ID id;
        uint32_t h;
        if (row_id(row, &id, &h)) e = c1_find_id<ID>(ids, id, h >> (32 - log2H), H);
      }
      const uint64_t bc = __ballot(cl);
      if (cl && cmove) {  // (the query's HAVING alone: the merge's copy never carries pull / retention / FINAL bounds)
        uint64_t* cd = closed + (ccur + __popcll(bc & lt)) * q.sw;
        for (int k = 0; k < q.sw; k++) cd[k] = row[k];
        nhc += having_ok_words(q.having.a.w_val >= 0 ? row[q.having.a.w_val] : 0,
                               q.having.a.w_cnt >= 0 ? row[q.having.a.w_cnt] : 0, q.having) ? 1 : 0;
      }
      ccur += __popcll(bc);
      const uint64_t bl = __ballot(live);
      if (live) {
        const uint64_t ri = cur + __popcll(bl & lt);
        uint64_t* dst = dst0 + ri * q.sw;
        bool was, now;
        const int64_t t = e >= 0 ? tmin + (int64_t)(rt[e] & ~RT_MATCHED) - 1 : 0;
        c1v_emit<PM>(q, smem, dst, row, e, 0, 0, t, &was, &now);
        nh += q.having.active && now ? 1 : 0;
        if (q.chg)
          q.chg[(uint64_t)p * q.cmax + ri] =
              e >= 0 ? (uint8_t)(CHG_TOUCHED | (was ? CHG_OLD : 0) | (now ? CHG_NEW : 0)) : (uint8_t)0;
      }
      cur += __popcll(bl);
    }
    if (nrow > 0) lds_barrier();  // the resident rows have read their entries before the walk clears them
    const uint32_t wmask = wbits ? (1u << wbits) - 1u : 0u;
    for (int k = lb0; k < lb1; k += 64) {
      const int i = k + lane;
      const uint32_t e = i < lb1 ? list[i] : dummy;
      const uint32_t rv = rt[e];
      const ID id = ids[e];
      const bool isnew = i < lb1 && !(rv & RT_MATCHED) && !c1v_is_pane<ID, PANES>(id, wbits);
      const uint64_t bl = __ballot(isnew);
      if (isnew) {
        const uint64_t ri = cur + __popcll(bl & lt);
        uint64_t* dst = dst0 + ri * q.sw;
        int64_t key, wi;
        if constexpr (sizeof(ID) == 4) {
          key = kmin + (int64_t)((uint32_t)id >> (wbits + (PANES ? 1 : 0)));
          wi = (int64_t)((uint32_t)id & wmask);
        } else {
          key = kmin + (int64_t)((uint64_t)id >> 32);
          wi = (int64_t)((uint64_t)id & 0x7FFFFFFFull);
        }
        bool was, now;
        c1v_emit<PM>(q, smem, dst, nullptr, (int)e, key, (wbase + wi) * q.adv, tmin + (int64_t)rv - 1, &was, &now);
        nh += q.having.active && now ? 1 : 0;
        if (q.chg) q.chg[(uint64_t)p * q.cmax + ri] = (uint8_t)(CHG_TOUCHED | (now ? CHG_NEW : 0));
      }
      if (i < lb1) {
        ids[e] = EMPTY;
        c1v_clear<PM>(q, smem, (int)e);
      }
      cur += __popcll(bl);
    }
    if (q.having.active) {
      nh = (int)wave_sum(nh);
      nhc = (int)wave_sum(nhc);
      if (lane == 0 && nh) atomicAdd(&hnew[p], (unsigned long long)nh);
      if (lane == 0 && nhc) atomicAdd(hclosed, (unsigned long long)nhc);
    }
    lds_barrier();
    C1M_T(4);
    if (threadIdx.x == 0) nnew = 0;
    lds_barrier();
  }
}

// ------------------------------------------------------------------ host side

size_t c1_merge_lds(int log2H, int idw, int log2B) {
  const size_t H = (size_t)1 << log2H, B = (size_t)1 << log2B;
  return (H + 64) * (idw + 8) + ((H * 2 + 15) & ~(size_t)15) + (C1_SEGMAX + 4) * 8 + (B + 1) * 12 + 8 +
         C1_SEGOF * 2;  // (segment table: 8 B per entry, both layouts fit)
}

// Whether the COUNT(*) pipeline may take this push (the general path's c1 plan, TUMBLING, the
// two-level partition layout).  The push may still be declined on the device (k_c1_check).
bool c1_eligible(khip_agg* a, int64_t n) {
  PartState& s = a->part;
  const bool cnt1 = a->ap.n_ops == 1 && a->ap.ops[0].kind == OP_INC && a->ap.ops[0].word == 3 && a->sw == 4 &&
                    s.rw == 2;
  return cnt1 && a->windowed && a->desc.window_kind == KHIP_WINDOW_TUMBLING && s.log2P >= 11 && s.log2P <= 16 &&
         s.mH >= 256 && a->desc.advance_ms <= ((int64_t)1 << 31) && !(a->desc.flags & KHIP_FLAG_PART_CLAIM) &&
         n > 0 && n < ((int64_t)1 << 31) && knob("KHIP_C1P", 1) != 0 && knob("KHIP_PAD", 0) == 0 &&
         knob("KHIP_MERGE", 1) != 0 && knob("KHIP_SCATTER2", 1) != 0;
}

// The value pipeline: every update op reads one argument column (or is COUNT(*)), at most one op
// per kind, TUMBLING or HOPPING with size a multiple of the advance (panes), rows of <= 8 words.
// *col = the argument column.
bool c1v_eligible(khip_agg* a, int64_t n, int* col) {
  PartState& s = a->part;
  if (!a->windowed || a->sw > C1V_MAXW || a->ap.n_ops < 1 || s.rw < 2) return false;
  const int64_t size = a->desc.size_ms, adv = a->desc.advance_ms;
  if (a->desc.window_kind == KHIP_WINDOW_HOPPING) {
    if (size % adv != 0 || size / adv > 16) return false;
  } else if (a->desc.window_kind != KHIP_WINDOW_TUMBLING) {
    return false;
  }
  int c = -1, seen = 0;
  for (int o = 0; o < a->ap.n_ops; o++) {
    const UpdOp op = a->ap.ops[o];
    if (op.kind < OP_INC || op.kind > OP_MAX || op.word < 3 || op.word >= a->sw) return false;
    const int bit = op.kind == OP_ADD_F64 ? (1 << OP_ADD_I64) : (1 << op.kind);
    if (seen & bit) return false;
    seen |= bit;
    if (op.kind == OP_INC) continue;
    if (c >= 0 && op.col != c) return false;
    c = op.col;
  }
  if (c < 0) return false;  // COUNT(*) alone: the COUNT(*) pipeline's
  const int t = a->ap.col_type[c];
  if (t != KHIP_TYPE_INT32 && t != KHIP_TYPE_INT64 && t != KHIP_TYPE_DOUBLE) return false;
  *col = c;
  return s.log2P >= 11 && s.log2P <= 16 && s.mH >= 256 && adv <= ((int64_t)1 << 31) &&
         !(a->desc.flags & KHIP_FLAG_PART_CLAIM) && n > 0 && n < ((int64_t)1 << 31) && knob("KHIP_C1V", 1) != 0 &&
         knob("KHIP_PAD", 0) == 0 && knob("KHIP_MERGE", 1) != 0 && knob("KHIP_SCATTER2", 1) != 0;
}

// Dynamic LDS of a value merge that still fits two workgroups per CU (160 KB, less the kernel's
// static LDS).
constexpr size_t C1V_LDS2 = 80 * 1024 - 256;

// LDS layout of k_c1v_merge (byte offsets into q); returns the bytes.
static size_t c1v_layout(khip_agg* a, int log2H, int idw, int log2B, C1VQ* q) {
  const size_t E = ((size_t)1 << log2H) + 64, H = (size_t)1 << log2H, B = (size_t)1 << log2B;
  size_t off = E * idw;
  off = (off + 7) & ~(size_t)7;
  q->off_sum = q->off_min = q->off_max = q->off_star = q->off_cnt = -1;
  for (int o = 0; o < a->ap.n_ops; o++) {
    const int k = a->ap.ops[o].kind;
    if (k == OP_ADD_I64 || k == OP_ADD_F64) q->off_sum = 1;
    if (k == OP_MIN) q->off_min = 1;
    if (k == OP_MAX) q->off_max = 1;
    if (k == OP_INC) q->off_star = 1;
    if (k == OP_INC_VALID) q->off_cnt = 1;
  }
  auto place = [&](int32_t* f, size_t bytes) {
    if (*f < 0) return;
    *f = (int32_t)off;
    off += E * bytes;
  };
  place(&q->off_sum, 8);
  place(&q->off_min, 8);
  place(&q->off_max, 8);
  q->off_rt = (int32_t)off;
  off += E * 4;
  place(&q->off_star, 4);
  place(&q->off_cnt, 4);
  off = (off + 15) & ~(size_t)15;
  q->off_list = (int32_t)off;
  off += (H * 2 + 15) & ~(size_t)15;
  q->off_spre = (int32_t)off;
  off += (C1_SEGMAX + 4) * 8 + C1_SEGOF * 2;
  (void)B;
  return off;
}

constexpr int C1V_UV = 4;  // value scatter: records per thread per step

// One attempt's geometry and scratch pointers (c1_prepare), handed to every stage.
struct C1Geo {
  bool val, panes, wide;  // value pipeline; its HOPPING panes; wide records (COUNT(*) only)
  int P, CH, fbits, log2B, B, F;
  int64_t n, nT, S, nSt, nchunk_max;  // records, tiles, scatter step (records), steps, refine chunks at most
  size_t seg_bytes;
  int64_t* ci;
  int* cstart;
  uint16_t* seg;
  uint32_t *srecAT, *srecT;  // the WIDE records' ts words (12 B/record in all)
  int sh;             // log2 of the steps per tile
  uint32_t *tt, *tb;  // run positions: [bucket][tile] totals, [bucket][tile + 1] bases (k_c1_runpos)
  uint16_t *rl, *ro;  // [bucket][step]: the run's place within its tile, the bucket's offset in the step's run
  int64_t adv, close0;
  FastDiv fd;
};

// The merges' parameters and table sizes.
struct C1Merge {
  C1Q cq;
  C1VQ vq0;
  int log2H, v_log2H;
  int v_pm;   // the plane mask when a specialised value merge exists for it
  int v_wpc;  // value merge workgroups per CU
};

// What follows an attempt k_c1_check declined.
enum C1Next { C1_DONE, C1_DECLINED, C1_AGAIN_KBASE, C1_AGAIN_WIDE };

// Geometry, scratch sizing and the c1info block's first initialisation.
static khip_status c1_prepare(khip_agg* a, int64_t n, const C1In& in, C1Geo* g) {
  PartState& s = a->part;
  g->val = in.cols != nullptr || in.rows != nullptr;
  g->panes = g->val && a->desc.window_kind == KHIP_WINDOW_HOPPING;
  g->CH = g->val ? C1V_CH : C1_CH;
  g->P = (int)s.P;
  g->fbits = s.log2P - s.log2P / 2;
  g->log2B = s.log2P - g->fbits;
  g->B = 1 << g->log2B;
  g->F = 1 << g->fbits;
  g->n = n;
  g->nT = ceil_div(n, C1_TILE);
  g->S = g->val ? (int64_t)C1V_UV * C1_NT : (int64_t)8 * C1_NT;
  g->nSt = g->nT * (C1_TILE / g->S);  // (runs per bucket)
  g->nchunk_max = ceil_div(n, g->CH) + g->B;
  const int64_t B = g->B, nSt = g->nSt, nT = g->nT;
  static_assert(C1_TILE / (C1V_UV * C1_NT) == 32 && C1_TILE / (8 * C1_NT) == 16, "steps per tile");
  g->sh = g->val ? 5 : 4;
  KHIP_TRY(s.c1rc.ensure((size_t)B * nT * 4));
  KHIP_TRY(s.c1rp.ensure((size_t)B * (nT + 1) * 4));
  KHIP_TRY(s.c1rl.ensure((size_t)B * nSt * 2));
  KHIP_TRY(s.c1ro.ensure((size_t)B * nSt * 2));
  KHIP_TRY(s.c1bb.ensure((size_t)(B + 1) * 8));
  g->seg_bytes = ((size_t)g->nchunk_max * (g->F + 1) * 2 + 255) & ~(size_t)255;  // cstart 256-B aligned
  KHIP_TRY(s.c1seg.ensure(g->seg_bytes + (size_t)(B + 1) * 4));
  KHIP_TRY(s.tilemax.ensure(nT * 32));  // per tile: stream-time max, smallest ts, late bound, ok
  KHIP_TRY(s.tpart.ensure(nT * 8 * T_NPART));
  KHIP_TRY(s.prn.ensure((size_t)g->P * 4));
  KHIP_TRY(s.res.ensure(16));
  KHIP_TRY(s.closed_ctr.ensure(8));
  if (s.scat_cap < n) {
    KHIP_TRY(s.srec.ensure((size_t)(n + 1) * s.rw * 8));
    s.scat_cap = n;
  }
  KHIP_TRY(s.srec.ensure((size_t)(n + 1) * 16));  // (s.rw >= 2: no-ops)
  KHIP_TRY(s.srecA.ensure((size_t)(n + 1) * std::max(s.rw, 2) * 8));
  g->ci = s.ctr.as<int64_t>() + CTR_ALLOC;  // the c1info block lies behind the counters (part_init)
#ifdef KHIP_TUNING
  {
    const int64_t dbg = knob("KHIP_C1_DEBUG", 0);
    KHIP_TRY_HIP(hipMemcpyAsync(g->ci + CI_N - 1, &dbg, 8, hipMemcpyHostToDevice, a->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
  }
#endif
  g->cstart = (int*)(s.c1seg.as<char>() + g->seg_bytes);
  g->seg = s.c1seg.as<uint16_t>();
  g->adv = a->desc.advance_ms;
  g->fd = make_fastdiv(g->adv);
  g->close0 = a->host_stream_time >= 0 ? a->host_stream_time - a->grace : INT64_MIN;
  // wide records (key hash + u32 ts words) when the key range did not fit 32 bits last time: the
  // host predicts the format, k_c1_check declines a compact push whose keys do not fit
  g->wide = !g->val && s.c1_wide;
  g->srecAT = (uint32_t*)(s.srecA.as<uint64_t>() + n + 1);
  g->srecT = (uint32_t*)(s.srec.as<uint64_t>() + n + 1);
  g->tt = s.c1rc.as<uint32_t>();
  g->tb = s.c1rp.as<uint32_t>();
  g->rl = s.c1rl.as<uint16_t>();
  g->ro = s.c1ro.as<uint16_t>();
  return KHIP_OK;
}

// 1. records → step runs (the key range, time base and bucket counts in the same read)
// 2. each tile's base in its buckets and the buckets' totals (k_c1_runpos)
static khip_status c1_scatter(khip_agg* a, const C1In& in, const C1Geo& g) {
  PartState& s = a->part;
  ev_record_part(a, 0);
  const int has_kb = s.c1_kb_valid ? 1 : 0;
  const int64_t* st_at = in.st_at;
  if (g.val) {
    constexpr int UV = C1V_UV;
    const RowsIn* rows = in.rows;
    const C1VCol vc{rows ? nullptr : in.cols->data[in.vcol], rows ? nullptr : in.cols->valid[in.vcol],
                    a->ap.col_type[in.vcol]};
    const RowsIn ri = rows ? *rows : RowsIn{};
    auto sk = rows ? (st_at ? k_c1v_scatter<UV, C1_NT, true, true> : k_c1v_scatter<UV, C1_NT, false, true>)
                   : (st_at ? k_c1v_scatter<UV, C1_NT, true, false> : k_c1v_scatter<UV, C1_NT, false, false>);
    const size_t lds = run_stage_lds(g.B, UV * C1_NT, 16, false) + run_cnt_lds(g.B, C1_TILE / (UV * C1_NT));
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)sk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(sk, dim3(g.nT), dim3(C1_NT), lds, a->stream, in.keys, in.ts, in.kv, in.rv, vc, ri, g.n, g.nT,
                       g.log2B, g.rl, g.ro, g.tt, (ulonglong2*)s.srecA.p, s.tilemax.as<int64_t>(),
                       s.tpart.as<int64_t>(), g.ci, st_at, a->desc.size_ms, g.adv, g.fd,
                       a->desc.size_ms != g.adv ? 1 : 0, a->grace, (const int64_t*)a->stream_time.as<int64_t>(),
                       s.c1_kbase, has_kb);
  } else {
    constexpr int U = 8;
    auto sk = g.wide ? (st_at ? k_c1_scatter<U, C1_NT, true, true> : k_c1_scatter<U, C1_NT, true, false>)
                     : (st_at ? k_c1_scatter<U, C1_NT, false, true> : k_c1_scatter<U, C1_NT, false, false>);
    const size_t lds = run_stage_lds(g.B, U * C1_NT, 8, g.wide) + run_cnt_lds(g.B, C1_TILE / (U * C1_NT));
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)sk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(sk, dim3(g.nT), dim3(C1_NT), lds, a->stream, in.keys, in.ts, in.kv, in.rv, g.n, g.nT, g.log2B,
                       g.rl, g.ro, g.tt, s.srecA.as<uint64_t>(), s.tilemax.as<int64_t>(), s.tpart.as<int64_t>(), g.ci,
                       st_at, g.srecAT, a->desc.size_ms, g.adv, g.fd, a->grace,
                       (const int64_t*)a->stream_time.as<int64_t>(), s.c1_kbase, has_kb);
  }
  KHIP_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_c1_runpos, dim3(g.B), dim3(1024), 0, a->stream, (const uint32_t*)g.tt, g.nT, g.tb);
  KHIP_TRY_HIP(hipGetLastError());
  ev_record_part(a, 1);
  return KHIP_OK;
}

// 5b. chunks → partition-sorted records and the segment table
static khip_status c1_refine(khip_agg* a, const C1Geo& g) {
  PartState& s = a->part;
  if (g.val) {
    auto rk = k_c1v_refine<C1V_CH / C1_NT, C1_NT>;
    const size_t lds = (((size_t)g.F * 8 + 15) & ~(size_t)15) + (size_t)C1V_CH * 16;
    hipFuncSetAttribute((const void*)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(rk, dim3((unsigned)g.nchunk_max), dim3(C1_NT), lds, a->stream, (const ulonglong2*)s.srecA.p,
                       s.c1bb.as<int64_t>(), g.cstart, g.log2B, s.log2P, g.fbits, (ulonglong2*)s.srec.p, g.seg, g.ci,
                       (const uint32_t*)g.tb, (const uint16_t*)g.rl, (const uint16_t*)g.ro, g.nT, g.sh, g.S,
                       (const uint32_t*)s.c1ci.as<uint32_t>());
  } else {
    constexpr int U = C1_CH / C1_NT;
    auto rk = g.wide ? k_c1_refine<U, C1_NT, true> : k_c1_refine<U, C1_NT, false>;
    const size_t lds = (size_t)g.F * 8 + (size_t)C1_CH * 8;
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(rk, dim3((unsigned)g.nchunk_max), dim3(C1_NT), lds, a->stream, s.srecA.as<uint64_t>(),
                       s.c1bb.as<int64_t>(), g.cstart, g.log2B, s.log2P, g.fbits, s.srec.as<uint64_t>(), g.seg, g.ci,
                       (const uint32_t*)g.srecAT, g.srecT, (const uint32_t*)g.tb, (const uint16_t*)g.rl,
                       (const uint16_t*)g.ro, g.nT, g.sh, g.S, (const uint32_t*)s.c1ci.as<uint32_t>());
  }
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

// The record stages: scatter, run positions, check, chunks, refine.
static khip_status c1_records(khip_agg* a, const C1In& in, const C1Geo& g) {
  PartState& s = a->part;
  KHIP_TRY(c1_scatter(a, in, g));
  // 4. accept or decline (and the bucket bases, the push's statistics)
  hipLaunchKernelGGL(k_c1_check, dim3(1), dim3(1024), 0, a->stream, s.tilemax.as<int64_t>(),
                     (const int64_t*)s.tpart.as<int64_t>(), g.nT, a->desc.size_ms, g.adv, g.fd, a->grace, g.close0,
                     s.res_fresh ? 1 : 0, g.log2B, s.log2P, g.wide ? 1 : 0, g.CH, g.val ? 31 : 32, g.panes ? 1 : 0,
                     (const uint32_t*)g.tb, s.c1bb.as<int64_t>(), g.cstart, g.ci, a->stream_time.as<int64_t>(),
                     s.res.as<int64_t>(), s.ctr.as<unsigned long long>(), s.closed_ctr.as<unsigned long long>(),
                     (unsigned long long)s.closed_n);
  // 5. refine: each chunk's step runs (k_c1_chunks), chunks → partition-sorted, segment table
  KHIP_TRY(s.c1ci.ensure((size_t)g.nchunk_max * 8));
  hipLaunchKernelGGL(k_c1_chunks, dim3((unsigned)ceil_div(g.nchunk_max, 256)), dim3(256), 0, a->stream,
                     (const int*)g.cstart, g.B, (const uint32_t*)g.tb, (const uint16_t*)g.rl, g.nT, g.sh, g.CH,
                     (const int64_t*)g.ci, s.c1ci.as<uint32_t>());
  KHIP_TRY(c1_refine(a, g));
  ev_record_part(a, 2);
  return KHIP_OK;
}

// The COUNT(*) merge's parameters.
static C1Q c1_make_q(khip_agg* a, const C1Geo& g, int log2H) {
  C1Q cq{};
  cq.log2P = a->part.log2P;
  cq.fbits = g.fbits;
  cq.log2H = log2H;
  cq.sw = a->sw;
  cq.hv_active = a->having.active;
  cq.hv_op = a->having.op;
  cq.hv_i64 = a->having.i64;
  cq.hmax = (int)((int64_t)(1 << log2H) * 3 / 4);
  cq.size = a->desc.size_ms;
  cq.adv = g.adv;
  cq.fd = g.fd;
  cq.fd32 = make_fastdiv32((uint32_t)g.adv);
  return cq;
}

// The value merge's parameters: the largest table (up to 2^12 entries) whose LDS lets two
// workgroups share a CU, and the plane mask when a specialised merge exists for it.
static void c1v_make_q(khip_agg* a, const C1Geo& g, int vcol, C1Merge* m) {
  C1VQ& vq0 = m->vq0;
  // sized for 32-bit identities (the common case); 64-bit ones (a key range past 31 - window
  // bits) run at one workgroup per CU when their table does not fit two
  m->v_log2H = 12;
  while (m->v_log2H > 9 && c1v_layout(a, m->v_log2H, 4, g.log2B, &vq0) > C1V_LDS2) m->v_log2H--;
  m->v_log2H = (int)knob("KHIP_C1V_LOG2H", m->v_log2H);

  vq0.log2P = a->part.log2P;
  vq0.fbits = g.fbits;
  vq0.log2H = m->v_log2H;
  vq0.sw = a->sw;
  vq0.hmax = (int)((int64_t)(1 << m->v_log2H) * 3 / 4);
  vq0.fan = (int)(a->desc.size_ms / g.adv);
  vq0.f64 = 0;
  for (int k = 0; k < C1V_MAXW; k++) {
    vq0.word_op[k] = -1;
    vq0.init[k] = (uint64_t)a->init.w[k];
  }
  for (int o = 0; o < a->ap.n_ops; o++) {
    vq0.word_op[a->ap.ops[o].word] = a->ap.ops[o].kind;
    if (a->ap.ops[o].kind == OP_ADD_F64) vq0.f64 = 1;
  }
  if (a->ap.col_type[vcol] == KHIP_TYPE_DOUBLE) vq0.f64 = 1;
  int pm = 0;
  for (int o = 0; o < a->ap.n_ops; o++) {
    const int k = a->ap.ops[o].kind;
    pm |= k == OP_INC ? PM_STAR : k == OP_INC_VALID ? PM_CNT : k == OP_MIN ? PM_MIN : k == OP_MAX ? PM_MAX : PM_SUM;
  }
  pm |= PM_SPEC | (vq0.f64 ? PM_F64 : 0);
  m->v_pm = ((pm != PM_C5 && pm != PM_C3) || knob("KHIP_C1V_SPEC", 1) == 0) ? 0 : pm;
  vq0.size = a->desc.size_ms;
  vq0.adv = g.adv;
  vq0.fd = g.fd;
  vq0.fd32 = make_fastdiv32((uint32_t)g.adv);
  vq0.having = a->having;
}

// One pass's merge over the nwork items of wk (null: one per partition).  Compact records: both
// identity widths are launched, the one k_c1_check did not choose exits at once; wide records:
// 64-bit identities.
static khip_status c1_launch_merge(khip_agg* a, const C1Geo& g, const C1Merge& m, int pass, const uint32_t* wk,
                                   int64_t nwork, unsigned long long* dbg) {
  PartState& s = a->part;
  unsigned long long* ctr = s.ctr.as<unsigned long long>();
  uint8_t* chg = a->changelog ? a->chg.as<uint8_t>() : nullptr;  // (a retry's regrow moves it)
  for (int idw = g.wide ? 1 : 0; idw < 2 && g.val; idw++) {
    C1VQ vq = m.vq0;
    const size_t lds = c1v_layout(a, m.v_log2H, idw == 0 ? 4 : 8, g.log2B, &vq);
    vq.cmax = s.cmax;
    vq.chg = chg;
    // the benchmarks' plane shapes have instantiations of their own (PM_C5, PM_C3), every other
    // one reads the planes from the parameters; AU 2 at <= 128 VGPRs (two workgroups per CU)
    auto pick = [&](auto pmc) {
      constexpr int PMv = decltype(pmc)::value;
      return g.panes ? (idw == 0 ? k_c1v_merge<512, 2, uint32_t, true, 4, PMv> : k_c1v_merge<512, 2, uint64_t, true, 4, PMv>)
                     : (idw == 0 ? k_c1v_merge<512, 2, uint32_t, false, 4, PMv> : k_c1v_merge<512, 2, uint64_t, false, 4, PMv>);
    };
    auto mk = m.v_pm == PM_C5 ? pick(std::integral_constant<int, PM_C5>{})
                              : (m.v_pm == PM_C3 ? pick(std::integral_constant<int, PM_C3>{}) : pick(std::integral_constant<int, 0>{}));
    hipFuncSetAttribute((const void*)mk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    KHIP_TRY(s.c1vq.ensure(sizeof(C1VQ)));
    KHIP_TRY(s.c1vq_h.ensure(2 * sizeof(C1VQ)));
    C1VQ* hq = (C1VQ*)s.c1vq_h.p + idw;
    *hq = vq;
    KHIP_TRY_HIP(hipMemcpyAsync(s.c1vq.p, hq, sizeof(C1VQ), hipMemcpyHostToDevice, a->stream));
    const int64_t vgrid = std::min<int64_t>(nwork, (int64_t)s.n_cu * (lds <= C1V_LDS2 ? m.v_wpc : 1));
    hipLaunchKernelGGL(mk, dim3(vgrid), dim3(512), lds, a->stream, s.c1vq.as<C1VQ>(), wk, nwork, s.c1bb.as<int64_t>(),
                       g.cstart, g.seg, (const ulonglong2*)s.srec.p, pass == 0 ? 1 : 0, s.buf[0].as<uint64_t>(),
                       s.buf[1].as<uint64_t>(), s.sel.as<uint8_t>(), s.cnt.as<int64_t>(),
                       s.newcnt.as<unsigned long long>(), s.fail.as<uint8_t>(), ctr + CTR_NEED, g.close0,
                       s.closed.as<uint64_t>(), s.closed_ctr.as<unsigned long long>(),
                       (unsigned long long)s.closed_cap, g.ci, s.hnew.as<unsigned long long>(), ctr + CTR_HAVING_CLOSED,
                       s.prn.as<uint32_t>(), dbg);
  }
  C1Q cq = m.cq;
  cq.cmax = s.cmax;
  cq.chg = chg;
  const int64_t grid = std::min<int64_t>(nwork, (int64_t)s.n_cu * knob("KHIP_MERGE_WG_PER_CU", 2));
  for (int idw = g.wide ? 1 : 0; idw < 2 && !g.val; idw++) {
    auto mk = g.wide ? k_c1_merge<512, 3, uint64_t, true>
                     : (idw == 0 ? k_c1_merge<512, 4, uint32_t, false> : k_c1_merge<512, 4, uint64_t, false>);
    const size_t lds = c1_merge_lds(m.log2H, idw == 0 ? 4 : 8, g.log2B);
    hipFuncSetAttribute((const void*)mk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(mk, dim3(grid), dim3(512), lds, a->stream, cq, wk, nwork, s.c1bb.as<int64_t>(), g.cstart, g.seg,
                       s.srec.as<uint64_t>(), pass == 0 ? 1 : 0, s.buf[0].as<uint64_t>(), s.buf[1].as<uint64_t>(),
                       s.sel.as<uint8_t>(), s.cnt.as<int64_t>(), s.newcnt.as<unsigned long long>(),
                       s.fail.as<uint8_t>(), ctr + CTR_NEED, g.close0, s.closed.as<uint64_t>(),
                       s.closed_ctr.as<unsigned long long>(), (unsigned long long)s.closed_cap, g.ci,
                       s.hnew.as<unsigned long long>(), ctr + CTR_HAVING_CLOSED, s.prn.as<uint32_t>(),
                       (const uint32_t*)g.srecT, dbg);
  }
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

// A declined attempt (hci: the c1info copy; nothing persistent was written): decline the push, or
// run it again with the keys' true base (once per record format) or with the wide records.
static khip_status c1_declined_next(khip_agg* a, const C1In& in, const C1Geo& g, bool kretried, C1Next* next) {
  PartState& s = a->part;
  const int64_t* hci = s.info()->c1info;
  bool go_wide = !g.val && hci[CI_REASON] == 1;  // only the record format was wrong
  if (hci[CI_REASON] == 2 && !kretried) {  // a key outside the field above kb: the true range
    long long kr[2] = {INT64_MIN, INT64_MIN};
    KHIP_TRY(s.c1kr.ensure(16));
    KHIP_TRY_HIP(hipMemcpyAsync(s.c1kr.p, kr, 16, hipMemcpyHostToDevice, a->stream));
    hipLaunchKernelGGL(k_c1_krange, dim3((unsigned)std::min<int64_t>(ceil_div(g.n, 256), 2048)), dim3(256), 0,
                       a->stream, in.rows ? (const int64_t*)in.rows->rows : in.keys,
                       in.rows ? (int64_t)in.rows->rw : 1, g.n, s.c1kr.as<long long>());
    KHIP_TRY_HIP(hipMemcpyAsync(kr, s.c1kr.p, 16, hipMemcpyDeviceToHost, a->stream));
    KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
    const int64_t kmin = (int64_t)~(uint64_t)kr[0], kmax = (int64_t)kr[1];
    if ((uint64_t)kmax - (uint64_t)kmin < (1ULL << (g.val ? 31 : 32)) - 1) {  // again with kb = kmin
      s.c1_kbase = kmin;
      s.c1_kb_valid = true;
      *next = C1_AGAIN_KBASE;
      return KHIP_OK;
    }
    go_wide = !g.val;  // the range itself is past the compact records
  }
  if (go_wide) s.c1_wide = true;
  *next = go_wide ? C1_AGAIN_WIDE : C1_DECLINED;
  return KHIP_OK;
}

// Sub-passes per partition: the pipeline's own LDS table (hmax), not the general merge's — a
// partition starts with enough of them for the hinted groups, and keeps those a push needed.
static void c1_start_bits(PartState& s, int64_t hm) {
  if ((int64_t)s.c1psbits.size() == s.P && s.c1ps_hmax == hm) return;
  int s0 = 0;
  while (s0 < RETRY_MAX_SBITS && s.hint_groups / s.P > (hm * 7 / 10) << s0) s0++;
  s.c1psbits.assign(s.P, (uint8_t)s0);
  s.c1ps_hmax = hm;
}

// *declined = true when k_c1_check declined the push (nothing persistent was touched: the caller
// runs the general path on the same batch).  A declined attempt may be followed by one with the
// keys' true base, and (COUNT(*)) by one with wide records, which again may change its key base.
khip_status c1_push(khip_agg* a, int64_t n, const C1In& in, int64_t* tot, bool* declined) {
  PartState& s = a->part;
  *declined = false;
  const bool probe = knob("KHIP_AGG_PROBE", 0) != 0;
  bool kretried = false, wide_tried = false;
  for (;;) {  // attempts (at most four)
    C1Geo g;
    KHIP_TRY(c1_prepare(a, n, in, &g));
    KHIP_TRY(part_grow_closed(a));
    KHIP_TRY(c1_records(a, in, g));
    // 6. merge partitions (+ retries: DESIGN.md (d))
    C1Merge m{};
    m.log2H = (int)knob("KHIP_C1_LOG2H", 12);
    m.cq = c1_make_q(a, g, m.log2H);
    m.v_wpc = (int)knob("KHIP_C1V_WG_PER_CU", 2);
    if (g.val) c1v_make_q(a, g, in.vcol, &m);
    c1_start_bits(s, g.val ? m.vq0.hmax : m.cq.hmax);
    RetryPlan r;
    retry_begin(r, s.c1psbits);
    const bool subs0 = !r.work.empty();
    if (subs0) KHIP_TRY(part_upload_plan(a, r.image));
    std::vector<uint8_t> host_fail;
    DevBuf dbgbuf;
    if (probe) {
      KHIP_TRY(dbgbuf.ensure(64));
      KHIP_TRY_HIP(hipMemsetAsync(dbgbuf.p, 0, 64, a->stream));
    }
    PushInfo* pi = s.info();
    const unsigned long long* c2 = pi->ctr;
    int64_t added_total = 0;
    C1Next next = C1_DONE;
    for (int pass = 0;; pass++) {
      unsigned long long* dbg = probe && pass == 0 ? dbgbuf.as<unsigned long long>() : nullptr;
      if (pass > 0) KHIP_TRY_HIP(hipMemsetAsync(s.ctr.p, 0, CTR_PER_PASS * 8, a->stream));
      const uint32_t* wk = (pass == 0 && !subs0) ? nullptr : s.work.as<uint32_t>();
      const int64_t nwork = wk ? (int64_t)r.work.size() : g.P;
      KHIP_TRY(c1_launch_merge(a, g, m, pass, wk, nwork, dbg));
      // one copy back per pass: the counters (with them the closed store's rows after this pass,
      // CTR_CLOSED: closed rows leave in the pass that writes their item) and, on pass 0, the c1info
      // block behind them
      KHIP_TRY(part_pass_commit(a, pass, r, pass == 0 ? (const int64_t*)g.ci : (const int64_t*)nullptr,
                                s.prn.as<uint32_t>(), s.closed_ctr.as<unsigned long long>(), g.nT, true));
      KHIP_TRY_HIP(hipStreamSynchronize(a->stream));
      if (pass == 0 && pi->c1info[CI_GATE] == 0) {  // declined: nothing was written
        KHIP_TRY(c1_declined_next(a, in, g, kretried, &next));
        break;
      }
      if (pass == 0 && g.wide && ++s.c1_wide_n % 64 == 0) s.c1_wide = false;  // now and then: compact records again?
      if (pass == 0 && !g.wide) {  // the next push's key base: this one's minimum, less a margin for keys below it
        const int64_t km = pi->c1info[CI_KMINC], slack = (int64_t)1 << (g.val ? 26 : 28);
        s.c1_kbase = km >= INT64_MIN + slack ? km - slack : km;
        s.c1_kb_valid = true;
      }
      if (dbg) {
        unsigned long long ph[8] = {};
        if (hipMemcpy(ph, dbgbuf.p, sizeof(ph), hipMemcpyDeviceToHost) == hipSuccess) {
          const double us = (double)std::min<int64_t>(g.P, 2 * s.n_cu) * 100.0;  // 100 MHz ticks → us per workgroup
          fprintf(stderr, "[%s merge probe] per workgroup (us): start+evict %.1f records %.1f fold %.1f "
                  "mark+count+reserve %.1f write %.1f\n", g.val ? "c1v" : "c1", ph[0] / us, ph[1] / us, ph[2] / us,
                  ph[3] / us, ph[4] / us);
        }
      }
      if (c2[CTR_NEED] & C1_FATAL)  // (cannot happen: the store holds every live row)
        return fail(KHIP_E_DEVICE, "the closed store's capacity would be exceeded by a merge's closed rows");
      added_total += (int64_t)c2[CTR_ADDED];
      KHIP_TRY(part_pass_failed(a, &host_fail));
#ifdef KHIP_TUNING
      if (knob("KHIP_C1_TRACE", 0) != 0) {  // one line per pass: the tests' witness that a push was retried
        int64_t nsub, ft, fr;
        part_retry_trace_counts(r, wk != nullptr, host_fail, &nsub, &ft, &fr);
        fprintf(stderr,
                "[c1 trace] val=%d P=%d cmax=%lld log2H=%d pass=%d items=%lld sub_items=%lld failed=%llu fail_table=%lld "
                "fail_region=%lld closed_before=%lld closed_after=%llu\n",
                g.val ? 1 : 0, g.P, (long long)s.cmax, g.val ? m.v_log2H : m.log2H, pass, (long long)nwork,
                (long long)nsub, c2[CTR_FAILED], (long long)ft, (long long)fr, (long long)s.closed_n, c2[CTR_CLOSED]);
      }
#endif
      if (c2[CTR_FAILED] == 0) break;
      KHIP_TRY(part_plan_retry(a, r, pass, host_fail));
    }
    if (next == C1_AGAIN_KBASE) {
      kretried = true;
      continue;
    }
    if (next == C1_AGAIN_WIDE && !wide_tried) {  // the keys needed the wide records: this push again with them
      wide_tried = true;
      kretried = false;
      continue;
    }
    if (next != C1_DONE) {
      *declined = true;
      return KHIP_OK;
    }
    retry_learn(s.c1psbits, r);
    s.res_fresh = false;
    s.last_c1 = true;
    // the closed store's rows after every pass (k_part_commit refreshes CTR_CLOSED on each)
    part_push_epilogue(a, (int64_t)c2[CTR_CLOSED], added_total, tot);
    return KHIP_OK;
  }
}

}  // namespace khip
