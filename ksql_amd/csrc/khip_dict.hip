// khip_dict.hip — the device dictionary of serialized STRING keys (khip_dict.hpp): its kernels and
// the KeyDict host functions.  Used by the aggregate's UTF8 GROUP BY keys (khip_agg.hip), the table
// aggregation's PRIMARY KEYs (khip_agg_table.hip) and the join's STRING-keyed tables (khip_join.hip).
#include <algorithm>

#include "khip_util.hpp"

#include "khip_agg_internal.hpp"

namespace khip {

// ------------------------------------------------------------------- kernels
// Slot (32 B, one random access): w0 dict word: 0 empty | fresh: bit63 | fp22 << 40 | batch row
// (40 bits) | resident: bit62 | fp22 << 40 | o / 8 (40 bits); w1 = o | min(len, 0xFFFF) << 48 (the
// key's id = its arena offset o, and its length); w2, w3 = the key's first 16 bytes as words
// (keys of up to 16 bytes compare there; longer ones against the arena entry).  Arena entry at o
// (8-aligned): [u64 hash][i64 len][bytes, padded to 8].  A map is three passes, none over the
// whole table:
//   k_dict_probe    per row: hash, probe; a resident slot compares in place; an empty slot is
//                   claimed (fresh word naming the row; the slot and its arena entry's place go to
//                   one of DICT_NL claim lists, one block-aggregated append); a fresh slot of the same fingerprint, claimed by
//                   another row of this batch, leaves the row PENDING on it
//   k_dict_commit   per claim: the arena entry (its list's base + its place in the list), the slot
//                   made resident with the key's words, the claiming row's id (no atomics)
//   k_dict_resolve  per pending row: the (now resident) slot compares; a different key of the same
//                   fingerprint goes on a retry list (probed again: the slot no longer misleads it)
// A probe gives up after DICT_PROBE slots (the table is then too full: dict_map unclaims the
// batch's fresh words, grows the table and maps the batch again).
constexpr int DICT_PROBE = 256;
constexpr uint64_t DICT_LOW = (1ULL << 40) - 1;
constexpr int DICT_NL = 1024;  // claim lists (one per block residue: no hot append word)
constexpr int64_t KID_PEND = (int64_t)1 << 62;
constexpr uint64_t DICT_ID = (1ULL << 48) - 1;

__device__ __forceinline__ int64_t entry_bytes(int64_t len) { return 16 + ((len + 7) & ~7LL); }

#ifdef KHIP_TUNING
// Tuning build: KHIP_DICT_HASHMASK keeps only these bits of every key hash (different keys then
// share whole hashes, not just fingerprints: tests/test_gpu_dict.py); KHIP_KEY_INLINE=0 sends the
// digit keys through the dictionary too.
__constant__ uint64_t g_dict_hmask = ~0ULL;
__constant__ int g_key_inline = 1;
#endif

// The key of batch row i: words (short keys), hash.
struct DKey {
  uint64_t kw[KW_MAX];
  uint64_t h;
  int64_t len;
  const uint8_t* kb;
  bool sk;
};
__device__ __forceinline__ void dkey_words(DKey& k, const int64_t* __restrict__ koff, const uint8_t* __restrict__ kbytes,
                                           int64_t i) {
  const int64_t o0 = koff[i];
  k.len = koff[i + 1] - o0;
  k.kb = kbytes + o0;
  k.sk = k.len <= 8 * KW_MAX;
  if (k.sk) key_words(k.kb, k.len, k.kw);
}
__device__ __forceinline__ void dkey_hash(DKey& k) {
  k.h = k.sk ? hash_key_words(k.kw, k.len) : hash_bytes_dev(k.kb, k.len);
#ifdef KHIP_TUNING
  k.h &= g_dict_hmask;
#endif
}
__device__ __forceinline__ void dkey_load(DKey& k, const int64_t* __restrict__ koff, const uint8_t* __restrict__ kbytes,
                                          int64_t i) {
  dkey_words(k, koff, kbytes, i);
  dkey_hash(k);
}

// Key k's inline id (khip_dict.hpp), when it is 0..17 ASCII digits.
__device__ __forceinline__ bool key_inline(const DKey& k, int64_t* code) {
#ifdef KHIP_TUNING
  if (!g_key_inline) return false;
#endif
  static_assert(KW_MAX == 3, "inline keys are read from three key words");
  return k.sk && inline_id_words(k.kw, k.len, code);
}

// A resident slot (w0 fingerprint already matched) holds key k?
__device__ __forceinline__ bool dslot_eq(const ulonglong2& a, const ulonglong2& b, const DKey& k,
                                         const uint8_t* __restrict__ arena) {
  const int64_t slen = (int64_t)(a.y >> 48);
  if (k.len <= 16) return slen == k.len && b.x == k.kw[0] && b.y == (k.len > 8 ? k.kw[1] : 0ULL);
  if (slen != (k.len < 0xFFFF ? k.len : 0xFFFF)) return false;
  const int64_t o = (int64_t)(a.y & DICT_ID);
  if (*(const uint64_t*)(arena + o) != k.h || *(const int64_t*)(arena + o + 8) != k.len) return false;
  return k.sk ? key_words_eq_aligned(k.kw, arena + o + 16, k.len) : bytes_eq_aligned(arena + o + 16, k.kb, k.len);
}

// rows: null (row j = j) or a row list (the retry pass).  lists: DICT_NL regions of lcap entries
// [slot | the entry's byte offset in its list << 34]; lw[L]: entries << 40 | entry bytes of list L.
// nd[0] += the rows that probed (valid, not inline), nd[1] += the rows left pending (counted per
// wave by ballots, summed per block in LDS at the end: one global atomic per block).
__global__ __launch_bounds__(256) void k_dict_probe(ulonglong2* __restrict__ slots, uint64_t dmask,
                                                    const uint8_t* __restrict__ arena, const int64_t* __restrict__ koff,
                                                    const uint8_t* __restrict__ kbytes, const uint8_t* __restrict__ kv,
                                                    const uint8_t* __restrict__ rv, const int64_t* __restrict__ ts,
                                                    const int64_t* __restrict__ rows, int64_t n,
                                                    int64_t* __restrict__ kid, int64_t* __restrict__ khash,
                                                    uint64_t* __restrict__ lists, int64_t lcap,
                                                    unsigned long long* __restrict__ lw, int* __restrict__ fail,
                                                    uint64_t fpm, unsigned long long* __restrict__ nd) {
  __shared__ unsigned long long wsum[4];  // per wave: claims << 40 | entry bytes
  __shared__ unsigned long long bbase;
  __shared__ unsigned long long bsum[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = blockIdx.x & (DICT_NL - 1);
  if (threadIdx.x < 2) bsum[threadIdx.x] = 0;
  unsigned long long bprobed = 0, bpend = 0;  // (the wave's counts over its tiles)
  for (int64_t j0 = blockIdx.x * (int64_t)blockDim.x; j0 < n; j0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = j0 + threadIdx.x;
    bool claimed = false, probed = false, pending = false;
    uint64_t cslot = 0, eb = 0;
    if (j < n) {
      const int64_t i = rows ? rows[j] : j;
      if (!(bit_get(kv, i) && bit_get(rv, i) && (ts == nullptr || ts[i] >= 0))) {
        kid[i] = 0;
        if (khash) khash[i] = 0;
      } else {
        DKey k;
        dkey_words(k, koff, kbytes, i);
        int64_t code;
        const bool inl = key_inline(k, &code);
        k.h = 0;
        if (!inl) dkey_hash(k);
        probed = !inl;
        if (khash) khash[i] = inl ? code : (int64_t)k.h;
        const uint64_t fp = (k.h >> 40) & fpm;
        const uint64_t fresh = (1ULL << 63) | (fp << 40) | (uint64_t)i;
        uint64_t slot = k.h & dmask;
        bool done = inl;
        if (inl) kid[i] = code;
        for (int probe = 0; probe < DICT_PROBE && !done; probe++) {
          ulonglong2 a = slots[2 * slot];  // a stale empty / fresh word is settled by the CAS below
          uint64_t w = a.x;
          if (w == 0) {
            const uint64_t old = atomicCAS((unsigned long long*)&slots[2 * slot].x, 0ULL, (unsigned long long)fresh);
            if (old == 0) {
              kid[i] = -(int64_t)(slot + 1);  // commit writes the id
              claimed = true;
              cslot = slot;
              eb = (uint64_t)entry_bytes(k.len);
              done = true;
              break;
            }
            w = old;
          }
          if (((w >> 40) & 0x3FFFFFULL) == fp) {
            if (w >> 63) {  // claimed by another row of this batch: resolved after the commit
              kid[i] = -(int64_t)(slot + 1) - KID_PEND;
              pending = true;
              done = true;
            } else {
              const ulonglong2 b = slots[2 * slot + 1];
              if (a.x != w) a = slots[2 * slot];  // (the word moved on since the first read)
              if (dslot_eq(a, b, k, arena)) {
                kid[i] = (int64_t)(a.y & DICT_ID);
                done = true;
              }
            }
          }
          if (!done) slot = (slot + 1) & dmask;
        }
        if (!done) {
          kid[i] = 0;
          *fail = 1;
        }
      }
    }
    bprobed += (unsigned long long)__popcll(__ballot(probed));
    bpend += (unsigned long long)__popcll(__ballot(pending));
    // the block's claims → list L: one atomic per block and tile for both the count and the bytes
    const uint64_t x = claimed ? ((1ULL << 40) | eb) : 0ULL;
    uint64_t incl = x;
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tot = 0;
    for (int k = 0; k < 4; k++) {
      before += k < wave ? wsum[k] : 0;
      tot += wsum[k];
    }
    if (threadIdx.x == 0) bbase = tot ? atomicAdd(&lw[L], (unsigned long long)tot) : 0ULL;
    __syncthreads();
    if (claimed) {
      const uint64_t at = bbase + before + incl - x;  // this claim's entries << 40 | bytes before it
      const uint64_t idx = at >> 40, boff = at & ((1ULL << 40) - 1);
      if ((int64_t)idx < lcap && boff < (1ULL << 30)) lists[(uint64_t)L * lcap + idx] = cslot | (boff << 34);
      else *fail = 2;  // (lcap covers every row a list's blocks can claim)
    }
  }
  __syncthreads();
  if (lane == 0 && bprobed) atomicAdd(&bsum[0], bprobed);
  if (lane == 0 && bpend) atomicAdd(&bsum[1], bpend);
  __syncthreads();
  if (threadIdx.x < 2 && bsum[threadIdx.x]) atomicAdd(&nd[threadIdx.x], bsum[threadIdx.x]);
}

// The inline ids of a batch, before any dictionary work: rows without a key get 0, inline keys
// their id (khash: the id), other keys KID_DICT; nd[0] += the rows left for the dictionary, nd[1]
// += the inline rows (one atomic per block each; ts is not read: a late row's id is never used).
// Branch-free loads, R rows per thread: every row's offsets, then every row's first four aligned
// key words (clamped to the words that hold its bytes, so no load leaves the key column; an empty
// key reads the word of the column's first byte, or nothing when the column is empty), then the
// SWAR check per row.
constexpr int64_t KID_DICT = INT64_MIN;
template <int R>
__global__ __launch_bounds__(256) void k_key_inline(const int64_t* __restrict__ koff, const uint8_t* __restrict__ kbytes,
                                                    const uint8_t* __restrict__ kv, const uint8_t* __restrict__ rv,
                                                    const int64_t* __restrict__ ts, int64_t n, int64_t* __restrict__ kid,
                                                    int64_t* __restrict__ khash, unsigned long long* __restrict__ nd) {
  (void)ts;
  const int64_t kfirst = koff[0];
  const bool has_bytes = koff[n] > kfirst;
  const uint8_t* anchor = kbytes + kfirst;  // (a byte of the column when has_bytes)
  __shared__ unsigned int bsum[2];
  if (threadIdx.x < 2) bsum[threadIdx.x] = 0;
  unsigned int cnt = 0, ninl = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j0 < n; j0 += stride * R) {
    int64_t o0[R], len[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int64_t i = j0 + r * stride < n ? j0 + r * stride : n - 1;
      o0[r] = koff[i];
      len[r] = koff[i + 1] - o0[r];
    }
    uint64_t A[R][KW_MAX + 1];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint8_t* p = kbytes + o0[r];
      const int64_t lb = len[r] < 8 * KW_MAX ? len[r] : 8 * KW_MAX;  // (longer keys are never inline)
      const uint64_t a = (uint64_t)p;
      const uint64_t* base = (const uint64_t*)(p - (a & 7));
      const int last = lb > 0 ? (int)(((a & 7) + (uint64_t)lb - 1) >> 3) : 0;
      const uint64_t* b0 = lb > 0 ? base : (const uint64_t*)(anchor - ((uint64_t)anchor & 7));
#pragma unroll
      for (int k = 0; k <= KW_MAX; k++) A[r][k] = has_bytes ? b0[k < last ? k : last] : 0ULL;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int64_t i = j0 + r * stride;
      if (i >= n) break;
      int64_t code = 0;
      if (bit_get(kv, i) && bit_get(rv, i)) {
        // key_words from the loaded aligned words
        const uint64_t a = (uint64_t)(kbytes + o0[r]);
        const int sh = (int)(a & 7) * 8;
        DKey k;
        k.len = len[r];
        k.sk = k.len <= 8 * KW_MAX;
#pragma unroll
        for (int q = 0; q < KW_MAX; q++) {
          uint64_t x = sh ? (A[r][q] >> sh) | (A[r][q + 1] << (64 - sh)) : A[r][q];
          const int64_t left = k.len - 8 * q;
          if (left <= 0) x = 0;
          else if (left < 8) x &= (1ULL << (8 * left)) - 1;
          k.kw[q] = x;
        }
        if (key_inline(k, &code)) {
          ninl++;
        } else {
          code = KID_DICT;
          cnt++;
        }
      }
      kid[i] = code;
      if (khash) khash[i] = code;
    }
  }
  __syncthreads();
  if (cnt) atomicAdd(&bsum[0], cnt);
  if (ninl) atomicAdd(&bsum[1], ninl);
  __syncthreads();
  if (threadIdx.x < 2 && bsum[threadIdx.x]) atomicAdd(&nd[threadIdx.x], (unsigned long long)bsum[threadIdx.x]);
}

// The lists' arena bases after a probe round (one block, a thread per list): lbase[L] = the arena's
// used bytes + the entry bytes of the lists before L; the used bytes and the key count advance.
// Nothing when the round failed (c's first word: the probe's failure flag).
__global__ __launch_bounds__(1024) void k_dict_bases(unsigned long long* __restrict__ c,
                                                     const unsigned long long* __restrict__ lw,
                                                     int64_t* __restrict__ lbase) {
  static_assert(DICT_NL == 1024, "a thread per list");
  __shared__ unsigned long long ws[16], wk[16];
  if (*(const volatile int*)c != 0) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long x = lw[t];
  const unsigned long long by = x & ((1ULL << 40) - 1), ke = x >> 40;
  unsigned long long incl = by, kin = ke;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long y = __shfl_up(incl, off, 64), z = __shfl_up(kin, off, 64);
    if (lane >= off) {
      incl += y;
      kin += z;
    }
  }
  if (lane == 63) {
    ws[wave] = incl;
    wk[wave] = kin;
  }
  __syncthreads();
  unsigned long long before = 0, tot = 0, ktot = 0;
  for (int k = 0; k < 16; k++) {
    before += k < wave ? ws[k] : 0ULL;
    tot += ws[k];
    ktot += wk[k];
  }
  lbase[t] = (int64_t)(c[1] + before + incl - by);
  __syncthreads();  // (every thread has read c[1])
  if (t == 0) {
    c[1] += tot;
    c[2] += ktot;
  }
}

// One thread per claim (list L, entries t, t + stride, ...): the arena entry at its list's base +
// its byte offset, the slot made resident with the key's words, the claiming row's id.  lbase[L]:
// the list's arena base.  Nothing when the round failed.
__global__ __launch_bounds__(256) void k_dict_commit(ulonglong2* __restrict__ slots, const uint64_t* __restrict__ lists,
                                                     int64_t lcap, const unsigned long long* __restrict__ lw,
                                                     const int64_t* __restrict__ lbase, uint8_t* __restrict__ arena,
                                                     const int64_t* __restrict__ koff, const uint8_t* __restrict__ kbytes,
                                                     int64_t* __restrict__ kid, const unsigned long long* __restrict__ c) {
  if (*(const volatile int*)c != 0) return;
  const int L = blockIdx.y;
  const int64_t cntL = (int64_t)(lw[L] >> 40);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < cntL; t += (int64_t)gridDim.x * blockDim.x) {
  const uint64_t le = lists[(uint64_t)L * lcap + t];
  const uint64_t slot = le & ((1ULL << 34) - 1);
  const uint64_t w = slots[2 * slot].x;
  const int64_t r = (int64_t)(w & DICT_LOW);
  DKey k;
  dkey_load(k, koff, kbytes, r);
  const int64_t o = lbase[L] + (int64_t)(le >> 34);
  *(uint64_t*)(arena + o) = k.h;
  *(int64_t*)(arena + o + 8) = k.len;
  if (k.sk) {
    for (int q = 0; q < (int)((k.len + 7) >> 3); q++) ((uint64_t*)(arena + o + 16))[q] = k.kw[q];
  } else {
    for (int64_t b = 0; b < k.len; b++) arena[o + 16 + b] = k.kb[b];
  }
  const uint64_t fp = (w >> 40) & 0x3FFFFFULL;
  const uint64_t lenw = (uint64_t)(k.len < 0xFFFF ? k.len : 0xFFFF) << 48;
  slots[2 * slot + 1] = make_ulonglong2(k.len <= 16 ? k.kw[0] : 0ULL, k.len <= 16 && k.len > 8 ? k.kw[1] : 0ULL);
  slots[2 * slot] = make_ulonglong2((1ULL << 62) | (fp << 40) | ((uint64_t)o >> 3), (uint64_t)o | lenw);
  kid[r] = o;
  }
}

// Rows left pending on a slot another row claimed: the slot is resident now.  A different key of
// the same fingerprint goes on the retry list.
__global__ __launch_bounds__(256) void k_dict_resolve(const ulonglong2* __restrict__ slots,
                                                      const uint8_t* __restrict__ arena,
                                                      const int64_t* __restrict__ koff,
                                                      const uint8_t* __restrict__ kbytes, const int64_t* __restrict__ rows,
                                                      int64_t n, int64_t* __restrict__ kid,
                                                      int64_t* __restrict__ retry, unsigned long long* __restrict__ nretry,
                                                      const unsigned long long* __restrict__ c,
                                                      const unsigned long long* __restrict__ npend) {
  if (*(const volatile int*)c != 0 || *npend == 0) return;  // (a failed round, or no row pending)
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = rows ? rows[j] : j;
    const int64_t x = kid[i];
    if (x >= -KID_PEND) continue;  // an id, or the claimer's (written by the commit)
    const uint64_t slot = (uint64_t)(-(x + KID_PEND) - 1);
    DKey k;
    dkey_load(k, koff, kbytes, i);
    const ulonglong2 a = slots[2 * slot], b = slots[2 * slot + 1];
    if (dslot_eq(a, b, k, arena)) {
      kid[i] = (int64_t)(a.y & DICT_ID);
    } else {
      kid[i] = 0;
      retry[atomicAdd(nretry, 1ULL)] = i;
    }
  }
}

// Read-only dictionary probe (pull queries, join probes): key bytes → resident key id (arena
// offset), or -1 when the key was never seen.  Every slot is resident between maps.
__global__ __launch_bounds__(256) void k_dict_find(const ulonglong2* __restrict__ slots, uint64_t dmask,
                                                   const uint8_t* __restrict__ arena,
                                                   const int64_t* __restrict__ koff, const uint8_t* __restrict__ kbytes,
                                                   int64_t n, int64_t* __restrict__ kid, uint64_t fpm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    DKey k;
    dkey_words(k, koff, kbytes, i);
    int64_t code;
    if (key_inline(k, &code)) {
      kid[i] = code;
      continue;
    }
    dkey_hash(k);
    const uint64_t fp = (k.h >> 40) & fpm;
    uint64_t slot = k.h & dmask;
    int64_t found = -1;
    for (int probe = 0; probe <= (int)dmask && probe < (1 << 20); probe++) {
      const ulonglong2 a = slots[2 * slot];
      if (a.x == 0) break;
      if (((a.x >> 40) & 0x3FFFFFULL) == fp && dslot_eq(a, slots[2 * slot + 1], k, arena)) {
        found = (int64_t)(a.y & DICT_ID);
        break;
      }
      slot = (slot + 1) & dmask;
    }
    kid[i] = found;
  }
}

// A failed map: the batch's fresh claims → empty (the table is as before the batch).
__global__ __launch_bounds__(256) void k_dict_unclaim(ulonglong2* __restrict__ slots, int64_t dcap) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < dcap; s += (int64_t)gridDim.x * blockDim.x)
    if (slots[2 * s].x >> 63) slots[2 * s] = make_ulonglong2(0ULL, 0ULL);
}

__global__ __launch_bounds__(256) void k_dict_rehash(const ulonglong2* __restrict__ os, int64_t ocap,
                                                     ulonglong2* __restrict__ ns, uint64_t nmask,
                                                     const uint8_t* __restrict__ arena) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < ocap; s += (int64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = os[2 * s];
    if (a.x == 0) continue;
    const uint64_t h = *(const uint64_t*)(arena + (a.y & DICT_ID));
    uint64_t d = h & nmask;
    while (atomicCAS((unsigned long long*)&ns[2 * d].x, 0ULL, (unsigned long long)a.x) != 0ULL) d = (d + 1) & nmask;
    ns[2 * d + 1] = os[2 * s + 1];
    ns[2 * d].y = a.y;
  }
}

// ------------------------------------------------------------------- host side: KeyDict (khip_dict.hpp)

// The fingerprint bits a probe compares before the key (22; the tuning build's KHIP_DICT_FPMASK
// narrows them so that different keys meet on claimed slots: the pending / retry rounds).
static uint64_t dict_fp_mask() { return (uint64_t)knob("KHIP_DICT_FPMASK", 0x3FFFFF) & 0x3FFFFFULL; }

static khip_status dict_grow(KeyDict& d, hipStream_t s, int64_t new_cap) {
  DevBuf ns;
  KHIP_TRY(ns.ensure((size_t)new_cap * 32));
  KHIP_TRY_HIP(hipMemsetAsync(ns.p, 0, (size_t)new_cap * 32, s));
  if (d.dcap > 0 && d.docc > 0) {
    hipLaunchKernelGGL(k_dict_rehash, dim3(grid_for(d.dcap, 256)), dim3(256), 0, s, d.slots.as<ulonglong2>(), d.dcap,
                       ns.as<ulonglong2>(), (uint64_t)(new_cap - 1), d.arena.as<uint8_t>());
    KHIP_TRY_HIP(hipGetLastError());
  }
  KHIP_TRY_HIP(hipStreamSynchronize(s));
  d.slots.release();
  d.slots = std::move(ns);
  ns.p = nullptr;
  d.dcap = new_cap;
  return KHIP_OK;
}

khip_status dict_init(KeyDict& d, hipStream_t s) {
#ifdef KHIP_TUNING
  const uint64_t hm = (uint64_t)knob("KHIP_DICT_HASHMASK", -1);
  KHIP_TRY_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dict_hmask), &hm, 8));
  const int inl = (int)knob("KHIP_KEY_INLINE", 1);
  KHIP_TRY_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_key_inline), &inl, 4));
#endif
  KHIP_TRY(d.ctr.ensure(64 + 16 * DICT_NL));  // (dict_round's counters)
  return dict_grow(d, s, 4096);
}

// One round over `rows` (null: every row): probe, commit the claims, resolve the pending rows.
// Returns the rows to retry (a different key behind a pending row's fingerprint) in d.retry,
// their count in *nretry; *failed when a probe ran out of budget (nothing committed then).
// Counters (d.ctr, u64): [0] probe failure | [1] arena bytes used | [2] keys added | [3] retries |
// [4 ..] DICT_NL list words | then DICT_NL list arena bases | rows probed | rows pending.
static khip_status dict_round(KeyDict& d, hipStream_t s, const int64_t* koff, const uint8_t* kbytes, const uint8_t* kv,
                              const uint8_t* rv, const int64_t* ts, const int64_t* rows, int64_t n, int64_t* kid,
                              int64_t* khash, int64_t* nretry, bool* failed) {
  unsigned long long* c = d.ctr.as<unsigned long long>();
  unsigned long long* lw = c + 4;
  int64_t* lbase = (int64_t*)(c + 4 + DICT_NL);
  unsigned long long* nd = c + 4 + 2 * DICT_NL;
  const int g = grid_for(n, 256);
  // a list takes the claims of blocks L, L + DICT_NL, ...: at most every row those blocks visit
  const int64_t lcap = ceil_div(g, DICT_NL) * 256 * ceil_div(n, 256LL * g);
  KHIP_TRY(d.lists.ensure((size_t)lcap * DICT_NL * 8));
  KHIP_TRY(d.retry.ensure((size_t)std::max<int64_t>(n, 1) * 8));
  KHIP_TRY_HIP(hipMemsetAsync(c, 0, 8, s));
  KHIP_TRY_HIP(hipMemsetAsync(c + 3, 0, 8 + 8 * DICT_NL, s));
  KHIP_TRY_HIP(hipMemsetAsync(nd, 0, 16, s));
  // probe → list bases → commit → resolve, with no host round trip in between: each later kernel
  // does nothing when the probe failed (the table is grown and the round mapped again)
  hipLaunchKernelGGL(k_dict_probe, dim3(g), dim3(256), 0, s, d.slots.as<ulonglong2>(), (uint64_t)(d.dcap - 1),
                     d.arena.as<uint8_t>(), koff, kbytes, kv, rv, ts, rows, n, kid, khash, d.lists.as<uint64_t>(), lcap,
                     lw, (int*)c, dict_fp_mask(), nd);
  hipLaunchKernelGGL(k_dict_bases, dim3(1), dim3(DICT_NL), 0, s, c, (const unsigned long long*)lw, lbase);
  hipLaunchKernelGGL(k_dict_commit, dim3((unsigned)std::min<int64_t>(4, ceil_div(lcap, 256LL)), DICT_NL), dim3(256), 0,
                     s, d.slots.as<ulonglong2>(), d.lists.as<uint64_t>(), lcap, lw, lbase, d.arena.as<uint8_t>(), koff,
                     kbytes, kid, (const unsigned long long*)c);
  hipLaunchKernelGGL(k_dict_resolve, dim3(g), dim3(256), 0, s, d.slots.as<ulonglong2>(), d.arena.as<uint8_t>(), koff,
                     kbytes, rows, n, kid, d.retry.as<int64_t>(), c + 3, (const unsigned long long*)c,
                     (const unsigned long long*)(nd + 1));
  KHIP_TRY_HIP(hipGetLastError());
  unsigned long long h[6];
  KHIP_TRY_HIP(hipMemcpyAsync(h, c, 32, hipMemcpyDeviceToHost, s));
  KHIP_TRY_HIP(hipMemcpyAsync(h + 4, nd, 16, hipMemcpyDeviceToHost, s));
  KHIP_TRY_HIP(hipStreamSynchronize(s));
  *failed = (h[0] & 0xFFFFFFFFULL) != 0;
  d.round_probed = (int64_t)h[4];
  if (!rows) d.last_probed = d.round_probed;  // (the first round sees every row)
  *nretry = *failed ? 0 : (int64_t)h[3];
  if (!*failed) {  // (cumulative over the map's rounds)
    d.round_used = (int64_t)h[1];
    d.round_keys = (int64_t)h[2];
  }
  return KHIP_OK;
}

khip_status dict_map(KeyDict& d, hipStream_t s, const int64_t* koff, const uint8_t* kbytes, int64_t key_bytes_total,
                     const uint8_t* kv, const uint8_t* rv, const int64_t* ts, int64_t n, int64_t* kid, int64_t* khash) {
  // inline ids first: a batch whose keys are all inline (or invalid) never touches the dictionary.
  // (Skipped while the maps find no inline key at all — the probe turns inline keys into their ids
  // too — and tried again every 16th map.)
  if (d.last_inline != 0 || (++d.maps & 15) == 0) {
    unsigned long long* nd = d.ctr.as<unsigned long long>() + 4 + 2 * DICT_NL + 2;
    KHIP_TRY_HIP(hipMemsetAsync(nd, 0, 16, s));
    // rows per thread (1 / 2 / 4 / 8: 751 / 740 / 807 / 982 us on C2 --utf8, profiles/r05/ab/inline_rows.txt)
    const int ir = (int)knob("KHIP_INLINE_R", 2);
    auto ik = ir >= 8 ? k_key_inline<8> : (ir >= 4 ? k_key_inline<4> : (ir >= 2 ? k_key_inline<2> : k_key_inline<1>));
    hipLaunchKernelGGL(ik, dim3(grid_for(ceil_div(n, (int64_t)std::max(ir, 1)), 256, 4096)), dim3(256), 0, s, koff, kbytes, kv,
                       rv, ts, n, kid, khash, nd);
    KHIP_TRY_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    KHIP_TRY_HIP(hipMemcpyAsync(h, nd, 16, hipMemcpyDeviceToHost, s));
    KHIP_TRY_HIP(hipStreamSynchronize(s));
    d.last_inline = (int64_t)h[1];
    if (h[0] == 0) {
      d.last_probed = d.round_probed = 0;
      if (d.last_added < 0) d.last_added = 0;
      return KHIP_OK;
    }
  }
  // room for the keys this batch may add at load <= 1/2: an eighth of the rows on the first map,
  // then twice the last map's new keys (at least 1/16 of the rows that reached the dictionary:
  // inline keys never do) — a batch that brings more fails its probes and is mapped again into a
  // larger table, so the table tracks the key count, not the batch size
  const int64_t est =
      d.last_added < 0 ? std::max<int64_t>(n / 8, 4096)
                       : std::min<int64_t>(n, std::max<int64_t>({2 * d.last_added, std::min(n, d.last_probed) / 16, 4096}));
  if (2 * (d.docc + est) > d.dcap) KHIP_TRY(dict_grow(d, s, next_pow2(2 * (d.docc + est))));
  const int64_t need = d.arena_used + key_bytes_total + 16 * n + 16;
  if ((size_t)need > d.arena.bytes) {
    DevBuf na;
    KHIP_TRY(na.ensure((size_t)std::max<int64_t>(need * 2, 1 << 20)));
    if (d.arena_used) KHIP_TRY_HIP(hipMemcpyAsync(na.p, d.arena.p, d.arena_used, hipMemcpyDeviceToDevice, s));
    KHIP_TRY_HIP(hipStreamSynchronize(s));
    d.arena.release();
    d.arena = std::move(na);
    na.p = nullptr;
  }
  unsigned long long* c = d.ctr.as<unsigned long long>();
  const unsigned long long start[3] = {0ULL, (unsigned long long)d.arena_used, 0ULL};
  KHIP_TRY_HIP(hipMemcpyAsync(c, start, 24, hipMemcpyHostToDevice, s));
  d.round_used = d.arena_used;
  d.round_keys = 0;
  const int64_t* rows = nullptr;
  int64_t m = n;
  DevBuf rl;  // a retry round's rows (the previous round's retry list)
  for (int round = 0, grown = 0; m > 0; round++) {
    int64_t nretry = 0;
    bool failed = false;
    KHIP_TRY(dict_round(d, s, koff, kbytes, kv, rv, ts, rows, m, kid, khash, &nretry, &failed));
    if (failed) {  // undo this round's claims, grow, and map its rows again
      if (++grown > 6 || d.dcap >= ((int64_t)1 << 34)) return fail(KHIP_E_DEVICE, "key dictionary probe budget exhausted");
      hipLaunchKernelGGL(k_dict_unclaim, dim3(grid_for(d.dcap, 256)), dim3(256), 0, s, d.slots.as<ulonglong2>(), d.dcap);
      KHIP_TRY_HIP(hipGetLastError());
      // (room for every row that probed, as distinct keys, at load <= 1/2)
      KHIP_TRY(dict_grow(d, s, std::max<int64_t>(d.dcap * 4, next_pow2(2 * (d.docc + d.round_probed)))));
      continue;
    }
    if (round > 64) return fail(KHIP_E_DEVICE, "key dictionary: rows unresolved after 64 rounds");
    if (nretry == 0) break;
    KHIP_TRY(rl.ensure((size_t)nretry * 8));
    KHIP_TRY_HIP(hipMemcpyAsync(rl.p, d.retry.p, (size_t)nretry * 8, hipMemcpyDeviceToDevice, s));
    rows = rl.as<int64_t>();
    m = nretry;
  }
  d.arena_used = d.round_used;
  d.docc += d.round_keys;
  d.last_added = d.round_keys;
  return KHIP_OK;
}

khip_status dict_find(KeyDict& d, hipStream_t s, const int64_t* koff, const uint8_t* kbytes, int64_t n, int64_t* kid) {
  if (n <= 0) return KHIP_OK;
  hipLaunchKernelGGL(k_dict_find, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, d.slots.as<ulonglong2>(),
                     (uint64_t)(d.dcap - 1), d.arena.as<uint8_t>(), koff, kbytes, n, kid, dict_fp_mask());
  KHIP_TRY_HIP(hipGetLastError());
  return KHIP_OK;
}

khip_status dict_clear(KeyDict& d, hipStream_t s) {
  // the next batches likely bring as many keys as the dictionary held: a table far larger than
  // that (sized by a first map's every-row estimate) is given back
  const int64_t held = d.docc;
  const int64_t keep = std::max<int64_t>(4096, next_pow2(4 * std::max<int64_t>(held, 1)));
  d.docc = 0;
  if (d.dcap >= 4 * keep) KHIP_TRY(dict_grow(d, s, keep));
  if (d.dcap) KHIP_TRY_HIP(hipMemsetAsync(d.slots.p, 0, d.dcap * 32, s));
  if (held > 0) d.last_added = held;  // the next map re-inserts about as many
  d.arena_used = 0;
  return KHIP_OK;
}

void dict_release(KeyDict& d) {
  DevBuf* bufs[] = {&d.slots, &d.arena, &d.ctr, &d.lists, &d.retry};
  for (DevBuf* b : bufs) b->release();
  d.dcap = d.docc = d.arena_used = 0;
}

}  // namespace khip
