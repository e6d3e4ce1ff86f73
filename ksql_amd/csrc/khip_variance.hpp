// khip_variance.hpp — STDDEV_SAMP / STDDEV_SAMPLE over INT / BIGINT: the decode of a group's
// additive integer state into the result (DESIGN.md "STDDEV aggregates").  Host and device; no
// other header of the project is needed (tools/variance_check.cpp builds it alone).
//
// State of one argument column, every word kept by commutative u64 adds (and subtracts: the table
// engine's undo), so any order, any cut into pushes and any retry give the same words:
//   n        non-null records (the column's count word, shared with COUNT / AVG)
//   sum      INT: the 64-bit sum of the sign-extended values (exact); BIGINT: Σx mod 2^64 (the word
//            SUM / AVG read)
//   hi       BIGINT only: Σ (x >> 32), arithmetic shift, signed (exact)
//   sq[j]    Σ of the 32-bit limb j of x² — 2 limbs for INT (x² < 2^63), 4 for BIGINT (x² <= 2^126)
// Exact while a group has at most 2^32 - 1 non-null records (no word can then carry out: a limb
// is < 2^32, |x >> 32| <= 2^31).  Beyond that the words wrap and the result is unspecified.
//
//   T = Σx  = INT: sum;  BIGINT: hi * 2^32 + ((sum - (hi << 32)) mod 2^64)   (the low parts' sum
//                                                                            is < 2^64)
//   Q = Σx² = Σ_j sq[j] * 2^(32 j)
//   n < 2          -> 0.0
//   M2 = RN((n Q - T²) / n)        one round-half-even of the exact rational, 192-bit integers
//   STDDEV_SAMP   = M2 / (double)(n - 1)
//   STDDEV_SAMPLE = sqrt(STDDEV_SAMP)
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KHIP_VAR_HD __host__ __device__ inline
#else
#define KHIP_VAR_HD inline
#endif

namespace khip {

struct U192 {
  uint64_t w[3];  // little-endian
};

KHIP_VAR_HD void mul64(uint64_t a, uint64_t b, uint64_t* lo, uint64_t* hi) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  *lo = (mid << 32) | (uint32_t)p00;
  *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// r += v * 2^(64 i + sh) (mod 2^192), sh in [0, 64)
KHIP_VAR_HD void u192_add_shifted(U192* r, uint64_t v, int i, int sh) {
  uint64_t part[2] = {v << sh, sh ? v >> (64 - sh) : 0};
  uint64_t carry = 0;
  for (int k = i, j = 0; k < 3; k++, j++) {
    const uint64_t a = j < 2 ? part[j] : 0;
    const uint64_t s = r->w[k] + a;
    const uint64_t c1 = s < a;
    const uint64_t t = s + carry;
    carry = c1 | (uint64_t)(t < s);
    r->w[k] = t;
  }
}

KHIP_VAR_HD U192 u192_mul64(const U192& a, uint64_t b) {  // mod 2^192
  U192 r{{0, 0, 0}};
  for (int k = 0; k < 3; k++) {
    uint64_t lo, hi;
    mul64(a.w[k], b, &lo, &hi);
    u192_add_shifted(&r, lo, k, 0);
    if (k + 1 < 3) u192_add_shifted(&r, hi, k + 1, 0);
  }
  return r;
}

KHIP_VAR_HD U192 u192_sub(const U192& a, const U192& b) {  // mod 2^192
  U192 r;
  uint64_t borrow = 0;
  for (int k = 0; k < 3; k++) {
    const uint64_t d = a.w[k] - b.w[k];
    const uint64_t b1 = a.w[k] < b.w[k];
    r.w[k] = d - borrow;
    borrow = b1 | (uint64_t)(d < borrow);
  }
  return r;
}

KHIP_VAR_HD U192 u192_shl(const U192& a, int s) {  // s in [0, 192)
  U192 r{{0, 0, 0}};
  const int ws = s >> 6, bs = s & 63;
  for (int k = 2; k >= ws; k--) {
    uint64_t v = a.w[k - ws] << bs;
    if (bs && k - ws - 1 >= 0) v |= a.w[k - ws - 1] >> (64 - bs);
    r.w[k] = v;
  }
  return r;
}

KHIP_VAR_HD int u192_bits(const U192& a) {  // bit length (0 for 0)
  for (int k = 2; k >= 0; k--)
    if (a.w[k]) {
      int b = 63;
      while (!((a.w[k] >> b) & 1)) b--;
      return 64 * k + b + 1;
    }
  return 0;
}

KHIP_VAR_HD bool u192_bit(const U192& a, int i) { return (a.w[i >> 6] >> (i & 63)) & 1; }

// a / n and the remainder (n > 0).
KHIP_VAR_HD U192 u192_divmod(const U192& a, uint64_t n, uint64_t* rem) {
  U192 q{{0, 0, 0}};
  uint64_t r = 0;
  if (n <= 0xFFFFFFFFull) {  // 32-bit limbs: (r << 32 | limb) fits 64 bits
    for (int k = 5; k >= 0; k--) {
      const uint64_t limb = (a.w[k >> 1] >> ((k & 1) * 32)) & 0xFFFFFFFFull;
      const uint64_t cur = (r << 32) | limb;
      const uint64_t d = cur / n;
      r = cur - d * n;
      q.w[k >> 1] |= d << ((k & 1) * 32);
    }
  } else {  // (past the exact range: bit by bit, the remainder's 65th bit in `top`)
    for (int i = 191; i >= 0; i--) {
      const uint64_t top = r >> 63;
      r = (r << 1) | (uint64_t)u192_bit(a, i);
      if (top || r >= n) {
        r -= n;
        q.w[i >> 6] |= 1ull << (i & 63);
      }
    }
  }
  *rem = r;
  return q;
}

// RN(D / n): the exact rational rounded once, half to even, to a double (n > 0).
KHIP_VAR_HD double u192_div_rn(const U192& D, uint64_t n) {
  uint64_t r;
  U192 q = u192_divmod(D, n, &r);
  int L = u192_bits(q);
  int s = 0;  // the quotient is taken of D * 2^s, so that it has at least 55 bits
  if (L < 55) {
    if (L == 0 && r == 0) return 0.0;
    s = L == 0 ? 119 : 55 - L;  // (D < n * 2^L: D * 2^s stays below 2^184)
    q = u192_divmod(u192_shl(D, s), n, &r);
    L = u192_bits(q);
  }
  const int k = L - 53;  // >= 2
  uint64_t m = 0;
  for (int i = 0; i < 53; i++) m |= (uint64_t)u192_bit(q, k + i) << i;
  const bool half = u192_bit(q, k - 1);
  bool sticky = r != 0;
  for (int i = 0; i < k - 1 && !sticky; i++) sticky = u192_bit(q, i);
  if (half && (sticky || (m & 1))) m++;  // (2^53 is a double too)
  return ldexp((double)m, k - s);
}

// The state of one column (see the file header).  n_limbs: 2 (INT) or 4 (BIGINT).
KHIP_VAR_HD double variance_m2(bool bigint, uint64_t n, uint64_t sum, uint64_t hi, const uint64_t* sq, int n_limbs) {
  // |T| as 128 bits and T's sign
  uint64_t t_lo, t_hi;
  bool neg;
  if (!bigint) {
    const int64_t t = (int64_t)sum;
    neg = t < 0;
    t_lo = neg ? 0 - (uint64_t)t : (uint64_t)t;
    t_hi = 0;
  } else {
    const uint64_t low = sum - (hi << 32);  // Σ (x & 0xFFFFFFFF), below 2^64
    // T = (int64)hi * 2^32 + low as a two's complement 128-bit number
    uint64_t lo = hi << 32, up = (uint64_t)((int64_t)hi >> 32);
    lo += low;
    up += lo < low;
    neg = (int64_t)up < 0;
    if (neg) {
      lo = ~lo + 1;
      up = ~up + (lo == 0);
    }
    t_lo = lo;
    t_hi = up;
  }
  (void)neg;  // T enters squared
  // T² mod 2^192
  U192 tt{{0, 0, 0}};
  uint64_t lo, up;
  mul64(t_lo, t_lo, &lo, &up);
  u192_add_shifted(&tt, lo, 0, 0);
  u192_add_shifted(&tt, up, 1, 0);
  mul64(t_lo, t_hi, &lo, &up);  // twice, at 2^64
  u192_add_shifted(&tt, lo, 1, 1);
  u192_add_shifted(&tt, up, 2, 1);
  mul64(t_hi, t_hi, &lo, &up);  // at 2^128
  u192_add_shifted(&tt, lo, 2, 0);
  // Q
  U192 Q{{0, 0, 0}};
  for (int j = 0; j < n_limbs; j++) u192_add_shifted(&Q, sq[j], j >> 1, (j & 1) * 32);
  const U192 D = u192_sub(u192_mul64(Q, n), tt);
  return u192_div_rn(D, n);
}

// STDDEV_SAMP (sample = false: the variance, as the reference returns it) or STDDEV_SAMPLE.
KHIP_VAR_HD double variance_result(bool sample, bool bigint, int64_t n, uint64_t sum, uint64_t hi, const uint64_t* sq,
                                   int n_limbs) {
  if (n < 2) return 0.0;
  const double v = variance_m2(bigint, (uint64_t)n, sum, hi, sq, n_limbs) / (double)(n - 1);
  return sample ? sqrt(v) : v;
}

}  // namespace khip
