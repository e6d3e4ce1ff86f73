// khip_correlation.hpp — CORRELATION(x, y) over an INT or a BIGINT pair: the decode of a group's
// additive integer state into the Pearson coefficient (DESIGN.md "CORRELATION aggregate").  Host
// and device; no other header of the project is needed but khip_variance.hpp, whose mul64 it uses
// (tools/correlation_check.cpp builds it alone).
//
// State of one (x, y) pair of argument columns.  A record counts when x and y are both non-null
// (CorrelationUdaf.java:88-90); every word is kept by commutative u64 adds (and subtracts: the table
// engine's undo), so any order, any cut into pushes and any retry give the same words:
//   n        the pairs
//   sx, sy   INT: one word, the sum of the sign-extended values; BIGINT: two words, Σ (v & 0xFFFFFFFF)
//            and Σ (v >> 32), arithmetic shift, signed
//   sxx, syy Σ of the 32-bit limb j of v² — 2 limbs for INT, 4 for BIGINT (as STDDEV's)
//   sxy      with p = x y in two's complement (INT: 64 bits, BIGINT: 128 bits): Σ of its 32-bit limbs,
//            the top limb taken with an arithmetic shift (signed), the others unsigned — 2 / 4 words
// Every addend is an unsigned 32-bit limb or a signed quantity of magnitude <= 2^31, so no word can
// carry out while a group has at most 2^32 - 1 pairs.  Beyond that the words wrap and the result is
// unspecified (nothing faults).
//
//   Sx = Σx, Sy = Σy, Sxx = Σx², Syy = Σy², Sxy = Σxy   rebuilt exactly (signed top parts, carries)
//   N  = n Sxy - Sx Sy (signed),  DX = n Sxx - Sx²,  DY = n Syy - Sy²        exact, 256-bit integers
//   r  = RN(N) / sqrt(RN(DX) * RN(DY))   each RN one round-half-even of the integer to a double, then
//                                        the reference's own three operations in its order (map,
//                                        CorrelationUdaf.java:127-133)
//   n = 0 or RN(DX) * RN(DY) = 0  ->  the canonical quiet NaN (the reference's 0.0 / 0.0)
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "khip_variance.hpp"

namespace khip {

struct I256 {
  uint64_t w[4];  // two's complement, little-endian
};

KHIP_VAR_HD I256 i256_add(const I256& a, const I256& b) {
  I256 r;
  uint64_t carry = 0;
  for (int k = 0; k < 4; k++) {
    const uint64_t s = a.w[k] + b.w[k];
    const uint64_t c1 = s < b.w[k];
    r.w[k] = s + carry;
    carry = c1 | (uint64_t)(r.w[k] < s);
  }
  return r;
}

KHIP_VAR_HD I256 i256_neg(const I256& a) {
  I256 r;
  uint64_t carry = 1;
  for (int k = 0; k < 4; k++) {
    r.w[k] = ~a.w[k] + carry;
    carry = carry && r.w[k] == 0;
  }
  return r;
}

KHIP_VAR_HD I256 i256_sub(const I256& a, const I256& b) { return i256_add(a, i256_neg(b)); }

// v (sign-extended when sgn, else zero-extended) * 2^(32 k), k in [0, 4)
KHIP_VAR_HD I256 i256_word(uint64_t v, bool sgn, int k) {
  const uint64_t ext = sgn && (v >> 63) ? ~0ull : 0ull;
  const uint64_t t[4] = {v, ext, ext, ext};
  I256 r{{0, 0, 0, 0}};
  const int ws = k >> 1, bs = (k & 1) * 32;
  for (int i = 3; i >= ws; i--) {
    uint64_t x = t[i - ws] << bs;
    if (bs && i - ws - 1 >= 0) x |= t[i - ws - 1] >> (64 - bs);
    r.w[i] = x;
  }
  return r;
}

// a b mod 2^256 (two's complement: signed and unsigned alike)
KHIP_VAR_HD I256 i256_mul(const I256& a, const I256& b) {
  I256 r{{0, 0, 0, 0}};
  for (int i = 0; i < 4; i++)
    for (int j = 0; i + j < 4; j++) {
      uint64_t lo, hi;
      mul64(a.w[i], b.w[j], &lo, &hi);
      I256 t{{0, 0, 0, 0}};
      t.w[i + j] = lo;
      if (i + j + 1 < 4) t.w[i + j + 1] = hi;
      r = i256_add(r, t);
    }
  return r;
}

// RN(a): the signed integer rounded once, half to even, to a double.
KHIP_VAR_HD double i256_to_double(const I256& a) {
  const bool neg = a.w[3] >> 63;
  const I256 m = neg ? i256_neg(a) : a;  // (-2^255 is its own negation: read as 2^255, unsigned)
  int L = 0;  // bit length
  for (int k = 3; k >= 0 && !L; k--)
    if (m.w[k]) {
      int b = 63;
      while (!((m.w[k] >> b) & 1)) b--;
      L = 64 * k + b + 1;
    }
  if (L == 0) return 0.0;
  double d;
  if (L <= 53) {
    d = (double)m.w[0];
  } else {
    const int k = L - 53;  // the bits below the 53 kept
    uint64_t f = 0;
    for (int i = 0; i < 53; i++) f |= ((m.w[(k + i) >> 6] >> ((k + i) & 63)) & 1) << i;
    const bool half = (m.w[(k - 1) >> 6] >> ((k - 1) & 63)) & 1;
    bool sticky = false;
    for (int i = 0; i < k - 1 && !sticky; i++) sticky = (m.w[i >> 6] >> (i & 63)) & 1;
    if (half && (sticky || (f & 1))) f++;  // (2^53 is a double too)
    d = ldexp((double)f, k);
  }
  return neg ? -d : d;
}

KHIP_VAR_HD double correlation_nan() {  // the canonical quiet NaN (the host's 0.0 / 0.0 has the sign bit set)
  const uint64_t b = 0x7FF8000000000000ull;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// Σv from its words (see the file header).
KHIP_VAR_HD I256 corr_sum(bool bigint, const uint64_t* s) {
  return bigint ? i256_add(i256_word(s[0], false, 0), i256_word(s[1], true, 1)) : i256_word(s[0], true, 0);
}

// Σ of a 2- or 4-limb quantity; top_signed: the last limb is a signed sum (Σxy), else unsigned (Σv²).
KHIP_VAR_HD I256 corr_limbs(bool bigint, const uint64_t* s, bool top_signed) {
  const int n = bigint ? 4 : 2;
  I256 r{{0, 0, 0, 0}};
  for (int j = 0; j < n; j++) r = i256_add(r, i256_word(s[j], top_signed && j == n - 1, j));
  return r;
}

// The words of one pair (see the file header): sx / sy 1 (INT) or 2 (BIGINT) words, sxx / syy / sxy
// 2 or 4.
KHIP_VAR_HD double correlation_result(bool bigint, uint64_t n, const uint64_t* sx, const uint64_t* sy,
                                      const uint64_t* sxx, const uint64_t* syy, const uint64_t* sxy) {
  if (n == 0) return correlation_nan();
  const I256 N_ = i256_word(n, false, 0);
  const I256 Sx = corr_sum(bigint, sx), Sy = corr_sum(bigint, sy);
  const I256 Sxx = corr_limbs(bigint, sxx, false), Syy = corr_limbs(bigint, syy, false);
  const I256 Sxy = corr_limbs(bigint, sxy, true);
  const double num = i256_to_double(i256_sub(i256_mul(N_, Sxy), i256_mul(Sx, Sy)));
  const double dx = i256_to_double(i256_sub(i256_mul(N_, Sxx), i256_mul(Sx, Sx)));
  const double dy = i256_to_double(i256_sub(i256_mul(N_, Syy), i256_mul(Sy, Sy)));
  const double den2 = dx * dy;
  if (den2 == 0.0) return correlation_nan();
  const double r = num / sqrt(den2);
  return r != r ? correlation_nan() : r;  // (a state past the limit may have a negative DX DY)
}

}  // namespace khip
