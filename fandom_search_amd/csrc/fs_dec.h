// fs_dec.h -- the text of a distance field to the double Python's float() gives for it, on the
// host and on the device from one function (fs_matches.hip, fs_matches_parse_double).
//
// Grammar (what repr(float) writes, and the empty field): "", "nan", "inf", "-inf", or
//   [-] digits [. digits] [(e|E) [+|-] digits]   with at most 17 significant digits
// (leading zeros do not count, trailing ones do).  Anything else is FS_DEC_NOT_MINE and
// carries no value: the caller hands the field to float().
//
// The conversion is the one of D. Lemire, "Number parsing at a gigabyte per second" (2021): the
// decimal significand w (< 2^64) times a 128-bit approximation of 5^q, rounded from the top of
// the 128-bit product; the second half of the table entry is consulted when the first product's
// low bits cannot decide.  J. Mushtak and D. Lemire, "Fast number parsing without fallback"
// (2023) prove that this decides every w < 2^64, so there is no slow path and every string of
// the grammar comes back FS_DEC_SURE.
#ifndef FS_DEC_H
#define FS_DEC_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_DEC_HD __host__ __device__
#else
#define FS_DEC_HD
#endif

enum { FS_DEC_SURE = 0, FS_DEC_NOT_MINE = 1 };

namespace fs_dec_host {
#define FS_POW5_QUAL static
#include "fs_pow5.h"
#undef FS_POW5_QUAL
}  // namespace fs_dec_host
#if defined(__HIPCC__)
namespace fs_dec_dev {
#define FS_POW5_QUAL __device__ static
#include "fs_pow5.h"
#undef FS_POW5_QUAL
}  // namespace fs_dec_dev
#endif

constexpr int kDecQMin = -342, kDecQMax = 308;
constexpr uint32_t kDecMaxDigits = 17;

FS_DEC_HD inline uint64_t fs_dec_pow5(int q, int half) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fs_dec_dev::fs_pow5_128[2 * (q - kDecQMin) + half];
#else
  return fs_dec_host::fs_pow5_128[2 * (q - kDecQMin) + half];
#endif
}

FS_DEC_HD inline void fs_dec_mul(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *lo = a * b;
  *hi = __umul64hi(a, b);
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *lo = (uint64_t)p;
  *hi = (uint64_t)(p >> 64);
#endif
}

FS_DEC_HD inline int fs_dec_clz(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)x);
#else
  return __builtin_clzll(x);
#endif
}

FS_DEC_HD inline double fs_dec_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, sizeof d);
  return d;
}

// w * 10^q, correctly rounded (round to nearest, ties to even); w != 0, kDecQMin <= q <= kDecQMax
FS_DEC_HD inline uint64_t fs_dec_round(uint64_t w, int q) {
  const int lz = fs_dec_clz(w);
  w <<= lz;
  uint64_t hi, lo;
  fs_dec_mul(w, fs_dec_pow5(q, 0), &hi, &lo);
  if ((hi & 0x1FF) == 0x1FF) {               // the 9 bits under the 55 that are kept
    uint64_t hi2, lo2;
    fs_dec_mul(w, fs_dec_pow5(q, 1), &hi2, &lo2);
    lo += hi2;
    if (hi2 > lo) ++hi;
  }
  const int upper = (int)(hi >> 63);
  const int shift = upper + 64 - 52 - 3;
  uint64_t m = hi >> shift;
  // floor(log2(5^q)) + q + 63: the binary exponent of the product's top bit
  int p2 = (int)(((int64_t)(152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023;
  if (p2 <= 0) {                             // subnormal, or zero
    if (-p2 + 1 >= 64) return 0;
    m >>= -p2 + 1;
    m += m & 1;
    m >>= 1;
    return m;                                // (m == 2^52: the smallest normal, exponent field 1)
  }
  if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;   // a tie
  m += m & 1;
  m >>= 1;
  if (m >= (2ull << 52)) {
    m = 1ull << 52;
    ++p2;
  }
  m &= ~(1ull << 52);
  if (p2 >= 0x7FF) return 0x7FFull << 52;
  return m | ((uint64_t)p2 << 52);
}

// The field get(0) .. get(len - 1).  FS_DEC_SURE: *out is float(text) bit for bit (NaN for the
// empty field); FS_DEC_NOT_MINE: *out is not written.
template <class Get>
FS_DEC_HD inline int fs_dec_parse(const Get& get, uint32_t len, double* out) {
  if (len == 0) {
    *out = fs_dec_bits(0x7FF8ull << 48);
    return FS_DEC_SURE;
  }
  uint32_t i = 0;
  const bool neg = get(0) == '-';
  if (neg) i = 1;
  const uint64_t sign = neg ? 1ull << 63 : 0;
  if (len - i == 3) {
    const int a = get(i), b = get(i + 1), c = get(i + 2);
    if (a == 'i' && b == 'n' && c == 'f') {
      *out = fs_dec_bits(sign | (0x7FFull << 52));
      return FS_DEC_SURE;
    }
    if (!neg && a == 'n' && b == 'a' && c == 'n') {
      *out = fs_dec_bits(0x7FF8ull << 48);
      return FS_DEC_SURE;
    }
  }
  uint64_t w = 0;
  uint32_t nd = 0;          // significant digits
  int64_t e10 = 0;
  bool any = false;
  for (; i < len; ++i) {
    const int c = get(i);
    if (c < '0' || c > '9') break;
    any = true;
    if (w != 0 || c != '0') {
      if (nd < 19) w = w * 10 + (uint64_t)(c - '0');
      ++nd;
    }
  }
  if (!any) return FS_DEC_NOT_MINE;
  if (i < len && get(i) == '.') {
    ++i;
    any = false;
    for (; i < len; ++i) {
      const int c = get(i);
      if (c < '0' || c > '9') break;
      any = true;
      --e10;
      if (w != 0 || c != '0') {
        if (nd < 19) w = w * 10 + (uint64_t)(c - '0');
        ++nd;
      }
    }
    if (!any) return FS_DEC_NOT_MINE;
  }
  if (i < len && (get(i) == 'e' || get(i) == 'E')) {
    ++i;
    bool eneg = false;
    if (i < len && (get(i) == '+' || get(i) == '-')) {
      eneg = get(i) == '-';
      ++i;
    }
    int64_t ev = 0;
    any = false;
    for (; i < len; ++i) {
      const int c = get(i);
      if (c < '0' || c > '9') break;
      any = true;
      if (ev < 100000) ev = ev * 10 + (c - '0');
    }
    if (!any) return FS_DEC_NOT_MINE;
    e10 += eneg ? -ev : ev;
  }
  if (i != len || nd > kDecMaxDigits) return FS_DEC_NOT_MINE;
  uint64_t bits;
  if (w == 0 || e10 < kDecQMin)
    bits = 0;                                // w < 10^17: w * 10^-343 is under half the least subnormal
  else if (e10 > kDecQMax)
    bits = 0x7FFull << 52;
  else
    bits = fs_dec_round(w, (int)e10);
  *out = fs_dec_bits(sign | bits);
  return FS_DEC_SURE;
}

#endif  // FS_DEC_H
