// The arithmetic of COCO's compressed RLE string (refer/external/maskApi.c:203-216 rleToString, :217-230 rleFrString;
// gtmask.cpp hgl_rle_to_string / parse_rle_string are the sequential host forms and the yardstick), written so that every
// count and every character group stands alone: plain functions that compile under g++ (the sanitizer harness
// tests/native/rle_string_walk_sanitize.cpp) and as __device__ code (rle_string.hip).  Nothing here needs HIP when __HIPCC__
// is absent.
//
//   Delta        x_i = counts[i] - (i > 2 ? counts[i-2] : 0) as a signed 64-bit value, in (-2^32, 2^32).
//   Length       x >= 0 takes the smallest k >= 1 with x < 2^(5k-1); x < 0 the smallest k >= 1 with x >= -2^(5k-1).
//                k <= 7, and 7 is reached by +-(2^32 - 1).
//   Characters   character j of the group is 48 + ((x >> 5j) & 31) + (j < k-1 ? 32 : 0), the shift arithmetic.
//   Reading      c = (uint8)(b - 48); only c & 31 and c & 32 are read, so bytes >= 112 are accepted as the host accepts them.
//                A byte with c & 32 == 0 ends a group.
//   Value        a group of k <= 7 characters is the sum of (c_j & 31) << 5j, sign-extended from bit 5k-1 when the last
//                character has bit 16 set; only the low 32 bits are ever used.
//   Un-delta     counts[0] = x_0; the odd indices are the running sum of x_1, x_3, ...; the even indices FROM 2 ON are the
//                running sum of x_2, x_4, ...: counts[2] does not add counts[0].  All sums modulo 2^32.
//   Refusals     the first offending group in string order decides: LONG when an eighth character of the group exists in the
//                string, TRUNCATED when the string ends inside a group of at most seven characters.  A long group lies before
//                the end of the string, so: any long group -> long; else a last byte that continues -> truncated.
#ifndef HGL_RLE_STRING_H
#define HGL_RLE_STRING_H
#include <stdint.h>

#ifdef __HIPCC__
#define RSTR_FN static __host__ __device__ inline
#else
#define RSTR_FN static inline
#endif

constexpr int RSTR_MAX_GROUP = 7;      // characters of the longest group: 5*7 = 35 bits hold a signed 33-bit difference

// the difference that stands for counts[i] in the string
RSTR_FN long long rstr_delta(const uint32_t* counts, long long i) {
  return (long long)counts[i] - (i > 2 ? (long long)counts[i - 2] : 0ll);
}

// the characters of the group of x (|x| < 2^32): 1 .. 7
RSTR_FN int rstr_length(long long x) {
  const unsigned long long y = (unsigned long long)(x < 0 ? ~x : x);      // x >= -2^(5k-1)  <=>  ~x < 2^(5k-1)
  int k = 1;
  while (k < RSTR_MAX_GROUP && (y >> (5 * k - 1)) != 0ull) ++k;
  return k;
}

// character j < k of the group of x
RSTR_FN uint8_t rstr_char(long long x, int j, int k) {
  return (uint8_t)(48u + ((unsigned)(x >> (5 * j)) & 31u) + (j < k - 1 ? 32u : 0u));      // x >> n: arithmetic (C++20; every compiler before)
}

// a byte of a string: its 5 payload bits, whether the group goes on behind it, whether it carries the sign as a last character
RSTR_FN unsigned rstr_digit(uint8_t b) { return (unsigned)(uint8_t)(b - 48u) & 31u; }
RSTR_FN bool rstr_more(uint8_t b) { return ((unsigned)(uint8_t)(b - 48u) & 32u) != 0u; }
RSTR_FN bool rstr_sign(uint8_t b) { return ((unsigned)(uint8_t)(b - 48u) & 16u) != 0u; }

// the low 32 bits of the value of the group g[0 .. k-1], 1 <= k <= 7, g[k-1] the byte that ends it
RSTR_FN uint32_t rstr_group_value(const uint8_t* g, int k) {
  unsigned long long ux = 0;
  for (int j = 0; j < k; ++j) ux |= (unsigned long long)rstr_digit(g[j]) << (5 * j);
  if (rstr_sign(g[k - 1])) ux |= ~0ull << (5 * k);      // 5k <= 35
  return (uint32_t)ux;
}

// the characters of the group that the byte at s[p] ends (it does not continue), in a string that begins at s[0]: the group
// reaches back over the bytes that continue, at most RSTR_MAX_GROUP - 1 of them in a string without a long group
RSTR_FN int rstr_group_length(const uint8_t* s, long long p) {
  int k = 1;
  while (k < RSTR_MAX_GROUP && p - k >= 0 && rstr_more(s[p - k])) ++k;
  return k;
}

// the byte at s[p] is the eighth (or a later) character of its group: the seven bytes before it all continue
RSTR_FN bool rstr_long_at(const uint8_t* s, long long p) {
  if (p < RSTR_MAX_GROUP) return false;
  for (int j = 1; j <= RSTR_MAX_GROUP; ++j)
    if (!rstr_more(s[p - j])) return false;
  return true;
}

// what x_i adds to the running sum of its parity: x_0 stands alone, it is counts[0] and no later count adds it
RSTR_FN uint32_t rstr_chain_term(long long i, uint32_t x) { return i == 0 ? 0u : x; }

// The un-delta of the stretch v[0 .. n) that holds x_(i0) .. x_(i0+n-1), in place, sequentially: carry[0] / carry[1] are the
// running sums of the even / odd chain before i0 (0, 0 before the first stretch) and are moved behind the stretch.  The form
// that the kernel's stride-2 scan is held against, at either parity of i0.
RSTR_FN void rstr_undelta_stretch(uint32_t* v, long long i0, long long n, uint32_t carry[2]) {
  for (long long j = 0; j < n; ++j) {
    const long long i = i0 + j;
    carry[i & 1] += rstr_chain_term(i, v[j]);
    if (i != 0) v[j] = carry[i & 1];
  }
}

#endif  // HGL_RLE_STRING_H
