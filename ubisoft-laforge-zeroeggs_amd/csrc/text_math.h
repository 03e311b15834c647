// Exact "%f" of a double in integer arithmetic, for the BVH motion text (csrc/text.hip on the device, tests/host/text_format_check.cpp
// on the host: no HIP include is needed, the qualifiers sit behind ZT_HD).  Same bytes as glibc's snprintf("%f") for every finite
// |x| < 1e15 -- the domain for which a number with its sign and separator is at most ZT_MAX_WIDTH = 24 bytes wide.
//
// x = m * 2^e from the bits (subnormals: e = -1074, no hidden bit).  In the domain e <= -3 always (m >= 2^52 for normals), so with
// k = -e the integer part is m >> k and the six decimals are round_half_even(f * 15625 / 2^(k - 6)), f = m mod 2^k (10^6 =
// 15625 * 2^6).  f * 15625 < 2^67 is kept in two 64-bit words, the tie is decided on the exact remainder, and a carry out of the
// decimals (0.9999995 -> 1.000000) goes into the integer part.  10^6 is even, so the parity that breaks the tie is the decimals' own.
#pragma once
#include <stdint.h>

#ifndef ZT_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZT_HD __host__ __device__ inline
#else
#define ZT_HD inline
#endif
#endif

#define ZT_MAX_WIDTH 24                          // '-' + 15 digits + '.' + 6 decimals + ' '
#define ZT_BITS_1E15 0x430C6BF526340000ULL       // the bits of 1e15 (exact in binary64): non-negative doubles order as their bits

struct ZtNum {
  uint64_t ip;      // integer digits, < 10^15
  uint32_t frac;    // the six decimals, < 10^6
  int neg;          // sign bit: "-0.000000" for -0.0 and -4e-7, as glibc
  int ok;           // 0: out of the domain (NaN, +-inf, |x| >= 1e15) -- ip = frac = neg = 0 then ("0.000000": a placeholder)
};

ZT_HD ZtNum zt_decompose(uint64_t bits) {
  ZtNum n;
  n.ip = 0; n.frac = 0; n.neg = 0; n.ok = 0;
  const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFULL;
  if (mag >= ZT_BITS_1E15) return n;             // (NaN and inf have larger bit patterns than any finite value)
  n.ok = 1;
  n.neg = (int)(bits >> 63);
  const int E = (int)(mag >> 52);
  const uint64_t m = (mag & 0x000FFFFFFFFFFFFFULL) | (E ? 0x0010000000000000ULL : 0);
  const int k = 1075 - (E ? E : 1);              // x = m / 2^k, 3 <= k <= 1074
  uint64_t f = m;
  if (k < 53) { n.ip = m >> k; f = m & ((1ULL << k) - 1); }
  if (k <= 6) { n.frac = (uint32_t)(f * 15625u) << (6 - k); return n; }      // (f < 2^6: exact)
  const int r = k - 6;                           // decimals = round_half_even(P / 2^r), P = f * 15625 < 2^67
  if (r >= 70) return n;                         // P / 2^r < 1/8
  const uint64_t a = (f >> 32) * 15625u, b = (f & 0xFFFFFFFFULL) * 15625u;   // P = a * 2^32 + b, a < 2^35, b < 2^46
  const uint64_t lo = (a << 32) + b;
  const uint64_t hi = (a >> 32) + (lo < b ? 1 : 0);
  uint64_t q;
  bool above, tie;                               // the remainder against half a unit of the last decimal
  if (r < 64) {
    q = (lo >> r) | (hi ? hi << (64 - r) : 0);   // (the quotient is < 10^6: whatever hi holds fits)
    const uint64_t rem = lo & ((1ULL << r) - 1), half = 1ULL << (r - 1);
    above = rem > half; tie = rem == half;
  } else {
    const int s = r - 64;                        // 0 .. 5
    q = hi >> s;
    const uint64_t rem_hi = hi & ((1ULL << s) - 1);
    if (s == 0) { above = lo > (1ULL << 63); tie = lo == (1ULL << 63); }
    else { const uint64_t half_hi = 1ULL << (s - 1); above = rem_hi > half_hi || (rem_hi == half_hi && lo != 0); tie = rem_hi == half_hi && lo == 0; }
  }
  q += (above || (tie && (q & 1))) ? 1 : 0;
  if (q >= 1000000u) { q -= 1000000u; n.ip += 1; }
  n.frac = (uint32_t)q;
  return n;
}

ZT_HD int zt_ndigits(uint64_t ip) {              // ip < 10^15 (+ 1 after a carry: 10^15 itself cannot occur, 999999999999999.9 < 1e15 rounds
  int nd = 1;                                    // within its decimals: the spacing of doubles there is 0.125)
  if (ip >= 100000000ULL) { ip /= 100000000ULL; nd += 8; }
  uint32_t v = (uint32_t)ip;
  if (v >= 10000u) { v /= 10000u; nd += 4; }
  if (v >= 100u) { v /= 100u; nd += 2; }
  if (v >= 10u) nd += 1;
  return nd;
}

// bytes of "%f" + the separator behind it
ZT_HD int zt_width(const ZtNum& n) { return n.neg + zt_ndigits(n.ip) + 8; }

// the characters of "%f" (no separator, no NUL) -> out[0 .. return value); an out-of-domain number gives its placeholder
template <class Out>
ZT_HD int zt_put(const ZtNum& n, Out out) {
  int p = 0;
  if (n.neg) out[p++] = '-';
  const int nd = zt_ndigits(n.ip);
  uint32_t hi = (uint32_t)(n.ip / 100000000ULL), lo = (uint32_t)(n.ip % 100000000ULL);      // hi < 10^7
  for (int i = nd - 1; i >= 0; --i) {
    uint32_t& w = nd - 1 - i >= 8 ? hi : lo;   // (the last eight digits come from lo)
    out[p + i] = (char)('0' + w % 10u);
    w /= 10u;
  }
  p += nd;
  out[p++] = '.';
  uint32_t f = n.frac;
  for (int i = 5; i >= 0; --i) { out[p + i] = (char)('0' + f % 10u); f /= 10u; }
  return p + 6;
}

// "%f" of the double with these bits -> out (at most ZT_MAX_WIDTH - 1 characters, no NUL); 0 and nothing written when it is out of
// the domain
ZT_HD int zt_format(uint64_t bits, char* out) {
  const ZtNum n = zt_decompose(bits);
  return n.ok ? zt_put(n, out) : 0;
}
