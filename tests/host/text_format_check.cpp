// csrc/text_math.h against glibc's snprintf("%f"): every value class the BVH motion text can meet, byte for byte, on the host.
// Usage: text_format_check [values per class, default 2000000].  Prints "text_format_check: ok" when nothing differs.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../ubisoft-laforge-zeroeggs_amd/csrc/text_math.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {      // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static double unit() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
static double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
static uint64_t to_bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }

static long g_checked = 0, g_bad = 0;

static bool in_domain(double x) { return isfinite(x) && fabs(x) < 1e15; }

static void check(double x, const char* cls) {
  char want[400], got[ZT_MAX_WIDTH + 8];
  ++g_checked;
  memset(got, '#', sizeof got);
  const int n = zt_format(to_bits(x), got);
  const ZtNum d = zt_decompose(to_bits(x));
  bool ok;
  if (!in_domain(x)) {
    ok = n == 0 && d.ok == 0 && got[0] == '#' && zt_width(d) == 9;      // reported, nothing emitted, placeholder "0.000000 "
    want[0] = 0;
  } else {
    const int w = snprintf(want, sizeof want, "%f", x);
    ok = d.ok == 1 && n == w && memcmp(want, got, (size_t)w) == 0 && got[n] == '#' && zt_width(d) == w + 1 && w + 1 <= ZT_MAX_WIDTH;
  }
  if (!ok && g_bad++ < 20) {
    got[n >= 0 && n < ZT_MAX_WIDTH ? n : 0] = 0;
    fprintf(stderr, "%s: x = %.17g (bits %016llx): snprintf \"%s\", text_math \"%s\" (%d)\n", cls, x, (unsigned long long)to_bits(x),
            want, got, n);
  }
}

int main(int argc, char** argv) {
  const long N = argc > 1 ? atol(argv[1]) : 2000000;
  // fixed values: signs of zero, carries, ties, the ends of the domain and everything outside it
  const double fixed[] = {0.0, -0.0, 4e-7, -4e-7, 5e-7, -5e-7, 0.9999995, 9.9999995, -99.9999995, 0.0078125, 5e-324, -5e-324,
                          2.2250738585072014e-308, 999999999999999.9, -999999999999999.9, 999999999999999.875, 0.5, 1.5, 2.5,
                          1e-6, 1.5e-6, 2.5e-6, 0.0000005, 0.0000015, 0.0000025, 1.0, 10.0, 123456789012345.0, 99999999.9999995,
                          100000000.0, 99999999.0, 0.1, 0.2, 0.3, 1e14, 562949953421311.9, 1125899906842623.0 / 2,
                          NAN, -NAN, INFINITY, -INFINITY, 1e15, -1e15, 1e300, -1e300, 1.7976931348623157e308, nextafter(1e15, 2e15)};
  for (double x : fixed) check(x, "fixed");
  if (zt_width(zt_decompose(to_bits(-999999999999999.9))) != 24 || !zt_decompose(to_bits(999999999999999.9)).ok) {
    fprintf(stderr, "-999999999999999.9 must be in the domain and 24 bytes wide with its sign and separator\n");
    ++g_bad;
  }
  const double outside[] = {NAN, INFINITY, -INFINITY, 1e15, -1e15, 1e300};
  for (double x : outside)
    if (zt_decompose(to_bits(x)).ok) { fprintf(stderr, "%g must be out of the domain\n", x); ++g_bad; }
  for (long i = 0; i < N; ++i) {
    check(from_bits(rnd()), "random bits");                                                   // (most are out of the domain)
    check(from_bits((rnd() & 0x800FFFFFFFFFFFFFULL) | ((uint64_t)(900 + rnd() % 173) << 52)), "random bits in the domain");
    check((unit() - 0.5) * 720.0, "degrees");
    check((double)(float)((unit() - 0.5) * 400.0), "float32 origin");
    check((double)(float)((unit() - 0.5) * 2.0) * (double)(float)(180.0 / 3.14159265358979), "float32 product");
    const long k = (long)(rnd() % 4000001) - 2000000;
    check((double)k / 128.0, "ties k/128");
    check(ldexp((double)k, -7 - (int)(rnd() % 20)), "ties k * 2^-7..-26");
    check(((double)k + 0.5) * 1e-6, "(k + 0.5) * 1e-6");
    check(nextafter(((double)k + 0.5) * 1e-6, (rnd() & 1) ? 1e9 : -1e9), "next to (k + 0.5) * 1e-6");
    check((double)(k / 1000) + (k < 0 ? -0.9999995 : 0.9999995), "carries");
    check(from_bits((rnd() & 0x800FFFFFFFFFFFFFULL)), "subnormals");
    check(from_bits((rnd() & 0x800FFFFFFFFFFFFFULL) | ((uint64_t)(1 + rnd() % 1000) << 52)), "tiny normals");
    check(ldexp(unit(), (int)(rnd() % 51)) * ((rnd() & 1) ? 1.0 : -1.0), "up to 2^50");
    check((double)(int64_t)(rnd() % 1000000000000000ULL) + (double)(rnd() % 8) * 0.125, "large with eighths");
  }
  if (g_bad) {
    fprintf(stderr, "text_format_check: %ld of %ld values differ\n", g_bad, g_checked);
    return 1;
  }
  printf("checked %ld values\ntext_format_check: ok\n", g_checked);
  return 0;
}
