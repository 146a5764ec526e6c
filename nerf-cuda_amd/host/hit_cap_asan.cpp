// Sanitizer driver of hit_cap_exponent (csrc/nrf_frame_plan.h; make hit_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so):
// the exponent by which nrf_ray_hits sizes the per-round sample queue, over the thresholds the entry point accepts, the ones it
// refuses and every fp32 neighbour of 0 and 1 -- and the property the kernel relies on: with cap = clamp(exponent(T) - hit_exp, 1, 8)
// halvings a ray at transmittance T gets within one more halving of T <= 1 - opacity (the rule compares exponents and ignores the two
// mantissas, as the rule for T < 1e-4 does), or the cap is the queue's eight.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../csrc/nrf_frame_plan.h"

static int g_fail = 0;
static long g_runs = 0;
static void expect(bool ok, const char* what, float opacity, int got) {
  ++g_runs;
  if (!ok) {
    ++g_fail;
    std::printf("FAILED %s: opacity %.9g -> %d\n", what, (double)opacity, got);
  }
}

int main() {
  using nrf::hit_cap_exponent;
  using nrf::SAMPLE_CAP_EXPONENT;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // the table of tests/test_ray_hits_cpu.py
  expect(hit_cap_exponent(0.5f) == 0, "table", 0.5f, hit_cap_exponent(0.5f));
  expect(hit_cap_exponent(0.9f) == -3, "table", 0.9f, hit_cap_exponent(0.9f));
  expect(hit_cap_exponent(0.99f) == -6, "table", 0.99f, hit_cap_exponent(0.99f));
  expect(hit_cap_exponent(std::nextafter(1.0f, 0.0f)) == SAMPLE_CAP_EXPONENT, "table", std::nextafter(1.0f, 0.0f), hit_cap_exponent(std::nextafter(1.0f, 0.0f)));
  expect(hit_cap_exponent(1.0f) == SAMPLE_CAP_EXPONENT, "table", 1.0f, hit_cap_exponent(1.0f));
  // what the entry point refuses keeps today's rule and raises nothing
  for (float bad : {0.0f, -0.0f, -0.5f, 1.5f, inf, -inf, nan, std::numeric_limits<float>::denorm_min() * -1.0f})
    expect(hit_cap_exponent(bad) == SAMPLE_CAP_EXPONENT, "refused", bad, hit_cap_exponent(bad));
  // a sweep of (0, 1): every fp32 neighbour at both ends, then a coarse walk through the middle
  auto check = [&](float p) {
    const int e = hit_cap_exponent(p);
    expect(e >= SAMPLE_CAP_EXPONENT && e <= 1, "range", p, e);  // (1: a threshold so small that 1 - opacity rounds to 1)
    const float target = 1.0f - p;  // the ray stops at T <= target
    for (float T : {1.0f, 0.75f, 0.5f, 0.3f, 0.01f, 1e-3f}) {
      if (!(T > target)) continue;
      int te = 0;
      (void)std::frexp(T, &te);
      const int cap = std::min(std::max(te - e, 1), 8);
      expect(cap == 8 || std::ldexp(T, -(cap + 1)) <= target || e == SAMPLE_CAP_EXPONENT, "enough samples", p, cap);
    }
  };
  float p = std::numeric_limits<float>::denorm_min();
  for (int i = 0; i < 4096; ++i, p = std::nextafter(p, 1.0f)) check(p);
  p = std::nextafter(1.0f, 0.0f);
  for (int i = 0; i < 4096; ++i, p = std::nextafter(p, 0.0f)) check(p);
  for (int i = 1; i < 100000; ++i) check((float)i / 100000.0f);
  // monotone: a higher threshold never gets a higher exponent
  int last = 1;
  for (int i = 1; i < 100000; ++i) {
    const int e = hit_cap_exponent((float)i / 100000.0f);
    expect(e <= last, "monotone", (float)i / 100000.0f, e);
    last = e;
  }
  std::printf("hit_cap_asan: %ld runs, %d failed\n", g_runs, g_fail);
  return g_fail ? 1 : 0;
}
