// Sanitizer driver of the step plan (csrc/nrf_step_plan.h; make step_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so):
// step_table into buffers of exactly its capacity and step_land on tables of exactly their length, over the option values the
// render calls meet and the ones they refuse -- every table access of the lower bound must stay inside [0, n) -- and step_land
// against the plain stepping loop for targets around every member, below the start, beyond the table and the non-finite ones.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../csrc/nrf_step_plan.h"

static int g_fail = 0;
static long g_runs = 0;
static void expect(bool ok, const char* what, float a, float b) {
  ++g_runs;
  if (!ok) {
    ++g_fail;
    std::printf("FAILED %s: %.9g %.9g\n", what, (double)a, (double)b);
  }
}

static float loop(float t, float tb, float g, float lo, float hi) {
  while (t < tb) t = nrf::step_next(t, g, lo, hi);
  return t;
}

int main() {
  using namespace nrf;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float NONE = -3.402823466e+38f;
  for (float min_near : {0.0f, 0.05f, 0.2f, 0.5f, 4.0f})
    for (float g : {0.0f, 1.0f / 256, 1.0f / 128, 1.0f / 64, 0.01f})
      for (float bound : {0.5f, 1.0f, 2.0f, 16.0f})
        for (uint32_t H : {30u, 64u, 96u, 128u, 512u})
          for (int capacity : {0, 1, 2, 8, 100, STEP_TABLE_CAPACITY, STEP_TABLE_CAPACITY + 5}) {
            const int room = capacity > STEP_TABLE_CAPACITY ? STEP_TABLE_CAPACITY : capacity;
            std::vector<float> buf((size_t)room);  // (exactly the room: a write beyond it is a finding)
            const int n = step_table(min_near, g, bound, H, capacity, buf.data());
            expect(n >= 0 && n <= room, "length", (float)n, (float)room);
            if (n == 0) continue;
            std::vector<float> tab(buf.begin(), buf.begin() + n);  // (exactly n: a read beyond it is a finding)
            const float lo = step_dt_min(), hi = step_dt_max(bound, H);
            for (int k = 1; k < n; ++k) expect(tab[k] > tab[k - 1], "increasing", tab[k - 1], tab[k]);
            auto check = [&](float t, float tb) {
              const float got = step_land(tab.data(), n, t, tb, g, lo, hi), want = loop(t, tb, g, lo, hi);
              expect(step_bits(got) == step_bits(want), "step_land", t, tb);
            };
            const int stride = n > 64 ? n / 32 : 1;
            for (int k = 0; k < n; k += stride)
              for (float tb : {tab[k], std::nextafter(tab[k], -inf), std::nextafter(tab[k], inf)}) check(tab[0], tb);
            for (float tb : {tab[n - 1], std::nextafter(tab[n - 1], inf), tab[n - 1] + 3.5f * hi, tab[0], 0.0f, -1.0f, nan, -inf, NONE})
              check(tab[0], tb);
            for (float t : {std::nextafter(tab[0], inf), std::nextafter(tab[0], -inf), tab[n / 2], nan, inf})
              for (float tb : {tab[n / 2], tab[n - 1] + hi, nan, NONE}) check(t, tb);
            expect(step_bits(step_land(nullptr, 0, tab[0], tab[n / 2], g, lo, hi)) == step_bits(loop(tab[0], tab[n / 2], g, lo, hi)), "no table", tab[0], tab[n / 2]);
          }
  // refused inputs make no table and write nothing
  float one[2] = {7.0f, 7.0f};
  for (float bad : {nan, -1.0f, inf}) {
    expect(step_table(bad, 0.0f, 1.0f, 128, 2, one) == 0 && one[0] == 7.0f, "refused min_near", bad, one[0]);
    expect(step_table(0.2f, bad, 1.0f, 128, 2, one) == 0 || bad == inf, "refused dt_gamma", bad, one[0]);
    expect(step_table(0.2f, 0.0f, bad == inf ? nan : bad, 128, 2, one) == 0, "refused bound", bad, one[0]);
  }
  expect(step_table(0.2f, 0.0f, 1.0f, 0, 2, one) == 0, "refused H", 0.0f, 0.0f);
  expect(step_table_lds_offset(1000, 600, 160 * 1024) == 1008 && step_table_lds_offset(160 * 1024 - 4095, 1024, 160 * 1024) == -1 &&
             step_table_lds_offset(5000, 0, 160 * 1024) == -1, "lds offset", 0.0f, 0.0f);
  std::printf("step_plan_asan: %ld runs, %d failed\n", g_runs, g_fail);
  return g_fail ? 1 : 0;
}
