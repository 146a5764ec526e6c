// Sanitizer driver of csrc/nrf_points_plan.h (make points_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the tap,
// guard and hit-position arithmetic of the point kernels (nrf_density, nrf_density_gradient, nrf_hit_gradients), compiled from the
// text the kernels compile.  Rows of fourteen fp32 bit patterns (hexadecimal) on stdin,
//     x[3] h bound o[3] d[3] t dt frac
// and one line per row on stdout, bit patterns again:
//     the 7 taps (21 words), guard of the centre alone, guard of the seven taps, the hit position (x, y, z, tq), inv2h,
//     h / frac valid (2 words)
// tests/test_density_points_cpu.py holds the output to the numpy replay the GPU tests use.  Built with -ffp-contract=off, as the
// library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../csrc/nrf_points_plan.h"

static float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}
static uint32_t as_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  long rows = 0;
  for (;;) {
    uint32_t w[14];
    int got = 0;
    for (; got < 14; ++got)
      if (std::scanf("%" SCNx32, &w[got]) != 1) break;
    if (got == 0) break;
    if (got != 14) {
      std::fprintf(stderr, "points_plan_check: row %ld has %d of 14 words\n", rows, got);
      return 2;
    }
    const float x[3] = {as_float(w[0]), as_float(w[1]), as_float(w[2])};
    const float h = as_float(w[3]), bound = as_float(w[4]);
    const float o[3] = {as_float(w[5]), as_float(w[6]), as_float(w[7])};
    const float d[3] = {as_float(w[8]), as_float(w[9]), as_float(w[10])};
    const float t = as_float(w[11]), dt = as_float(w[12]), frac = as_float(w[13]);
    for (int tap = 0; tap < nrf::POINTS_GRADIENT_TAPS; ++tap) {
      float p[3];
      nrf::points_tap(x, h, tap, p);
      std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " ", as_bits(p[0]), as_bits(p[1]), as_bits(p[2]));
    }
    std::printf("%d %d ", (int)nrf::points_guard(x, h, bound, nrf::points_taps(nrf::POINTS_VALUE)),
                (int)nrf::points_guard(x, h, bound, nrf::points_taps(nrf::POINTS_GRADIENT)));
    float q[4];
    nrf::hit_position(o, d, t, dt, frac, q);
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " ", as_bits(q[0]), as_bits(q[1]), as_bits(q[2]), as_bits(q[3]));
    std::printf("%08" PRIx32 " %d %d\n", as_bits(nrf::points_inv2h(h)), (int)nrf::points_step_valid(h, bound), (int)nrf::points_frac_valid(frac));
    ++rows;
  }
  std::fprintf(stderr, "points_plan_check: %ld rows\n", rows);
  return 0;
}
