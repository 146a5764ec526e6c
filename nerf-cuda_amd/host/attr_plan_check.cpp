// Sanitizer driver of csrc/nrf_attr_plan.h (make attr_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the arithmetic of
// the point attributes (nrf_point_attributes, nrf_mesh_attributes) from a gradient record to the unit direction, the normal and the
// length, and the 8-bit rule of an exported colour, compiled from the text the kernel compiles.  Rows of three fp32 bit patterns
// (hexadecimal) on stdin,
//     g_x g_y g_z
// and one line per row on stdout:
//     n[3] len d[3] as bit patterns, ok (0 / 1), the three direction inputs 0.5 d_k + 0.5 as bit patterns, and the 8-bit values of the
//     row's three words read as a colour (decimal)
// tests/test_point_attributes_cpu.py holds the output to the numpy replay the GPU tests use.  Built with -ffp-contract=off, as the
// library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../csrc/nrf_attr_plan.h"

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
    uint32_t w[3];
    int got = 0;
    for (; got < 3; ++got)
      if (std::scanf("%" SCNx32, &w[got]) != 1) break;
    if (got == 0) break;
    if (got != 3) {
      std::fprintf(stderr, "attr_plan_check: row %ld has %d of 3 words\n", rows, got);
      return 2;
    }
    const float g[3] = {as_float(w[0]), as_float(w[1]), as_float(w[2])};
    float d[3], n[3], len;
    const bool ok = nrf::attr_direction(g[0], g[1], g[2], d, n, len);
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d ", as_bits(n[0]),
                as_bits(n[1]), as_bits(n[2]), as_bits(len), as_bits(d[0]), as_bits(d[1]), as_bits(d[2]), (int)ok);
    std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " ", as_bits(nrf::attr_dir01(d[0])), as_bits(nrf::attr_dir01(d[1])),
                as_bits(nrf::attr_dir01(d[2])));
    std::printf("%u %u %u\n", (unsigned)nrf::attr_color_u8(g[0]), (unsigned)nrf::attr_color_u8(g[1]), (unsigned)nrf::attr_color_u8(g[2]));
    ++rows;
  }
  std::fprintf(stderr, "attr_plan_check: %ld rows\n", rows);
  return 0;
}
