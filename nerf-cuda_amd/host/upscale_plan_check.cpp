// Sanitizer driver of csrc/nrf_upscale_plan.h (make upscale_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the definition
// of the render buffer's upscaler (nrf_rb_upscale) -- the geometry, the Catmull-Rom weights, the reconstruction with its de-ringing clamp,
// the clamped unsharp mask and the packed pixel -- compiled from the text the kernel compiles.  One case on stdin:
//     in_width in_height out_width out_height (decimal)  amount (fp32 bit pattern, hexadecimal)
//     in_height * in_width texels of four fp32 bit patterns (hexadecimal), row-major
// and on stdout:
//     plan 0               the resolutions or the amount are out of range
//     plan 1 rx ry         the bits of the two ratios
//     r g b a rgba8        one line per output texel, row-major: the bits of the four channels and the packed dword
// tests/test_upscale_cpu.py holds the output to the numpy replay the GPU tests use (tests/upscale_replay.py).  Built with
// -ffp-contract=off, as the library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_upscale_plan.h"

struct Texel {
  float x, y, z, w;
};

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
  int iw, ih, ow, oh;
  uint32_t amount_bits;
  if (std::scanf("%d %d %d %d %" SCNx32, &iw, &ih, &ow, &oh, &amount_bits) != 5) {
    std::fprintf(stderr, "upscale_plan_check: no header\n");
    return 2;
  }
  nrf::UpscalePlan P;
  if (!nrf::upscale_plan(iw, ih, ow, oh, as_float(amount_bits), P)) {
    std::printf("plan 0\n");
    return 0;
  }
  if ((int64_t)ow * oh > (1 << 22)) {
    std::fprintf(stderr, "upscale_plan_check: more than 2^22 output texels\n");
    return 2;
  }
  std::vector<Texel> src((size_t)iw * ih);
  for (Texel& t : src) {
    uint32_t u[4];
    if (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &u[0], &u[1], &u[2], &u[3]) != 4) return 2;
    t = {as_float(u[0]), as_float(u[1]), as_float(u[2]), as_float(u[3])};
  }
  std::printf("plan 1 %08" PRIx32 " %08" PRIx32 "\n", as_bits(P.rx), as_bits(P.ry));
  // stage 1: the plane U
  std::vector<Texel> U((size_t)ow * oh);
  for (int Y = 0; Y < oh; ++Y) {
    int iy, cy[4];
    float fy, wy[4];
    nrf::upscale_source(Y, P.ry, iy, fy);
    nrf::upscale_taps(iy, ih, cy);
    nrf::upscale_weights(fy, wy);
    for (int X = 0; X < ow; ++X) {
      int ix, cx[4];
      float fx, wx[4];
      nrf::upscale_source(X, P.rx, ix, fx);
      nrf::upscale_taps(ix, iw, cx);
      nrf::upscale_weights(fx, wx);
      if (!(fx >= 0.0f && fx < 1.0f && fy >= 0.0f && fy < 1.0f)) {
        std::fprintf(stderr, "upscale_plan_check: a fraction outside [0, 1) at (%d, %d)\n", X, Y);
        return 3;
      }
      const auto at = [&](int j, int a) -> const Texel& { return src.at((size_t)cy[j] * iw + cx[a]); };
      Texel h[4];
      for (int j = 0; j < 4; ++j) h[j] = nrf::upscale_row(wx, at(j, 0), at(j, 1), at(j, 2), at(j, 3));
      U[(size_t)Y * ow + X] = nrf::upscale_column(wy, h[0], h[1], h[2], h[3], at(1, 1), at(1, 2), at(2, 1), at(2, 2));
    }
  }
  // stage 2 and the packed pixel
  for (int Y = 0; Y < oh; ++Y)
    for (int X = 0; X < ow; ++X) {
      const int n = nrf::upscale_clamp_index(Y - 1, oh), s = nrf::upscale_clamp_index(Y + 1, oh);
      const int w = nrf::upscale_clamp_index(X - 1, ow), e = nrf::upscale_clamp_index(X + 1, ow);
      const Texel o = nrf::upscale_sharpen(U.at((size_t)Y * ow + X), U.at((size_t)n * ow + X), U.at((size_t)s * ow + X), U.at((size_t)Y * ow + w),
                                           U.at((size_t)Y * ow + e), P.amount);
      std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", as_bits(o.x), as_bits(o.y), as_bits(o.z), as_bits(o.w),
                  nrf::upscale_rgba8(o));
    }
  std::fprintf(stderr, "upscale_plan_check: %d x %d -> %d x %d, %zu texels\n", iw, ih, ow, oh, U.size());
  return 0;
}
