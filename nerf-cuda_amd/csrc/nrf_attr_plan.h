// nrf_attr_plan.h -- the arithmetic of the point attributes (nrf_point_attributes, nrf_mesh_attributes) without a device: from the
// gradient record (g_x, g_y, g_z) of nrf_density_gradient -- the taps, the guard and points_difference of nrf_points_plan.h -- to
// the unit direction d = g / |g| along which a viewer meets the surface head-on and the outward normal n = -d, and the library's
// 8-bit rule for an exported colour.  attr_kernel (nrf_kernels_attr.hip) and host/attr_plan_check.cpp compile this text, so the
// kernel's definition and the tests' replay are one.  Every operation is ONE fp32 rounding, the square root and the division the
// correctly rounded IEEE ones: the library is built with -ffp-contract=off -fno-fast-math and hipcc's correctly rounded fp32
// divide and sqrt (its default), and a host build of this header has to be (host/Makefile: attr_asan).
#pragma once
#include <cstdint>

#include "nrf_points_plan.h"

namespace nrf {

// Below this squared length a gradient counts as none: 2^-60.  A product below 2^-126 (where a denormal mode could matter) can
// never change a sum that is at least 2^-60, so `ok` and everything after it do not depend on the denormal mode.
constexpr float ATTR_L2_FLOOR = 0x1p-60f;

// l2 = (g_x g_x + g_y g_y) + g_z g_z: three products, two sums, in this order
NRF_POINTS_HD inline float attr_length2(float gx, float gy, float gz) {
  const float xx = gx * gx, yy = gy * gy, zz = gz * gz;
  const float xy = xx + yy;
  return xy + zz;
}

// whether the gradient has a direction: l2 is finite (not NaN, not inf after an overflow of the squares) and at least the floor
NRF_POINTS_HD inline bool attr_length2_ok(float l2) { return l2 >= ATTR_L2_FLOOR && l2 <= 3.402823466e+38f; }

// From the gradient to (d, n, len).  A degenerate point has len = 0 and d = n = (+0, +0, +0); otherwise len = sqrt(l2),
// d_k = g_k / len and n_k = -d_k (exact).  Returns ok.
NRF_POINTS_HD inline bool attr_direction(float gx, float gy, float gz, float (&d)[3], float (&n)[3], float& len) {
  const float l2 = attr_length2(gx, gy, gz);
  const bool ok = attr_length2_ok(l2);
  len = ok ? __builtin_sqrtf(l2) : 0.0f;
  d[0] = ok ? gx / len : 0.0f;
  d[1] = ok ? gy / len : 0.0f;
  d[2] = ok ? gz / len : 0.0f;
  n[0] = ok ? -d[0] : 0.0f;
  n[1] = ok ? -d[1] : 0.0f;
  n[2] = ok ? -d[2] : 0.0f;
  return ok;
}

// What the network is given for a direction component (nerf_render.cu:313-314, as network_kernel forms it): 0.5 d_k, then + 0.5
NRF_POINTS_HD inline float attr_dir01(float dk) {
  const float u = 0.5f * dk;
  return u + 0.5f;
}

// The library's 8-bit rule (quant_u8 of nrf_render.h, nrf_quantize_u8 / nrf_read_u8): (unsigned char)(255.0 * x) with the product
// in double, saturating, NaN -> 0
NRF_POINTS_HD inline uint8_t attr_color_u8(float v) {
  const double s = 255.0 * (double)v;
  if (!(s > 0.0)) return 0;
  if (s >= 255.0) return 255;
  return (uint8_t)s;
}

}  // namespace nrf
