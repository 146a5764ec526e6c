// nrf_points_plan.h -- the arithmetic of the point queries (nrf_density, nrf_density_gradient, nrf_hit_gradients) without a device:
// the taps of the central differences, the guard that decides whether a point is evaluated at all, the position of a hit record
// on its ray and the host's 1 / (2 h).  points_kernel (nrf_kernels_points.hip) and host/points_plan_check.cpp compile this text,
// so the kernel's definition and the tests' replay are one.  Every operation is ONE fp32 rounding: the library is built with
// -ffp-contract=off -fno-fast-math, and a host build of this header has to be (host/Makefile: points_asan).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NRF_POINTS_HD __host__ __device__
#else
#define NRF_POINTS_HD
#endif

namespace nrf {

// what a launch of points_kernel computes
enum : int { POINTS_VALUE = 0, POINTS_GRADIENT = 1, POINTS_HIT_GRADIENT = 2 };
constexpr int POINTS_GRADIENT_TAPS = 7;  // the centre, then +x, -x, +y, -y, +z, -z
NRF_POINTS_HD constexpr int points_taps(int mode) { return mode == POINTS_VALUE ? 1 : POINTS_GRADIENT_TAPS; }

// Tap `tap` of the point x: the point with ONE coordinate replaced by x_k + h (tap 1 + 2 k) or x_k - h (tap 2 + 2 k); tap 0 is x.
// (selects, no indexing by `tap`: the kernel's tap loop is not unrolled and its registers must stay registers)
NRF_POINTS_HD inline void points_tap(const float (&x)[3], float h, int tap, float (&out)[3]) {
  out[0] = tap == 1 ? x[0] + h : (tap == 2 ? x[0] - h : x[0]);
  out[1] = tap == 3 ? x[1] + h : (tap == 4 ? x[1] - h : x[1]);
  out[2] = tap == 5 ? x[2] + h : (tap == 6 ? x[2] - h : x[2]);
}

// A coordinate may become an address only if it is finite and inside the box: |v| <= bound is false for NaN and, the bound being
// finite, for +-inf.  No clamping.
NRF_POINTS_HD inline bool points_in_box(float v, float bound) { return __builtin_fabsf(v) <= bound; }

// The guard: a point is evaluated if and only if every coordinate of every one of its taps is in the box (n_taps == 1: the centre
// alone; otherwise the seven taps of points_tap).  A refused point's outputs are 0 and none of its taps is gathered.
NRF_POINTS_HD inline bool points_guard(const float (&x)[3], float h, float bound, int n_taps) {
  bool ok = points_in_box(x[0], bound) && points_in_box(x[1], bound) && points_in_box(x[2], bound);
  if (n_taps > 1) {
    ok = ok && points_in_box(x[0] + h, bound) && points_in_box(x[0] - h, bound);
    ok = ok && points_in_box(x[1] + h, bound) && points_in_box(x[1] - h, bound);
    ok = ok && points_in_box(x[2] + h, bound) && points_in_box(x[2] - h, bound);
  }
  return ok;
}

// One component of the gradient from the sigmas of its two taps
NRF_POINTS_HD inline float points_difference(float s_plus, float s_minus, float inv2h) {
  const float d = s_plus - s_minus;
  return d * inv2h;
}

// Whether pixel p of a view is a hit of an nrf_ray_hits frame: it has a ray and its weight sum reached the threshold (the fp32
// compare nrf_ray_hits documents)
NRF_POINTS_HD inline bool points_is_hit(uint32_t p, uint32_t rays_per_view, float ws1, float opacity) {
  return p < rays_per_view && ws1 >= opacity;
}

// Where a hit record (t, dt) puts the query on the ray o + t d: tq = t - frac * dt (frac 1: the start of the crossing sample's
// interval, 0: its end), x = o + tq d.  out = (x, y, z, tq).
NRF_POINTS_HD inline void hit_position(const float (&o)[3], const float (&d)[3], float t, float dt, float frac, float (&out)[4]) {
  const float back = frac * dt;
  const float tq = t - back;
  const float sx = tq * d[0], sy = tq * d[1], sz = tq * d[2];
  out[0] = o[0] + sx;
  out[1] = o[1] + sy;
  out[2] = o[2] + sz;
  out[3] = tq;
}

// ---- the host's side ----
// 1 / (2 h), computed once per call and handed to the kernel
inline float points_inv2h(float h) { return 1.0f / (h + h); }
// the step the entry points accept: finite, > 0, <= bound (NaN fails both compares; +inf the second, the bound being finite)
inline bool points_step_valid(float h, float bound) { return h > 0.0f && h <= bound; }
inline bool points_frac_valid(float frac) { return frac >= 0.0f && frac <= 1.0f; }
inline bool points_opacity_valid(float opacity) { return opacity > 0.0f && opacity <= 1.0f; }

}  // namespace nrf
