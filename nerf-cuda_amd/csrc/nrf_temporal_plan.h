// nrf_temporal_plan.h -- the definition of the render buffer's temporal upscaler (nrf_rb_upscale_temporal) and of the motion vectors of a
// static scene (nrf_motion_vectors) without a device.  It builds on nrf_upscale_plan.h: the same geometry, taps, weights, reconstruction,
// sharpening and packed pixel.  temporal_kernel / motion_kernel (nrf_kernels_temporal.hip) and host/temporal_plan_check.cpp compile this
// text and nothing else does, so the kernels' definition and the tests' replay (tests/temporal_replay.py) are one.  Every fp32 operation is
// ONE rounding with no contraction, division is the correctly rounded IEEE one, every integer operation is exact, and there is no
// transcendental function.  No HIP types: a texel is any type with float members x, y, z, w.
//
//   planes     P [IH][IW] texels: the developed surface nrf_rb_upscale reads.  The history colour H [OH][OW] texels (never sharpened) and
//              the history weight Wt [OH][OW] float exist twice, previous and current, swapped after each call.  The presented plane
//              [OH][OW] is the upscaled plane.
//   jitter     j = (jx, jy), each finite and in [-0.5, 0.5]: the sample of render pixel (x, y) was taken at (x + 0.5 + jx, y + 0.5 + jy) in
//              render pixels.  A pinhole frame gets that by rendering with cam = (fl_x, fl_y, cx - jx, cy - jy).
//   source     per axis: s = upscale_source's s - j (one more rounded subtraction), i = (int)floorf(s), f = s - (float)i (rounded: it may
//              reach 1).  Taps and weights are upscale_taps / upscale_weights of i and f.
//   current    C = stage 1 of the spatial upscaler (upscale_row, upscale_column, the de-ringing clamp) at this s; with j = (0, 0) it is the
//              spatial upscaler's U bit for bit.
//   weight     per axis: n = clamp((int)floorf(s + 0.5f), 0, I - 1), d = (s - (float)n) * o with o = (float)O / (float)I from the host;
//              a = dx * dx + dy * dy, b = fmaxf(1.0f - a, 0.0f), wc = fmaxf(b * b, 0.015625f).
//   history    motion is a float2 [IH][IW] plane in OUTPUT pixels, or NULL; the vector m of output pixel (X, Y) is the entry of render pixel
//              (nx, ny) above; q = ((float)X + mx, (float)Y + my).  motion NULL or m exactly (0, 0): Hq and Wq are the previous planes'
//              texels at (X, Y), no arithmetic.  Otherwise, if m is finite and -0.5 <= q_c <= (float)O_c - 0.5f on both axes: Hq is
//              upscale_row / upscale_column (de-ringing included) on the previous H at base (int)floorf(q_c) and fraction
//              q_c - floorf(q_c), indices clamped to the plane; Wq is the previous Wt at clamp((int)floorf(q_c + 0.5f), 0, O_c - 1).  In
//              every other case Wq = 0.  TEMPORAL_RESET makes Wq = 0 everywhere and reads no history.
//   rectify    only with TEMPORAL_RECTIFY and only where history is blended: per channel Hq = fminf(fmaxf(Hq, lo), hi); lo / hi are fminf /
//              fmaxf nested from the left over the 3 x 3 render texels around (nx, ny) in row-major order, indices clamped.
//   blend      wh = fminf(Wq, max_history).  wh > 0: tot = wh + wc, alpha = wc / tot, H' = Hq + alpha * (C - Hq) per channel (all four),
//              Wt' = tot.  Otherwise (reset, no history, NaN): H' = C, Wt' = wc.
//   presented  stage 2 of the spatial upscaler (upscale_sharpen with the buffer's amount) on the plane H', and upscale_rgba8 if asked.
//   sequence   jitter_k = (halton<2>(k + 1) - 0.5f, halton<3>(k + 1) - 0.5f) with the reference's recurrence: f = 1, r = 0; while i > 0:
//              f = f / base, r = r + f * (float)(i % base), i /= base.  (The reference keeps this Halton variant commented out beside
//              its scrambled Sobol sequence; that one needs the reference's direction tables and is not restated here.)
//   motion     of a render pixel: each of the two cameras is a pose in ngp form (rotation R [3][3] row-major and centre c, as nrf_render
//              converts a pose) and cam = (fl_x, fl_y, cx, cy).  For a point x: v = x - c, p_k = (R[0][k] v_0 + R[1][k] v_1) + R[2][k] v_2;
//              p_z not finite or <= 0: invalid; else u = (p_x / p_z) * fl_x + cx, w = (p_y / p_z) * fl_y + cy.  x = o + t * d (the product
//              rounded, then the sum) with t = depth / alpha where alpha >= min_alpha and t is finite and > 0; otherwise the pixel is at
//              infinity: v = d for both cameras.  m = ((u_prev - u_cur) * ox, (w_prev - w_cur) * oy); either projection invalid or the ray
//              not finite: m = (+inf, +inf), which the fetch above reads as no history.  Both projections are through the unjittered
//              cameras.
#pragma once
#include <cstdint>

#include "nrf_upscale_plan.h"

namespace nrf {

constexpr uint32_t TEMPORAL_RESET = 1u, TEMPORAL_RECTIFY = 2u, TEMPORAL_FLAGS = 3u;
constexpr float TEMPORAL_HISTORY_MIN = 1.0f, TEMPORAL_HISTORY_MAX = 256.0f, TEMPORAL_HISTORY_DEFAULT = 64.0f;
constexpr float TEMPORAL_WEIGHT_FLOOR = 0.015625f;

NRF_UPSCALE_HD inline bool temporal_finite(float v) { return v - v == 0.0f; }
NRF_UPSCALE_HD inline bool temporal_jitter_valid(float j) { return j >= -0.5f && j <= 0.5f; }                                  // (NaN: false)
NRF_UPSCALE_HD inline bool temporal_history_valid(float h) { return h >= TEMPORAL_HISTORY_MIN && h <= TEMPORAL_HISTORY_MAX; }  // (NaN: false)

// What a launch needs: the spatial plan, the per-axis ratios o = O / I, the jitter, the history cap and the flags
struct TemporalPlan {
  UpscalePlan U;
  float ox = 0.f, oy = 0.f, jx = 0.f, jy = 0.f, max_history = 0.f;
  uint32_t flags = 0;
};
inline bool temporal_plan(int iw, int ih, int ow, int oh, float amount, float jx, float jy, float max_history, uint32_t flags, TemporalPlan& T) {
  if (!upscale_plan(iw, ih, ow, oh, amount, T.U)) return false;
  if (!temporal_jitter_valid(jx) || !temporal_jitter_valid(jy) || !temporal_history_valid(max_history) || (flags & ~TEMPORAL_FLAGS)) return false;
  T.ox = (float)ow / (float)iw;
  T.oy = (float)oh / (float)ih;
  T.jx = jx, T.jy = jy, T.max_history = max_history, T.flags = flags;
  return true;
}

// One axis of an output pixel: the tap base i, the fraction f, the nearest render texel n and its scaled distance d
NRF_UPSCALE_HD inline void temporal_source(int X, float r, float j, float o, int n_in, int& i, float& f, int& n, float& d) {
  const float centre = (float)X + 0.5f;
  const float scaled = centre * r;
  const float s0 = scaled - 0.5f;
  const float s = s0 - j;
  const float fl = __builtin_floorf(s);
  i = (int)fl;
  f = s - fl;
  const float near = s + 0.5f;
  n = upscale_clamp_index((int)__builtin_floorf(near), n_in);
  const float off = s - (float)n;
  d = off * o;
}
NRF_UPSCALE_HD inline float temporal_sample_weight(float dx, float dy) {
  const float a = dx * dx + dy * dy;
  const float b = __builtin_fmaxf(1.0f - a, 0.0f);
  return __builtin_fmaxf(b * b, TEMPORAL_WEIGHT_FLOOR);
}

// How the history of an output pixel is fetched: HISTORY_NONE (Wq = 0), HISTORY_TEXEL (the texel itself), HISTORY_RESAMPLE (bx, by, fx,
// fy: base and fraction of the reconstruction; wx, wy: the nearest texel of the weight plane)
enum : int { HISTORY_NONE = 0, HISTORY_TEXEL = 1, HISTORY_RESAMPLE = 2 };
struct HistoryFetch {
  int kind = HISTORY_NONE, bx = 0, by = 0, wx = 0, wy = 0;
  float fx = 0.f, fy = 0.f;
};
NRF_UPSCALE_HD inline bool temporal_history_axis(int X, float m, int n_out, int& base, float& frac, int& nearest) {
  const float q = (float)X + m;
  const float top = (float)n_out - 0.5f;
  if (!(q >= -0.5f && q <= top)) return false;
  const float fl = __builtin_floorf(q);
  base = (int)fl;
  frac = q - fl;
  const float near = q + 0.5f;
  nearest = upscale_clamp_index((int)__builtin_floorf(near), n_out);
  return true;
}
NRF_UPSCALE_HD inline HistoryFetch temporal_history_fetch(int X, int Y, bool have_motion, float mx, float my, int ow, int oh, uint32_t flags) {
  HistoryFetch h;
  if (flags & TEMPORAL_RESET) return h;
  if (!have_motion || (mx == 0.0f && my == 0.0f)) {
    h.kind = HISTORY_TEXEL;
    return h;
  }
  if (!temporal_finite(mx) || !temporal_finite(my)) return h;
  if (!temporal_history_axis(X, mx, ow, h.bx, h.fx, h.wx) || !temporal_history_axis(Y, my, oh, h.by, h.fy, h.wy)) return h;
  h.kind = HISTORY_RESAMPLE;
  return h;
}

// lo / hi of the 3 x 3 render texels around (nx, ny), row-major, nested from the left; at(y, x) returns a texel
template <class T>
NRF_UPSCALE_HD inline void temporal_fold_range(const T& p, T& lo, T& hi) {
  lo.x = __builtin_fminf(lo.x, p.x), lo.y = __builtin_fminf(lo.y, p.y), lo.z = __builtin_fminf(lo.z, p.z), lo.w = __builtin_fminf(lo.w, p.w);
  hi.x = __builtin_fmaxf(hi.x, p.x), hi.y = __builtin_fmaxf(hi.y, p.y), hi.z = __builtin_fmaxf(hi.z, p.z), hi.w = __builtin_fmaxf(hi.w, p.w);
}
template <class T>
NRF_UPSCALE_HD inline T temporal_rectify(const T& h, const T& lo, const T& hi) {
  T o;
  o.x = __builtin_fminf(__builtin_fmaxf(h.x, lo.x), hi.x);
  o.y = __builtin_fminf(__builtin_fmaxf(h.y, lo.y), hi.y);
  o.z = __builtin_fminf(__builtin_fmaxf(h.z, lo.z), hi.z);
  o.w = __builtin_fminf(__builtin_fmaxf(h.w, lo.w), hi.w);
  return o;
}

// The blend.  Returns true where history is used: then hq has to be valid (and rectified if asked)
NRF_UPSCALE_HD inline float temporal_history_weight(float wq, float max_history) { return __builtin_fminf(wq, max_history); }
NRF_UPSCALE_HD inline float temporal_blend1(float hq, float c, float alpha) {
  const float diff = c - hq;
  const float step = alpha * diff;
  return hq + step;
}
template <class T>
NRF_UPSCALE_HD inline T temporal_blend(const T& hq, const T& c, float wh, float wc, float& w_out) {
  const float tot = wh + wc;
  const float alpha = wc / tot;
  T o;
  o.x = temporal_blend1(hq.x, c.x, alpha);
  o.y = temporal_blend1(hq.y, c.y, alpha);
  o.z = temporal_blend1(hq.z, c.z, alpha);
  o.w = temporal_blend1(hq.w, c.w, alpha);
  w_out = tot;
  return o;
}

// The jitter sequence
template <uint32_t BASE>
inline float temporal_halton(uint64_t i) {
  float f = 1.0f, r = 0.0f;
  while (i > 0) {
    f = f / (float)BASE;
    const float term = f * (float)(uint32_t)(i % BASE);
    r = r + term;
    i /= BASE;
  }
  return r;
}
inline void temporal_jitter(uint32_t index, float (&j)[2]) {
  j[0] = temporal_halton<2>((uint64_t)index + 1) - 0.5f;
  j[1] = temporal_halton<3>((uint64_t)index + 1) - 0.5f;
}

// ---- the motion vectors of a static scene
struct MotionCamera {
  float R[9] = {}, c[3] = {}, cam[4] = {};  // rotation [3][3] row-major and centre in ngp form; fl_x, fl_y, cx, cy
};
struct MotionPlan {
  int iw = 0, ih = 0;
  float ox = 0.f, oy = 0.f, min_alpha = 0.f;
  MotionCamera cur, prev;
};
NRF_UPSCALE_HD inline bool motion_alpha_valid(float a) { return a > 0.0f && a <= 1.0f; }  // (NaN: false)
inline bool motion_plan(int iw, int ih, int ow, int oh, float min_alpha, MotionPlan& M) {
  if (!upscale_axis_valid(iw, ow) || !upscale_axis_valid(ih, oh) || !motion_alpha_valid(min_alpha)) return false;
  M.iw = iw, M.ih = ih;
  M.ox = (float)ow / (float)iw;
  M.oy = (float)oh / (float)ih;
  M.min_alpha = min_alpha;
  return true;
}
// a camera from a pose [4][4] row-major (its first 12 values are read), the scene scale and cam: the conversion nrf_render makes
inline void motion_camera(const float pose[16], float scale, const float cam[4], MotionCamera& K) {
  const int rows[3] = {1, 2, 0};
  for (int r = 0; r < 3; ++r) {
    const float* src = pose + 4 * rows[r];
    K.R[3 * r + 0] = src[0];
    K.R[3 * r + 1] = -src[1];
    K.R[3 * r + 2] = -src[2];
    K.c[r] = src[3] * scale + 0.0f;
  }
  for (int k = 0; k < 4; ++k) K.cam[k] = cam[k];
}
// v (a point minus the centre, or a direction) through one camera: false where the projection is invalid
NRF_UPSCALE_HD inline bool motion_project(const MotionCamera& K, const float (&v)[3], float& u, float& w) {
  float p[3];
  for (int k = 0; k < 3; ++k) p[k] = (K.R[0 + k] * v[0] + K.R[3 + k] * v[1]) + K.R[6 + k] * v[2];
  if (!temporal_finite(p[2]) || !(p[2] > 0.0f)) return false;
  u = (p[0] / p[2]) * K.cam[0] + K.cam[2];
  w = (p[1] / p[2]) * K.cam[1] + K.cam[3];
  return true;
}
NRF_UPSCALE_HD inline void motion_vector(const MotionPlan& M, const float (&o)[3], const float (&d)[3], float alpha, float depth, float& mx, float& my) {
  mx = my = __builtin_inff();
  for (int k = 0; k < 3; ++k)
    if (!temporal_finite(o[k]) || !temporal_finite(d[k])) return;
  float vc[3], vp[3];
  bool at_infinity = true;
  if (alpha >= M.min_alpha) {
    const float t = depth / alpha;
    if (temporal_finite(t) && t > 0.0f) {
      at_infinity = false;
      for (int k = 0; k < 3; ++k) {
        const float along = t * d[k];
        const float x = o[k] + along;
        vc[k] = x - M.cur.c[k];
        vp[k] = x - M.prev.c[k];
      }
    }
  }
  if (at_infinity)
    for (int k = 0; k < 3; ++k) vc[k] = vp[k] = d[k];
  float uc, wc, up, wp;
  if (!motion_project(M.cur, vc, uc, wc) || !motion_project(M.prev, vp, up, wp)) return;
  mx = (up - uc) * M.ox;
  my = (wp - wc) * M.oy;
}

// ---- the launches (nrf_kernels_temporal.hip): a HIP error code.  src float4 [ih][iw]; motion float2 [ih][iw] or NULL; hist_prev / w_prev
// float4 / float [oh][ow] (not read under TEMPORAL_RESET); hist_next / w_next the same, written; dst float4 [oh][ow]; rgba8 uint32
// [oh][ow] or NULL
int launch_temporal(const TemporalPlan& T, const void* src, const void* motion, const void* hist_prev, const void* w_prev, void* hist_next,
                    void* w_next, void* dst, void* rgba8, void* stream);
// rays_o / rays_d float [n][3], rgba float4 [n], depth_t float [n], out float2 [n], n = ih * iw
int launch_motion(const MotionPlan& M, const void* rays_o, const void* rays_d, const void* rgba, const void* depth_t, void* out, void* stream);

}  // namespace nrf
