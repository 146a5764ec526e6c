// nrf_upscale_plan.h -- the definition of the render buffer's spatial upscaler (nrf_rb_upscale) without a device: where an output pixel
// lies in the source plane, the Catmull-Rom weights, the reconstruction with its de-ringing clamp, the clamped unsharp mask and the packed
// 8-bit pixel.  upscale_kernel (nrf_kernels_upscale.hip) and host/upscale_plan_check.cpp compile this text and nothing else does, so the
// kernel's definition and the tests' replay (tests/upscale_replay.py) are one.  Every fp32 operation is ONE rounding with no contraction
// (the library is built with -ffp-contract=off -fno-fast-math, and a host build of this header has to be: host/Makefile, upscale_asan),
// every integer operation is exact, and there is no transcendental function.  No HIP types: a texel is any type with float members
// x, y, z, w (float4 on the device).
//
// The source plane P is [IH][IW] texels, the target plane [OH][OW], IW <= OW <= 8 IW, IH <= OH <= 8 IH, OW, OH <= 16384.
//   geometry   per axis: r = (float)I / (float)O, once on the host.  Output index X: s = ((float)X + 0.5f) * r - 0.5f (the sum, then the
//              product, then the difference, each rounded), i = (int)floorf(s), f = s - (float)i (exact, 0 <= f < 1).  The taps are
//              i - 1, i, i + 1, i + 2, each clamped to [0, I - 1] as integers.
//   weights    of t = f: w0 = t (-0.5 + t (1 - 0.5 t)), w1 = 1 + (t t)(-2.5 + 1.5 t), w2 = t (0.5 + t (2 - 1.5 t)),
//              w3 = (t t)(-0.5 + 0.5 t), every operation as parenthesised in upscale_weights.
//   stage 1    per channel, all four: for each tap row j, h_j = ((wx0 p0 + wx1 p1) + wx2 p2) + wx3 p3; v = ((wy0 h_0 + wy1 h_1) + wy2 h_2)
//              + wy3 h_3; lo / hi = fminf / fmaxf over the four inner texels (columns i, i + 1 and rows i, i + 1, clamped), taken as
//              f(f(p11, p12), f(p21, p22)); U = fminf(fmaxf(v, lo), hi).
//   stage 2    on the plane U, channels r, g, b (alpha is U's): n, s, w, e = the four neighbours of c = U[Y][X] with indices clamped to
//              the plane; blur = ((n + s) + (w + e)) * 0.25f, d = c - blur, x = c + amount * d,
//              out = fminf(fmaxf(x, min(c, n, s, w, e)), max(c, n, s, w, e)) with the minima and maxima nested from the left.
//   packed     r | g << 8 | b << 16 | a << 24 of out with the library's 8-bit rule ((unsigned char)(255.0 * x), saturating, NaN -> 0).
// (fminf / fmaxf return the other operand for a NaN; which of +0 and -0 they return for that pair is the one thing left open.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NRF_UPSCALE_HD __host__ __device__
#else
#define NRF_UPSCALE_HD
#endif

namespace nrf {

constexpr int UPSCALE_RATIO_MAX = 8, UPSCALE_OUT_MAX = 16384;
constexpr float UPSCALE_AMOUNT_MAX = 2.0f;

// one axis of an output resolution against the render resolution: in <= out <= 8 in, out <= 16384
NRF_UPSCALE_HD inline bool upscale_axis_valid(int in, int out) {
  return in > 0 && out >= in && out <= UPSCALE_OUT_MAX && (int64_t)out <= (int64_t)UPSCALE_RATIO_MAX * in;
}
NRF_UPSCALE_HD inline bool upscale_amount_valid(float amount) { return amount >= 0.0f && amount <= UPSCALE_AMOUNT_MAX; }  // (NaN: false)

// What a launch needs: the two resolutions, the per-axis ratios r = I / O and the sharpening amount
struct UpscalePlan {
  int iw = 0, ih = 0, ow = 0, oh = 0;
  float rx = 0.f, ry = 0.f, amount = 0.f;
};
inline bool upscale_plan(int iw, int ih, int ow, int oh, float amount, UpscalePlan& P) {
  if (!upscale_axis_valid(iw, ow) || !upscale_axis_valid(ih, oh) || !upscale_amount_valid(amount)) return false;
  P.iw = iw, P.ih = ih, P.ow = ow, P.oh = oh;
  P.rx = (float)iw / (float)ow;
  P.ry = (float)ih / (float)oh;
  P.amount = amount;
  return true;
}

// Geometry of one axis: output index X -> the tap base i (the taps are i - 1 .. i + 2) and the fraction f
NRF_UPSCALE_HD inline void upscale_source(int X, float r, int& i, float& f) {
  const float centre = (float)X + 0.5f;
  const float scaled = centre * r;
  const float s = scaled - 0.5f;
  const float fl = __builtin_floorf(s);
  i = (int)fl;
  f = s - fl;
}
NRF_UPSCALE_HD inline int upscale_clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// the four clamped tap indices of base i on an axis of n texels
NRF_UPSCALE_HD inline void upscale_taps(int i, int n, int (&tap)[4]) {
  for (int a = 0; a < 4; ++a) tap[a] = upscale_clamp_index(i - 1 + a, n);
}

// The Catmull-Rom weights of t
NRF_UPSCALE_HD inline void upscale_weights(float t, float (&w)[4]) {
  w[0] = t * (-0.5f + t * (1.0f - 0.5f * t));
  w[1] = 1.0f + (t * t) * (-2.5f + 1.5f * t);
  w[2] = t * (0.5f + t * (2.0f - 1.5f * t));
  w[3] = (t * t) * (-0.5f + 0.5f * t);
}

// ((w0 p0 + w1 p1) + w2 p2) + w3 p3: a tap row across, and the four rows down
NRF_UPSCALE_HD inline float upscale_dot4(const float (&w)[4], float p0, float p1, float p2, float p3) {
  return ((w[0] * p0 + w[1] * p1) + w[2] * p2) + w[3] * p3;
}
NRF_UPSCALE_HD inline float upscale_deringed(float v, float p11, float p12, float p21, float p22) {
  const float lo = __builtin_fminf(__builtin_fminf(p11, p12), __builtin_fminf(p21, p22));
  const float hi = __builtin_fmaxf(__builtin_fmaxf(p11, p12), __builtin_fmaxf(p21, p22));
  return __builtin_fminf(__builtin_fmaxf(v, lo), hi);
}

// Stage 1 in its two halves.  upscale_row: one tap row across, h = ((wx0 p0 + wx1 p1) + wx2 p2) + wx3 p3 per channel -- it depends on the
// source row and the output column only, so whoever evaluates many output rows may keep it.  upscale_column: the four rows down, and the
// de-ringing clamp among the four inner texels (p11, p12 of tap row 1, p21, p22 of tap row 2)
template <class T>
NRF_UPSCALE_HD inline T upscale_row(const float (&wx)[4], const T& p0, const T& p1, const T& p2, const T& p3) {
  T h;
  h.x = upscale_dot4(wx, p0.x, p1.x, p2.x, p3.x);
  h.y = upscale_dot4(wx, p0.y, p1.y, p2.y, p3.y);
  h.z = upscale_dot4(wx, p0.z, p1.z, p2.z, p3.z);
  h.w = upscale_dot4(wx, p0.w, p1.w, p2.w, p3.w);
  return h;
}
template <class T>
NRF_UPSCALE_HD inline T upscale_column(const float (&wy)[4], const T& h0, const T& h1, const T& h2, const T& h3, const T& p11, const T& p12,
                                       const T& p21, const T& p22) {
  T u;
  u.x = upscale_deringed(upscale_dot4(wy, h0.x, h1.x, h2.x, h3.x), p11.x, p12.x, p21.x, p22.x);
  u.y = upscale_deringed(upscale_dot4(wy, h0.y, h1.y, h2.y, h3.y), p11.y, p12.y, p21.y, p22.y);
  u.z = upscale_deringed(upscale_dot4(wy, h0.z, h1.z, h2.z, h3.z), p11.z, p12.z, p21.z, p22.z);
  u.w = upscale_deringed(upscale_dot4(wy, h0.w, h1.w, h2.w, h3.w), p11.w, p12.w, p21.w, p22.w);
  return u;
}

// Stage 2 of one channel: the clamped unsharp mask of c among its four neighbours on U
NRF_UPSCALE_HD inline float upscale_sharpen1(float c, float n, float s, float w, float e, float amount) {
  const float blur = ((n + s) + (w + e)) * 0.25f;
  const float d = c - blur;
  const float x = c + amount * d;
  const float lo = __builtin_fminf(__builtin_fminf(__builtin_fminf(__builtin_fminf(c, n), s), w), e);
  const float hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(c, n), s), w), e);
  return __builtin_fminf(__builtin_fmaxf(x, lo), hi);
}
template <class T>
NRF_UPSCALE_HD inline T upscale_sharpen(const T& c, const T& n, const T& s, const T& w, const T& e, float amount) {
  T o;
  o.x = upscale_sharpen1(c.x, n.x, s.x, w.x, e.x, amount);
  o.y = upscale_sharpen1(c.y, n.y, s.y, w.y, e.y, amount);
  o.z = upscale_sharpen1(c.z, n.z, s.z, w.z, e.z, amount);
  o.w = c.w;
  return o;
}

// The library's 8-bit rule (to_u8 of nrf_renderbuffer.hip): (unsigned char)(255.0 * x) with the product in double, saturating, NaN -> 0
NRF_UPSCALE_HD inline uint32_t upscale_u8(float v) {
  const double s = 255.0 * (double)v;
  if (!(s > 0.0)) return 0u;
  if (s >= 255.0) return 255u;
  return (uint32_t)s;
}
template <class T>
NRF_UPSCALE_HD inline uint32_t upscale_rgba8(const T& o) {
  return upscale_u8(o.x) | upscale_u8(o.y) << 8 | upscale_u8(o.z) << 16 | upscale_u8(o.w) << 24;
}

// ---- the launch (nrf_kernels_upscale.hip): a HIP error code; src float4 [ih][iw], dst float4 [oh][ow], rgba8 uint32 [oh][ow] or NULL
int launch_upscale(const UpscalePlan& P, const void* src, void* dst, void* rgba8, void* stream);

}  // namespace nrf
