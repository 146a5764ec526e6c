// nrf_overlay_plan.h -- the definition of the render buffer's colour functions, its image and false-colour overlays and its error map
// without a device.  nrf_renderbuffer.hip (present_kernel, overlay_depth_kernel), nrf_kernels_overlay.hip and host/overlay_plan_check.cpp
// compile this text, so the kernels' definition and the tests' replay (tests/overlay_replay.py) are one.  Every fp32 operation is ONE
// rounding with no contraction (the library is built with -ffp-contract=off -fno-fast-math, and a host build of this header has to be:
// host/Makefile, overlay_asan), every integer operation is exact.  The one transcendental function is the power inside the sRGB pair
// (pow_positive: two instructions on the device, libm's powf on the host).  Operation order is the reference's source text
// (R/src/render_buffer.cu:261-527, R/include/nerf-cuda/common_device.cuh:38-102), read as overlay_depth_kernel and develop() read it:
// an Eigen dot of four terms is (p0 + p1) + (p2 + p3), one of three p0 + (p1 + p2); max(x, 0) inside the curves is the device's fmaxf
// (deviation D-11, overlay_max0).  No HIP types: a texel is any type with float members x, y, z, w (float4 on the device).
//
//   pixel mapping   surface pixel (x, y) of a W x H surface -> (srcx, srcy) of an iw x ih image (overlay_source):
//                   scale = (float)(axis == 0 ? iw : ih) / (float)(axis == 0 ? W : H);
//                   fx = (float)x + 0.5f; fx -= (float)W * 0.5f; fx /= zoom; fx += center_x * (float)W;   fy likewise with H, center_y;
//                   u = (fx - (float)W * 0.5f) * scale + (float)iw * 0.5f;   v likewise;   srcx = to_index(floorf(u)), srcy likewise.
//                   to_index (overlay_index) saturates: a value below -2^31 or a NaN gives INT_MIN, one of 2^31 or more INT_MAX --
//                   both outside every image.  (The device's conversion saturates but turns a NaN into 0; the reference's bare cast
//                   is undefined for both.)
//   read_rgba       NRF_IMG_BYTE = 1: uint32 texels b0 | b1 << 8 | b2 << 16 | b3 << 24.  The texel 0x00FF00FF gives (-1, -1, -1, -1);
//                   otherwise a = (float)b3 * (1.0f / 255.0f) and channel k = T[b_k] * a, where T[b] = decode_srgb((float)b * (1.0f / 255.0f))
//                   is made ONCE on the host with libm (overlay_srgb8_table, nrf_rb_srgb8_table): the one deliberate difference from
//                   running the power per pixel on the device -- a Byte image is bit-exact against a CPU compile of the reference.
//                   NRF_IMG_HALF = 2: four fp16 values, widened exactly (overlay_half).  NRF_IMG_FLOAT = 3: a float4.
//   overlay image   per surface pixel (overlay_image_pixel): val = the texel at (srcx, srcy), zero when that lies outside the image.
//                   Render space sRGB: rgb = encode_srgb(rgb / w) * w for w > 0, else 0.  (Render space not sRGB: the background was
//                   decoded on the host, once per call.)  weight = (1 - w) * bg.w; rgb += bg.rgb * weight; w += weight.  Then the
//                   five-argument tonemap (develop_color): decode if the render space is sRGB, times gain[k] = powf(2, exposure[k])
//                   from the host, the film curve, encode if the display space is sRGB.  out = color * alpha + prev * (1.f - alpha)
//                   on all four channels.
//   false colour    per surface pixel (overlay_false_color_source, overlay_false_color_pixel): error_map_scale = brightness /
//                   (0.0000001f + average[0]); scale = (float)(axis == 0 ? tw : th) / (float)(axis == 0 ? W : H);
//                   u = ((float)x + 0.5f - (float)W * 0.5f) * scale + (float)tw * 0.5f;  v likewise;
//                   srcx = to_index(floorf(u * (float)mw / fmaxf(1.f, (float)tw))), srcy likewise; a pixel outside the mw x mh map is
//                   left untouched.  err = map[src] * error_map_scale; with viridis err *= 1.f / (1.f + err).  c = colormap_viridis
//                   (a Horner chain per channel, as written) or colormap_turbo; sat(c) clamps to [0, 1] with NaN -> 0;
//                   grey = r * 0.2126f + g * 0.7152f + b * 0.0722f summed left to right (this is NOT an Eigen dot);
//                   rgb = grey * sat(c), alpha untouched.
//   error map       (this project's own definition: the reference fills its map during training, which neither project has.)  Surface S
//                   and truth G are float4 [H][W]; the map is float [mh][mw], 1 <= mw <= min(W, 512), 1 <= mh <= min(H, 512).  Cell cx
//                   covers columns x0(cx) .. x0(cx + 1) - 1 with x0(c) = (c * W + mw - 1) / mw in integers (error_cell_begin), rows
//                   likewise: every cell holds at least one pixel.  Per pixel e = (((dr * dr) + (dg * dg)) + (db * db)) / 3.0f with
//                   d = S - G, alpha ignored (error_pixel).  One wave of 64 lanes reduces one cell: with the cell's pixels row-major
//                   as k = 0, 1, ..., lane l adds e_k for k = l (mod 64) in ascending k onto 0.0f; then for s = 32, 16, ..., 1 and
//                   lanes l < s, v[l] = v[l] + v[l + s]; the cell's value is v[0] / (float)count.  The average is the same scheme,
//                   one wave over the cells in row-major order: average[0] = v[0] / (float)(mw * mh).  NaNs propagate.  So the average
//                   is the MEAN OF THE CELL MEANS: it equals the image's mean squared error only when mw divides W and mh divides H
//                   (all cells the same size).  error_reduce is this order on a host, element by element.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NRF_OVERLAY_HD __host__ __device__
#define NRF_OVERLAY_UNROLL _Pragma("unroll")
#else
#define NRF_OVERLAY_HD
#define NRF_OVERLAY_UNROLL
#endif

namespace nrf {

// include/nerfhip.h's numbers (nrf_renderbuffer.hip asserts that they are)
constexpr int CS_LINEAR = 0, CS_SRGB = 1, CS_VISPOSNEG = 2;
constexpr int TM_IDENTITY = 0, TM_ACES = 1, TM_HABLE = 2, TM_REINHARD = 3;
constexpr int IMG_BYTE = 1, IMG_HALF = 2, IMG_FLOAT = 3;
constexpr int OVERLAY_SIZE_MAX = 16384, ERROR_MAP_MAX = 512;

// ---- colour ----
// the sRGB transfer pair as the reference states it (R/include/nerf-cuda/common_device.cuh:38-60: note the 0.41666 exponent).
// On the device the power is 2^(e log2 x) on the two transcendental instructions (v_log_f32, v_exp_f32; the argument is
// positive on this branch): within 2e-6 of libm's powf over the range a colour takes -- the general powf made the chain
// ALU-bound (32-52 us per 1080p plane against 20 us for the same stream without it, profiles/r05/rb_bench.txt).  The host
// forms (the background colour, once per call; the Byte table) stay libm's, which is the oracle's.
NRF_OVERLAY_HD inline float pow_positive(float x, float e) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x));
#else
  return powf(x, e);
#endif
}
NRF_OVERLAY_HD inline float decode_srgb(float v) { return v <= 0.04045f ? v / 12.92f : pow_positive((v + 0.055f) / 1.055f, 2.4f); }
NRF_OVERLAY_HD inline float encode_srgb(float v) { return v < 0.0031308f ? 12.92f * v : 1.055f * pow_positive(v, 0.41666f) - 0.055f; }

// A film curve, reduced on the host to what the pixel loop needs.  RATIONAL: y = (x^2 n2 + n1 x + n0) / (d2 x^2 + d1 x + d0)
// on max(x, 0) per channel (operation order as written: it is part of the contract with the oracle); LUMA: Reinhard's
// x / (1 + Y) on max(x, 0) with Y the Rec. 709 luminance.
enum : int { CURVE_NONE = 0, CURVE_RATIONAL = 1, CURVE_LUMA = 2 };
struct FilmCurve {
  int kind;
  float n2, n1, n0, d2, d1, d0;
};
inline FilmCurve film_curve(int tonemap) {  // render_buffer.cu:261-318, the constants of its two rational curves
  FilmCurve f{CURVE_NONE, 0, 0, 0, 0, 0, 0};
  if (tonemap == TM_ACES) {  // Narkowicz's fit, pre-scaled by 0.6
    f = {CURVE_RATIONAL, 0.6f * 0.6f * 2.51f, 0.6f * 0.03f, 0.0f, 0.6f * 0.6f * 2.43f, 0.6f * 0.59f, 0.14f};
  } else if (tonemap == TM_HABLE) {  // Hable's filmic operator, normalised so that the white point 11.2 maps to 1
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f, white = 11.2f;
    float n2 = A * F - A * E, n1 = C * B * F - B * E, n0 = 0.0f;
    float d2 = A * F, d1 = B * F;
    const float d0 = D * F * F;
    const float at_white_n = n2 * (white * white) + n1 * white + n0;
    const float at_white_d = d2 * (white * white) + d1 * white + d0;
    const float norm = at_white_d / at_white_n;
    f = {CURVE_RATIONAL, 4.0f * n2 * norm, 2.0f * n1 * norm, n0 * norm, 4.0f * d2, 2.0f * d1, d0};
  } else if (tonemap == TM_REINHARD) {
    f.kind = CURVE_LUMA;
  }
  return f;
}

// the curves' max(x, 0) as the device evaluates it (deviation D-11): a NaN and a -0 give +0.  On the device that is fmaxf; a host's
// fmaxf may keep the -0, so the host form spells the rule out
NRF_OVERLAY_HD inline float overlay_max0(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaxf(x, 0.f);
#else
  return x > 0.0f ? x : 0.0f;
#endif
}

// the reference's five-argument tonemap (render_buffer.cu:320-339) on one colour: into linear values if the render space is sRGB,
// times the per-channel gain 2^exposure, through the film curve, into the display's transfer function
NRF_OVERLAY_HD inline void develop_color(float (&c)[3], int render_space, const float (&gain)[3], const FilmCurve& f, int display_space) {
  NRF_OVERLAY_UNROLL
  for (int k = 0; k < 3; ++k) {
    if (render_space == CS_SRGB) c[k] = decode_srgb(c[k]);
    c[k] *= gain[k];
  }
  if (f.kind != CURVE_NONE) {
    NRF_OVERLAY_UNROLL
    for (int k = 0; k < 3; ++k) c[k] = overlay_max0(c[k]);
    if (f.kind == CURVE_LUMA) {
      const float scale = 1.f / ((0.2126f * c[0] + (0.7152f * c[1] + 0.0722f * c[2])) + 1.0f);  // a 3-term Eigen dot: p0 + (p1 + p2)
      NRF_OVERLAY_UNROLL
      for (int k = 0; k < 3; ++k) c[k] = c[k] * scale;
    } else {
      NRF_OVERLAY_UNROLL
      for (int k = 0; k < 3; ++k) {
        const float sq = c[k] * c[k];
        c[k] = (sq * f.n2 + f.n1 * c[k] + f.n0) / (f.d2 * sq + f.d1 * c[k] + f.d0);
      }
    }
  }
  if (display_space == CS_SRGB) {
    NRF_OVERLAY_UNROLL
    for (int k = 0; k < 3; ++k) c[k] = encode_srgb(c[k]);
  }
}

// __saturatef: into [0, 1], NaN -> 0
NRF_OVERLAY_HD inline float overlay_saturate(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }

// colormap_turbo, R/src/render_buffer.cu:413-429: the polynomial is evaluated as the fixed-size Eigen dot products do.  Eigen's
// unrolled scalar reduction splits a sum in halves, so a 4-term dot is (a0*b0 + a1*b1) + (a2*b2 + a3*b3), every operation rounded on
// its own (tests/test_reference_render_buffer_cpu.py holds the oracle's copy to the reference's own Eigen).
NRF_OVERLAY_HD inline float overlay_dot4(const float (&a)[4], float b0, float b1, float b2, float b3) {
  return (a[0] * b0 + a[1] * b1) + (a[2] * b2 + a[3] * b3);
}
NRF_OVERLAY_HD inline void colormap_turbo(float x, float (&c)[3]) {
  const float kR4[4] = {0.13572138f, 4.61539260f, -42.66032258f, 132.13108234f};
  const float kG4[4] = {0.09140261f, 2.19418839f, 4.84296658f, -14.18503333f};
  const float kB4[4] = {0.10667330f, 12.64194608f, -60.58204836f, 110.36276771f};
  const float kR2[2] = {-152.94239396f, 59.28637943f};
  const float kG2[2] = {4.27729857f, 2.82956604f};
  const float kB2[2] = {-89.90310912f, 27.34824973f};
  x = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);  // __saturatef (NaN -> 0)
  if (!(x == x)) x = 0.0f;
  const float x2 = x * x, x3 = x2 * x;
  const float v20 = x3 * x, v21 = x3 * x2;
  c[0] = overlay_dot4(kR4, 1.0f, x, x2, x3) + (v20 * kR2[0] + v21 * kR2[1]);
  c[1] = overlay_dot4(kG4, 1.0f, x, x2, x3) + (v20 * kG2[0] + v21 * kG2[1]);
  c[2] = overlay_dot4(kB4, 1.0f, x, x2, x3) + (v20 * kB2[0] + v21 * kB2[1]);
}
// colormap_viridis, :479-489: c0 + x (c1 + x (c2 + x (c3 + x (c4 + x (c5 + x c6))))) per channel, the Horner chain as written
NRF_OVERLAY_HD inline void colormap_viridis(float x, float (&c)[3]) {
  const float k[7][3] = {{0.2777273272234177f, 0.005407344544966578f, 0.3340998053353061f},
                         {0.1050930431085774f, 1.404613529898575f, 1.384590162594685f},
                         {-0.3308618287255563f, 0.214847559468213f, 0.09509516302823659f},
                         {-4.634230498983486f, -5.799100973351585f, -19.33244095627987f},
                         {6.228269936347081f, 14.17993336680509f, 56.69055260068105f},
                         {4.776384997670288f, -13.74514537774601f, -65.35303263337234f},
                         {-5.435455855934631f, 4.645852612178535f, 26.3124352495832f}};
  x = overlay_saturate(x);
  NRF_OVERLAY_UNROLL
  for (int j = 0; j < 3; ++j) {
    float h = k[6][j];
    NRF_OVERLAY_UNROLL
    for (int i = 5; i >= 0; --i) h = k[i][j] + x * h;
    c[j] = h;
  }
}

// ---- the pixel mapping ----
// a floored coordinate as an index: saturating, and a NaN lies outside every image
NRF_OVERLAY_HD inline int overlay_index(float floored) {
  if (!(floored >= -2147483648.0f)) return INT_MIN;  // (a NaN too)
  if (floored >= 2147483648.0f) return INT_MAX;
  return (int)floored;
}
// What overlay_depth, overlay_image and (without zoom and centre) overlay_false_color know of a call
struct OverlayMap {
  int W, H;          // the surface
  int iw, ih;        // the image (the training resolution for the false colours)
  int fov_axis;      // 0 or 1
  float zoom, center_x, center_y;
};
NRF_OVERLAY_HD inline void overlay_source(const OverlayMap& M, int x, int y, int& srcx, int& srcy) {
  const float scale = (float)(M.fov_axis == 0 ? M.iw : M.ih) / (float)(M.fov_axis == 0 ? M.W : M.H);
  float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
  fx -= (float)M.W * 0.5f; fx /= M.zoom; fx += M.center_x * (float)M.W;
  fy -= (float)M.H * 0.5f; fy /= M.zoom; fy += M.center_y * (float)M.H;
  const float u = (fx - (float)M.W * 0.5f) * scale + (float)M.iw * 0.5f;
  const float v = (fy - (float)M.H * 0.5f) * scale + (float)M.ih * 0.5f;
  srcx = overlay_index(__builtin_floorf(u));
  srcy = overlay_index(__builtin_floorf(v));
}
NRF_OVERLAY_HD inline bool overlay_inside(int srcx, int srcy, int w, int h) { return !(srcx >= w || srcy >= h || srcx < 0 || srcy < 0); }

// ---- read_rgba ----
// T[b] = srgb_to_linear((float)b * (1.0f / 255.0f)), b = 0 .. 255: host only, libm's power
inline void overlay_srgb8_table(float (&table)[256]) {
  for (int b = 0; b < 256; ++b) table[b] = decode_srgb((float)b * (1.0f / 255.0f));
}
template <class T>
NRF_OVERLAY_HD inline T overlay_texel(float x, float y, float z, float w) {
  T t;
  t.x = x, t.y = y, t.z = z, t.w = w;
  return t;
}
template <class T>
NRF_OVERLAY_HD inline T overlay_read_byte(uint32_t texel, const float* table) {
  if (texel == 0x00FF00FFu) return overlay_texel<T>(-1.0f, -1.0f, -1.0f, -1.0f);
  const float a = (float)(texel >> 24) * (1.0f / 255.0f);
  return overlay_texel<T>(table[texel & 255u] * a, table[(texel >> 8) & 255u] * a, table[(texel >> 16) & 255u] * a, a);
}
// an fp16 bit pattern as the fp32 of the same value (exact; a NaN keeps its payload)
NRF_OVERLAY_HD inline float overlay_half(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exponent = (h >> 10) & 31u;
  uint32_t mantissa = h & 0x3FFu, bits;
  if (exponent == 31u) {
    bits = sign | 0x7F800000u | (mantissa << 13);
  } else if (exponent != 0u) {
    bits = sign | ((exponent + 112u) << 23) | (mantissa << 13);
  } else if (mantissa == 0u) {
    bits = sign;
  } else {  // a denormal: mantissa * 2^-24, normalised
    uint32_t e = 113u;
    while (!(mantissa & 0x400u)) mantissa <<= 1, --e;
    bits = sign | (e << 23) | ((mantissa & 0x3FFu) << 13);
  }
  float f;
  __builtin_memcpy(&f, &bits, sizeof f);
  return f;
}
template <class T>
NRF_OVERLAY_HD inline T overlay_read_half(uint64_t texel) {
  return overlay_texel<T>(overlay_half((uint16_t)texel), overlay_half((uint16_t)(texel >> 16)), overlay_half((uint16_t)(texel >> 32)),
                          overlay_half((uint16_t)(texel >> 48)));
}

// ---- the image overlay ----
struct OverlayImage {
  OverlayMap map;
  float alpha;
  float gain[3];        // 2^exposure per channel, from the host
  float bg[4];          // the background colour in the RENDER colour space (decoded on the host unless that is sRGB)
  int render_space, display_space;  // CS_*
  FilmCurve film;
};
// the background in the render colour space: given display-referred, decoded once on the host unless the render space is sRGB
inline void overlay_background(const float (&given)[4], int render_space, float (&bg)[4]) {
  for (int k = 0; k < 3; ++k) bg[k] = render_space != CS_SRGB ? decode_srgb(given[k]) : given[k];
  bg[3] = given[3];
}
// val: the texel read (zeros outside the image); prev: the surface's pixel
template <class T>
NRF_OVERLAY_HD inline T overlay_image_pixel(const OverlayImage& A, const T& val, const T& prev) {
  float c[3] = {val.x, val.y, val.z};
  float w = val.w;
  if (A.render_space == CS_SRGB) {
    if (w > 0.0f) {
      NRF_OVERLAY_UNROLL
      for (int k = 0; k < 3; ++k) c[k] = encode_srgb(c[k] / w) * w;
    } else {
      c[0] = c[1] = c[2] = 0.0f;
    }
  }
  const float weight = (1 - w) * A.bg[3];
  NRF_OVERLAY_UNROLL
  for (int k = 0; k < 3; ++k) c[k] += A.bg[k] * weight;
  w += weight;
  develop_color(c, A.render_space, A.gain, A.film, A.display_space);
  const float ia = 1.f - A.alpha;
  return overlay_texel<T>(c[0] * A.alpha + prev.x * ia, c[1] * A.alpha + prev.y * ia, c[2] * A.alpha + prev.z * ia, w * A.alpha + prev.w * ia);
}

// ---- the false-colour overlay ----
struct OverlayFalseColor {
  int W, H;        // the surface
  int tw, th;      // the training resolution
  int mw, mh;      // the error map
  int fov_axis;
  float brightness;
  int viridis;
};
NRF_OVERLAY_HD inline void overlay_false_color_source(const OverlayFalseColor& A, int x, int y, int& srcx, int& srcy) {
  const float scale = (float)(A.fov_axis == 0 ? A.tw : A.th) / (float)(A.fov_axis == 0 ? A.W : A.H);
  const float u = ((float)x + 0.5f - (float)A.W * 0.5f) * scale + (float)A.tw * 0.5f;
  const float v = ((float)y + 0.5f - (float)A.H * 0.5f) * scale + (float)A.th * 0.5f;
  srcx = overlay_index(__builtin_floorf(u * (float)A.mw / __builtin_fmaxf(1.f, (float)A.tw)));
  srcy = overlay_index(__builtin_floorf(v * (float)A.mh / __builtin_fmaxf(1.f, (float)A.th)));
}
NRF_OVERLAY_HD inline float overlay_error_scale(float brightness, float average) { return brightness / (0.0000001f + average); }
// error: the map's value at the pixel's cell; color: the surface's pixel
template <class T>
NRF_OVERLAY_HD inline T overlay_false_color_pixel(const OverlayFalseColor& A, float error, float error_map_scale, const T& color) {
  float err = error * error_map_scale;
  if (A.viridis) err *= 1.f / (1.f + err);
  float c[3];
  if (A.viridis) colormap_viridis(err, c);
  else colormap_turbo(err, c);
  const float grey = color.x * 0.2126f + color.y * 0.7152f + color.z * 0.0722f;
  return overlay_texel<T>(grey * overlay_saturate(c[0]), grey * overlay_saturate(c[1]), grey * overlay_saturate(c[2]), color.w);
}

// ---- the error map ----
NRF_OVERLAY_HD inline bool error_map_axis_valid(int pixels, int cells) { return cells >= 1 && cells <= ERROR_MAP_MAX && cells <= pixels; }
// the first pixel of cell c on an axis of n pixels and m cells, 0 <= c <= m (c * n < 2^23)
NRF_OVERLAY_HD inline int error_cell_begin(int c, int n, int m) { return (c * n + m - 1) / m; }
template <class T>
NRF_OVERLAY_HD inline float error_pixel(const T& s, const T& g) {
  const float dr = s.x - g.x, dg = s.y - g.y, db = s.z - g.z;
  return (((dr * dr) + (dg * dg)) + (db * db)) / 3.0f;
}
// the wave's order on a host: value(k) is element k of `count`; the sum the wave's lane 0 ends with
template <class F>
inline float error_reduce(int64_t count, F value) {
  float v[64];
  for (int l = 0; l < 64; ++l) {
    v[l] = 0.0f;
    for (int64_t k = l; k < count; k += 64) v[l] = v[l] + value(k);
  }
  for (int s = 32; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) v[l] = v[l] + v[l + s];
  return v[0];
}

// ---- the launches (nrf_kernels_overlay.hip): a HIP error code each; every pointer is a device pointer
//   image: iw x ih texels of `type`; table: the 256 floats of overlay_srgb8_table (IMG_BYTE only); surface: float4 [H][W]
int launch_overlay_image(const OverlayImage& A, const void* image, int type, const float* table, void* surface, void* stream);
//   map: float [mh][mw]; average: one float
int launch_overlay_false_color(const OverlayFalseColor& A, const float* map, const float* average, void* surface, void* stream);
//   surface, truth: float4 [H][W]; map: float [mh][mw] and average: one float, both written
int launch_error_map(int W, int H, int mw, int mh, const void* surface, const void* truth, float* map, float* average, void* stream);

}  // namespace nrf
