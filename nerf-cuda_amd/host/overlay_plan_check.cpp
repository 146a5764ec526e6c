// Sanitizer driver of csrc/nrf_overlay_plan.h (make overlay_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the definition
// of the render buffer's image overlay, false-colour overlay and error map (nrf_rb_overlay_image, nrf_rb_overlay_false_color,
// nrf_rb_error_map) -- the pixel mapping with its saturating conversion, read_rgba with the Byte table, the blend over the background, the
// five-argument tonemap, the two colour maps, the cell bounds and the wave's order of the reduction -- compiled from the text the kernels
// compile.  Any number of cases on stdin; sizes and enumerators are decimal, every fp32 value is its bit pattern in hexadecimal:
//     I  W H iw ih type fov_axis render_space display_space curve   alpha zoom center_x center_y  e0 e1 e2  bg0 bg1 bg2 bg3
//        W * H surface texels (four words each, row-major), then iw * ih image texels: type 1 (Byte) one uint32 word each, type 2 (Half)
//        four 16-bit words each, type 3 (Float) four words each
//     F  W H tw th mw mh fov_axis viridis   brightness average
//        W * H surface texels, then mw * mh map values
//     E  W H mw mh
//        W * H surface texels, then W * H truth texels
// and on stdout, per case:
//     I, F   one line per surface pixel, row-major: srcx srcy (decimal) and the bits of the pixel's four channels afterwards
//     E      "map 0" where the map's size is out of range, else "map 1", one line of bits per cell, row-major, and "average" with its bits
// The background decode, 2^exposure and the Byte table are made here as the library makes them on the host (libm).
// tests/test_overlay_cpu.py holds the output to the numpy replay the GPU tests use (tests/overlay_replay.py).  Built with
// -ffp-contract=off, as the library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_overlay_plan.h"

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
static bool read_words(uint32_t* u, int n) {
  for (int k = 0; k < n; ++k)
    if (std::scanf("%" SCNx32, &u[k]) != 1) return false;
  return true;
}
static bool read_floats(float* f, int n) {
  for (int k = 0; k < n; ++k) {
    uint32_t u;
    if (!read_words(&u, 1)) return false;
    f[k] = as_float(u);
  }
  return true;
}
static bool read_plane(std::vector<Texel>& plane) {
  for (Texel& t : plane) {
    float f[4];
    if (!read_floats(f, 4)) return false;
    t = {f[0], f[1], f[2], f[3]};
  }
  return true;
}
static bool size_ok(int v) { return v > 0 && v <= nrf::OVERLAY_SIZE_MAX; }
static bool plane_ok(int w, int h) { return size_ok(w) && size_ok(h) && (int64_t)w * h <= (1 << 22); }
static void print_pixel(int srcx, int srcy, const Texel& o) {
  std::printf("%d %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", srcx, srcy, as_bits(o.x), as_bits(o.y), as_bits(o.z), as_bits(o.w));
}

static int overlay_image_case() {
  int W, H, iw, ih, type, axis, render_space, display_space, curve;
  if (std::scanf("%d %d %d %d %d %d %d %d %d", &W, &H, &iw, &ih, &type, &axis, &render_space, &display_space, &curve) != 9) return 2;
  float p[11];
  if (!read_floats(p, 11)) return 2;
  if (!plane_ok(W, H) || !plane_ok(iw, ih) || type < nrf::IMG_BYTE || type > nrf::IMG_FLOAT || (axis != 0 && axis != 1)) return 2;
  nrf::OverlayImage A{};
  A.map = {W, H, iw, ih, axis, p[1], p[2], p[3]};
  A.alpha = p[0];
  for (int k = 0; k < 3; ++k) A.gain[k] = powf(2.0f, p[4 + k]);
  const float given[4] = {p[7], p[8], p[9], p[10]};
  nrf::overlay_background(given, render_space, A.bg);
  A.render_space = render_space, A.display_space = display_space;
  A.film = nrf::film_curve(curve);
  std::vector<Texel> surface((size_t)W * H);
  if (!read_plane(surface)) return 2;
  const size_t texels = (size_t)iw * ih;
  std::vector<uint32_t> bytes;
  std::vector<uint64_t> halves;
  std::vector<Texel> floats;
  if (type == nrf::IMG_BYTE) {
    bytes.resize(texels);
    if (!read_words(bytes.data(), (int)texels)) return 2;
  } else if (type == nrf::IMG_HALF) {
    halves.resize(texels);
    for (uint64_t& t : halves) {
      uint32_t u[4];
      if (!read_words(u, 4) || (u[0] | u[1] | u[2] | u[3]) > 0xFFFFu) return 2;
      t = (uint64_t)u[0] | (uint64_t)u[1] << 16 | (uint64_t)u[2] << 32 | (uint64_t)u[3] << 48;
    }
  } else {
    floats.resize(texels);
    if (!read_plane(floats)) return 2;
  }
  float table[256];
  nrf::overlay_srgb8_table(table);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int srcx, srcy;
      nrf::overlay_source(A.map, x, y, srcx, srcy);
      Texel val{0.f, 0.f, 0.f, 0.f};
      if (nrf::overlay_inside(srcx, srcy, iw, ih)) {
        const size_t at = (size_t)srcx + (size_t)iw * (size_t)srcy;
        if (type == nrf::IMG_BYTE) val = nrf::overlay_read_byte<Texel>(bytes.at(at), table);
        else if (type == nrf::IMG_HALF) val = nrf::overlay_read_half<Texel>(halves.at(at));
        else val = floats.at(at);
      }
      print_pixel(srcx, srcy, nrf::overlay_image_pixel(A, val, surface.at((size_t)y * W + x)));
    }
  std::fprintf(stderr, "overlay_plan_check: image %d x %d of type %d over %d x %d\n", iw, ih, type, W, H);
  return 0;
}

static int false_color_case() {
  nrf::OverlayFalseColor A{};
  if (std::scanf("%d %d %d %d %d %d %d %d", &A.W, &A.H, &A.tw, &A.th, &A.mw, &A.mh, &A.fov_axis, &A.viridis) != 8) return 2;
  float p[2];
  if (!read_floats(p, 2)) return 2;
  if (!plane_ok(A.W, A.H) || !size_ok(A.tw) || !size_ok(A.th) || A.mw < 1 || A.mw > nrf::ERROR_MAP_MAX || A.mh < 1 || A.mh > nrf::ERROR_MAP_MAX ||
      (A.fov_axis != 0 && A.fov_axis != 1))
    return 2;
  A.brightness = p[0];
  std::vector<Texel> surface((size_t)A.W * A.H);
  if (!read_plane(surface)) return 2;
  std::vector<float> map((size_t)A.mw * A.mh);
  if (!read_floats(map.data(), (int)map.size())) return 2;
  const float error_map_scale = nrf::overlay_error_scale(A.brightness, p[1]);
  for (int y = 0; y < A.H; ++y)
    for (int x = 0; x < A.W; ++x) {
      int srcx, srcy;
      nrf::overlay_false_color_source(A, x, y, srcx, srcy);
      Texel o = surface.at((size_t)y * A.W + x);
      if (nrf::overlay_inside(srcx, srcy, A.mw, A.mh)) o = nrf::overlay_false_color_pixel(A, map.at((size_t)srcx + (size_t)A.mw * (size_t)srcy), error_map_scale, o);
      print_pixel(srcx, srcy, o);
    }
  std::fprintf(stderr, "overlay_plan_check: false colours of %d x %d cells over %d x %d\n", A.mw, A.mh, A.W, A.H);
  return 0;
}

static int error_map_case() {
  int W, H, mw, mh;
  if (std::scanf("%d %d %d %d", &W, &H, &mw, &mh) != 4) return 2;
  if (!plane_ok(W, H)) return 2;
  std::vector<Texel> surface((size_t)W * H), truth((size_t)W * H);
  if (!read_plane(surface) || !read_plane(truth)) return 2;
  if (!nrf::error_map_axis_valid(W, mw) || !nrf::error_map_axis_valid(H, mh)) {
    std::printf("map 0\n");
    return 0;
  }
  std::printf("map 1\n");
  std::vector<float> map((size_t)mw * mh);
  size_t covered = 0;
  for (int cy = 0; cy < mh; ++cy)
    for (int cx = 0; cx < mw; ++cx) {
      const int x0 = nrf::error_cell_begin(cx, W, mw), y0 = nrf::error_cell_begin(cy, H, mh);
      const int cw = nrf::error_cell_begin(cx + 1, W, mw) - x0, ch = nrf::error_cell_begin(cy + 1, H, mh) - y0;
      if (cw < 1 || ch < 1) {
        std::fprintf(stderr, "overlay_plan_check: an empty cell at (%d, %d)\n", cx, cy);
        return 3;
      }
      const int64_t count = (int64_t)cw * ch;
      covered += (size_t)count;
      const float sum = nrf::error_reduce(count, [&](int64_t k) {
        const size_t at = (size_t)(y0 + (int)(k / cw)) * W + (size_t)(x0 + (int)(k % cw));
        return nrf::error_pixel(surface.at(at), truth.at(at));
      });
      map[(size_t)cy * mw + cx] = sum / (float)count;
      std::printf("%08" PRIx32 "\n", as_bits(map[(size_t)cy * mw + cx]));
    }
  if (covered != surface.size()) {
    std::fprintf(stderr, "overlay_plan_check: the cells cover %zu of %zu pixels\n", covered, surface.size());
    return 3;
  }
  const float sum = nrf::error_reduce((int64_t)map.size(), [&](int64_t k) { return map.at((size_t)k); });
  std::printf("average %08" PRIx32 "\n", as_bits(sum / (float)(mw * mh)));
  std::fprintf(stderr, "overlay_plan_check: error map %d x %d -> %d x %d\n", W, H, mw, mh);
  return 0;
}

int main() {
  char mode;
  int cases = 0;
  while (std::scanf(" %c", &mode) == 1) {
    int rc;
    if (mode == 'I') rc = overlay_image_case();
    else if (mode == 'F') rc = false_color_case();
    else if (mode == 'E') rc = error_map_case();
    else rc = 2;
    if (rc != 0) {
      std::fprintf(stderr, "overlay_plan_check: case %d (mode %c) is malformed or fails its own checks\n", cases, mode);
      return rc;
    }
    ++cases;
  }
  if (cases == 0) {
    std::fprintf(stderr, "overlay_plan_check: no case\n");
    return 2;
  }
  std::fprintf(stderr, "overlay_plan_check: %d cases\n", cases);
  return 0;
}
