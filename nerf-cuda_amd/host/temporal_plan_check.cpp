// Sanitizer driver of csrc/nrf_temporal_plan.h (make temporal_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the definition
// of the render buffer's temporal upscaler (nrf_rb_upscale_temporal), of its jitter sequence and of the motion vectors of a static scene
// (nrf_motion_vectors), compiled from the text the kernels compile.  One case on stdin, decimal integers and fp32 bit patterns (hex):
//     T in_width in_height out_width out_height amount max_history n_frames
//       per frame: jitter_x jitter_y flags have_motion, in_height * in_width texels of four words, then (have_motion) as many pairs
//     J count
//     M in_width in_height out_width out_height min_alpha scale, then pose (16) cam (4) prev_pose (16) prev_cam (4),
//       then in_height * in_width rows of: o (3) d (3) alpha depth
// and on stdout:
//     plan 0                   the case is out of range (resolutions, amount, history length, a jitter, a flag, min_alpha)
//     T: plan 1 rx ry ox oy    then per frame and output texel, row-major: H' (4) Wt' presented (4) rgba8
//     J: one line per index    jitter_x jitter_y
//     M: plan 1 ox oy          then per render pixel: m_x m_y
// The history starts empty: frame 0 is a reset whatever its flags say, as the first nrf_rb_upscale_temporal of a buffer is.
// tests/test_temporal_cpu.py holds the output to the numpy replay the GPU tests use (tests/temporal_replay.py).  Built with
// -ffp-contract=off, as the library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_temporal_plan.h"

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
static bool read_float(float& f) {
  uint32_t u;
  if (std::scanf("%" SCNx32, &u) != 1) return false;
  f = as_float(u);
  return true;
}
static bool read_floats(float* f, int n) {
  for (int k = 0; k < n; ++k)
    if (!read_float(f[k])) return false;
  return true;
}

static int run_temporal() {
  int iw, ih, ow, oh, n_frames;
  float amount, max_history;
  if (std::scanf("%d %d %d %d", &iw, &ih, &ow, &oh) != 4 || !read_float(amount) || !read_float(max_history) || std::scanf("%d", &n_frames) != 1) return 2;
  nrf::TemporalPlan T;
  if (!nrf::temporal_plan(iw, ih, ow, oh, amount, 0.0f, 0.0f, max_history, 0u, T)) {
    std::printf("plan 0\n");
    return 0;
  }
  if ((int64_t)ow * oh > (1 << 22) || n_frames < 0 || n_frames > 64) {
    std::fprintf(stderr, "temporal_plan_check: more than 2^22 output texels or 64 frames\n");
    return 2;
  }
  std::printf("plan 1 %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", as_bits(T.U.rx), as_bits(T.U.ry), as_bits(T.ox), as_bits(T.oy));
  const size_t n_in = (size_t)iw * ih, n_out = (size_t)ow * oh;
  std::vector<Texel> src(n_in), hist[2] = {std::vector<Texel>(n_out, Texel{0, 0, 0, 0}), std::vector<Texel>(n_out, Texel{0, 0, 0, 0})};
  std::vector<float> motion(2 * n_in), weight[2] = {std::vector<float>(n_out, 0.0f), std::vector<float>(n_out, 0.0f)};
  int latest = 0;
  for (int frame = 0; frame < n_frames; ++frame) {
    float jx, jy;
    unsigned flags;
    int have_motion;
    if (!read_float(jx) || !read_float(jy) || std::scanf("%u %d", &flags, &have_motion) != 2) return 2;
    if (frame == 0) flags |= nrf::TEMPORAL_RESET;
    if (!nrf::temporal_plan(iw, ih, ow, oh, amount, jx, jy, max_history, flags, T)) {
      std::printf("plan 0\n");
      return 0;
    }
    for (Texel& t : src) {
      float v[4];
      if (!read_floats(v, 4)) return 2;
      t = {v[0], v[1], v[2], v[3]};
    }
    if (have_motion && !read_floats(motion.data(), (int)(2 * n_in))) return 2;
    const std::vector<Texel>& hp = hist[latest];
    const std::vector<float>& wp = weight[latest];
    std::vector<Texel>& hn = hist[1 - latest];
    std::vector<float>& wn = weight[1 - latest];
    const auto at = [&](int y, int x) -> const Texel& { return src.at((size_t)y * iw + x); };
    for (int Y = 0; Y < oh; ++Y) {
      int iy, ny, cy[4];
      float fy, dy, wy[4];
      nrf::temporal_source(Y, T.U.ry, T.jy, T.oy, ih, iy, fy, ny, dy);
      nrf::upscale_taps(iy, ih, cy);
      nrf::upscale_weights(fy, wy);
      for (int X = 0; X < ow; ++X) {
        int ix, nx, cx[4];
        float fx, dx, wx[4];
        nrf::temporal_source(X, T.U.rx, T.jx, T.ox, iw, ix, fx, nx, dx);
        nrf::upscale_taps(ix, iw, cx);
        nrf::upscale_weights(fx, wx);
        if (!(fx >= 0.0f && fx <= 1.0f && fy >= 0.0f && fy <= 1.0f) || ix < -1 || ix > iw - 1 || iy < -1 || iy > ih - 1) {
          std::fprintf(stderr, "temporal_plan_check: a fraction or a base out of range at (%d, %d)\n", X, Y);
          return 3;
        }
        Texel h[4];
        for (int j = 0; j < 4; ++j) h[j] = nrf::upscale_row(wx, at(cy[j], cx[0]), at(cy[j], cx[1]), at(cy[j], cx[2]), at(cy[j], cx[3]));
        Texel out = nrf::upscale_column(wy, h[0], h[1], h[2], h[3], at(cy[1], cx[1]), at(cy[1], cx[2]), at(cy[2], cx[1]), at(cy[2], cx[2]));
        const float wc = nrf::temporal_sample_weight(dx, dy);
        float w_out = wc, mx = 0.0f, my = 0.0f;
        if (have_motion && !(T.flags & nrf::TEMPORAL_RESET)) mx = motion.at(2 * ((size_t)ny * iw + nx)), my = motion.at(2 * ((size_t)ny * iw + nx) + 1);
        const nrf::HistoryFetch F = nrf::temporal_history_fetch(X, Y, have_motion != 0, mx, my, ow, oh, T.flags);
        Texel hq = out;
        float wq = 0.0f;
        if (F.kind == nrf::HISTORY_TEXEL) {
          hq = hp.at((size_t)Y * ow + X);
          wq = wp.at((size_t)Y * ow + X);
        } else if (F.kind == nrf::HISTORY_RESAMPLE) {
          int qx[4], qy[4];
          float vx[4], vy[4];
          nrf::upscale_taps(F.bx, ow, qx);
          nrf::upscale_taps(F.by, oh, qy);
          nrf::upscale_weights(F.fx, vx);
          nrf::upscale_weights(F.fy, vy);
          const auto hat = [&](int j, int a) -> const Texel& { return hp.at((size_t)qy[j] * ow + qx[a]); };
          Texel g[4];
          for (int j = 0; j < 4; ++j) g[j] = nrf::upscale_row(vx, hat(j, 0), hat(j, 1), hat(j, 2), hat(j, 3));
          hq = nrf::upscale_column(vy, g[0], g[1], g[2], g[3], hat(1, 1), hat(1, 2), hat(2, 1), hat(2, 2));
          wq = wp.at((size_t)F.wy * ow + F.wx);
        }
        const float wh = nrf::temporal_history_weight(wq, T.max_history);
        if (wh > 0.0f) {
          if (T.flags & nrf::TEMPORAL_RECTIFY) {
            Texel lo = at(nrf::upscale_clamp_index(ny - 1, ih), nrf::upscale_clamp_index(nx - 1, iw)), hi = lo;
            for (int j = -1; j <= 1; ++j)
              for (int a = -1; a <= 1; ++a)
                if (j != -1 || a != -1) nrf::temporal_fold_range(at(nrf::upscale_clamp_index(ny + j, ih), nrf::upscale_clamp_index(nx + a, iw)), lo, hi);
            hq = nrf::temporal_rectify(hq, lo, hi);
          }
          out = nrf::temporal_blend(hq, out, wh, wc, w_out);
        }
        hn.at((size_t)Y * ow + X) = out;
        wn.at((size_t)Y * ow + X) = w_out;
      }
    }
    for (int Y = 0; Y < oh; ++Y)
      for (int X = 0; X < ow; ++X) {
        const int n = nrf::upscale_clamp_index(Y - 1, oh), s = nrf::upscale_clamp_index(Y + 1, oh);
        const int w = nrf::upscale_clamp_index(X - 1, ow), e = nrf::upscale_clamp_index(X + 1, ow);
        const Texel& c = hn.at((size_t)Y * ow + X);
        const Texel o = nrf::upscale_sharpen(c, hn.at((size_t)n * ow + X), hn.at((size_t)s * ow + X), hn.at((size_t)Y * ow + w), hn.at((size_t)Y * ow + e), T.U.amount);
        std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n",
                    as_bits(c.x), as_bits(c.y), as_bits(c.z), as_bits(c.w), as_bits(wn.at((size_t)Y * ow + X)), as_bits(o.x), as_bits(o.y), as_bits(o.z),
                    as_bits(o.w), nrf::upscale_rgba8(o));
      }
    latest = 1 - latest;
  }
  std::fprintf(stderr, "temporal_plan_check: %d x %d -> %d x %d, %d frames\n", iw, ih, ow, oh, n_frames);
  return 0;
}

static int run_jitter() {
  int count;
  if (std::scanf("%d", &count) != 1 || count < 0 || count > (1 << 20)) return 2;
  for (int k = 0; k < count; ++k) {
    float j[2];
    nrf::temporal_jitter((uint32_t)k, j);
    std::printf("%08" PRIx32 " %08" PRIx32 "\n", as_bits(j[0]), as_bits(j[1]));
  }
  return 0;
}

static int run_motion() {
  int iw, ih, ow, oh;
  float min_alpha, scale, pose[16], cam[4], prev_pose[16], prev_cam[4];
  if (std::scanf("%d %d %d %d", &iw, &ih, &ow, &oh) != 4 || !read_float(min_alpha) || !read_float(scale)) return 2;
  if (!read_floats(pose, 16) || !read_floats(cam, 4) || !read_floats(prev_pose, 16) || !read_floats(prev_cam, 4)) return 2;
  nrf::MotionPlan M;
  if (!nrf::motion_plan(iw, ih, ow, oh, min_alpha, M)) {
    std::printf("plan 0\n");
    return 0;
  }
  if ((int64_t)iw * ih > (1 << 22)) return 2;
  nrf::motion_camera(pose, scale, cam, M.cur);
  nrf::motion_camera(prev_pose, scale, prev_cam, M.prev);
  std::printf("plan 1 %08" PRIx32 " %08" PRIx32 "\n", as_bits(M.ox), as_bits(M.oy));
  for (int i = 0; i < iw * ih; ++i) {
    float v[8];
    if (!read_floats(v, 8)) return 2;
    const float o[3] = {v[0], v[1], v[2]}, d[3] = {v[3], v[4], v[5]};
    float mx, my;
    nrf::motion_vector(M, o, d, v[6], v[7], mx, my);
    std::printf("%08" PRIx32 " %08" PRIx32 "\n", as_bits(mx), as_bits(my));
  }
  std::fprintf(stderr, "temporal_plan_check: %d x %d motion vectors\n", iw, ih);
  return 0;
}

int main() {
  char mode[4] = {0, 0, 0, 0};
  if (std::scanf("%3s", mode) != 1) {
    std::fprintf(stderr, "temporal_plan_check: no case\n");
    return 2;
  }
  int rc = 2;
  if (mode[0] == 'T' && !mode[1]) rc = run_temporal();
  else if (mode[0] == 'J' && !mode[1]) rc = run_jitter();
  else if (mode[0] == 'M' && !mode[1]) rc = run_motion();
  if (rc == 2) std::fprintf(stderr, "temporal_plan_check: malformed input\n");
  return rc;
}
