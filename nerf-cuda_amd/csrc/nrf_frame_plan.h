// nrf_frame_plan.h -- how a render call becomes launches, work queues and host-frame copies, without a device (plain C++17: a host
// compiler builds it alone).  Frame geometry (tiles, strips, shards), a view's region of interest, the queues of a persistent
// launch, the per-call rules and the copies / fills of a host frame: pure functions of ints and floats.  nrf_api.hip and
// nrf_kernels.hip's launch_render copy the results into ViewParams / ViewBatch / FrameParams and make the HIP calls;
// nrf_debug_frame_plan returns them (tests/test_frame_plan_cpu.py), host/frame_plan_asan.cpp runs them under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nrf {

// ---- frame geometry: 8x8 pixel tiles, strips of 4 tiles along x, strips dealt round-robin to the shards ----
constexpr long long QUEUE_POS_LIMIT = 0xffffff;  // the persistent kernel's queue positions (strip rows of all views x strips per row) are 24-bit
constexpr long long PLAN_LDS_LIMIT = 60 * 1024;  // what a planned launch may stage: a bin per position (plan_sort_kernel), the dilated table (plan_price_kernel)

inline int tiles_of(int px) { return (px + 7) / 8; }
inline int strips_per_row(int tiles_x) { return (tiles_x + 3) / 4; }
inline int total_strips(int W, int H) { return strips_per_row(tiles_of(W)) * tiles_of(H); }

inline int local_tiles(int W, int H, int shard_index, int shard_count) {
  const int total = total_strips(W, H);
  if (shard_index >= total) return 0;
  return 4 * ((total - shard_index + shard_count - 1) / shard_count);
}

inline int tiles_per_shard(int W, int H, int shard_count) { return 4 * ((total_strips(W, H) + shard_count - 1) / shard_count); }

inline int blocks_per_view(int n_local_tiles, int render_waves) { return (n_local_tiles + render_waves - 1) / render_waves; }

// views per launch: max_views, fewer when the frames are so large that the queue positions would not hold the launch
inline int views_per_launch(int tiles_x, int tiles_y, int max_views) {
  int per_launch = max_views;
  const long long per_view = (long long)tiles_y * strips_per_row(tiles_x);
  if (per_view * per_launch >= QUEUE_POS_LIMIT) per_launch = (int)std::max(1LL, (QUEUE_POS_LIMIT - 1) / std::max(per_view, 1LL));
  return per_launch;
}

// ---- regions of interest ----
inline bool roi_empty(const int roi[4]) { return roi[2] < roi[0] || roi[3] < roi[1]; }
inline void roi_clear(int roi[4]) {
  roi[0] = roi[1] = 0;
  roi[2] = roi[3] = -1;
}

// Pixel rectangle outside of which no ray of the view can enter `box` (the inflated box of occupied cells,
// NGP coordinates): the bounding rectangle of the projections of its 8 corners, 3 pixels wider on every side;
// the whole image when a corner is not safely in front of the camera; empty when the box is.  Conservative
// by construction: the box is convex, so a ray that enters it passes through the convex hull of the projected
// corners; rays inside the rectangle still take the exact per-ray slab test in the kernel.
inline void view_roi(const float R[9], const float org[3], const float cam[4], const float box[6], int W, int H, int roi[4]) {
  roi[0] = 0; roi[1] = 0; roi[2] = W - 1; roi[3] = H - 1;
  if (!(box[0] <= box[3])) {  // no occupied cell at all
    roi[2] = -1;
    roi[3] = -1;
    return;
  }
  // camera coordinates of a world offset p: v = R^-1 p (ray_dir applies R to the camera-space direction; poses
  // need not be orthonormal, so the inverse is computed, not assumed to be the transpose)
  const double a = R[0], b = R[1], cc = R[2], d = R[3], e = R[4], f = R[5], g = R[6], h = R[7], i = R[8];
  const double det = a * (e * i - f * h) - b * (d * i - f * g) + cc * (d * h - e * g);
  if (!(std::fabs(det) > 1e-12)) return;
  const double inv[9] = {(e * i - f * h) / det, (cc * h - b * i) / det, (b * f - cc * e) / det,
                         (f * g - d * i) / det, (a * i - cc * g) / det, (cc * d - a * f) / det,
                         (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
  double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
  for (int c = 0; c < 8; ++c) {
    const double p[3] = {(double)box[(c & 1) ? 3 : 0] - org[0], (double)box[(c & 2) ? 4 : 1] - org[1],
                         (double)box[(c & 4) ? 5 : 2] - org[2]};
    const double vx = inv[0] * p[0] + inv[1] * p[1] + inv[2] * p[2];
    const double vy = inv[3] * p[0] + inv[4] * p[1] + inv[5] * p[2];
    const double vz = inv[6] * p[0] + inv[7] * p[1] + inv[8] * p[2];
    if (!(vz > 1e-3)) return;  // corner beside / behind the camera (or NaN): keep the whole image
    const double u = cam[2] + cam[0] * vx / vz, v = cam[3] + cam[1] * vy / vz;
    if (!(u == u) || !(v == v)) return;
    lo[0] = u < lo[0] ? u : lo[0]; hi[0] = u > hi[0] ? u : hi[0];
    lo[1] = v < lo[1] ? v : lo[1]; hi[1] = v > hi[1] ? v : hi[1];
  }
  // pixel (i, j) looks through (i + 0.5, j + 0.5)
  const double m = 3.0;
  const double x0 = std::floor(lo[0] - 0.5 - m), y0 = std::floor(lo[1] - 0.5 - m);
  const double x1 = std::ceil(hi[0] - 0.5 + m), y1 = std::ceil(hi[1] - 0.5 + m);
  roi[0] = x0 < 0 ? 0 : (x0 > W ? W : (int)x0);
  roi[1] = y0 < 0 ? 0 : (y0 > H ? H : (int)y0);
  roi[2] = x1 < -1 ? -1 : (x1 > W - 1 ? W - 1 : (int)x1);
  roi[3] = y1 < -1 ? -1 : (y1 > H - 1 ? H - 1 : (int)y1);
}

// A camera thousands of scene sizes away: t + dt == t in fp32 once t passes ~2^24 dt (dt_min = 0.0034: t ~ 5.7e4), the
// march of render_utils.h:593-653 stops advancing and never ends (the reference hangs there; so would the kernel).
// Long before that the object is far below a pixel: such a view is background (an empty region of interest).
// max_distance: nrf_device.h MAX_CAMERA_DISTANCE; a NaN origin counts as too far.
inline void far_camera_roi(const float org[3], float max_distance, int roi[4]) {
  const float far2 = org[0] * org[0] + org[1] * org[1] + org[2] * org[2];
  if (!(far2 <= max_distance * max_distance)) roi_clear(roi);
}

// the strip rows [ty0, ty1] (inclusive) a region of interest touches; ty1 < ty0: none
struct StripRows { int ty0, ty1; };
inline StripRows roi_strip_rows(const int roi[4], int tiles_y) {
  if (roi_empty(roi)) return {0, -1};
  return {std::max(roi[1] >> 3, 0), std::min(roi[3] >> 3, tiles_y - 1)};
}

// the rows [lo, hi) of a frame that the strip rows of a view's region of interest cover (what plan_queues queues for the
// persistent kernel); every pixel outside them is the background
inline void roi_rows(const int roi[4], int H, int& lo, int& hi) {
  lo = hi = 0;
  const StripRows s = roi_strip_rows(roi, tiles_of(H));
  if (s.ty1 < s.ty0) return;
  lo = 8 * s.ty0;
  hi = std::min(H, 8 * (s.ty1 + 1));
}

// the columns [x0, x1) of whole tiles a view's region of interest touches: the tiles beside them are background (the kernel tests
// every tile's 8x8 pixels against the region)
inline void roi_cols(const int roi[4], int W, int& x0, int& x1) {
  x0 = x1 = 0;
  if (roi_empty(roi)) return;
  const int tx0 = std::max(roi[0] >> 3, 0), tx1 = std::min(roi[2] >> 3, tiles_of(W) - 1);
  if (tx1 < tx0) return;
  x0 = 8 * tx0;
  x1 = std::min(W, 8 * (tx1 + 1));
}

// ---- the work queues of a persistent launch ----
// per view: its local tiles [k_lo, k_hi) and its queue units [q_begin, q_begin + q_rows) = the strip rows from q_row0 on
struct ViewQueue { int k_lo, k_hi, q_begin, q_rows, q_row0; };
struct QueueInputs {
  int tiles_x, tiles_y, shard_index, shard_count, n_local_tiles;
  int queue_classes;              // FrameParams::queue_classes: 1 .. 8, anything else: 8
  int n_cus, persist_waves;       // DevModel's
  int render_waves;               // nrf_render.h RENDER_WAVES
};
struct QueuePlan {
  int q_total, n_classes, class_cols;
  int workgroups, blocks_per_view;
  long long n_pos;  // queue positions: units x class_cols
  bool refused;     // n_pos does not fit QUEUE_POS_LIMIT: the launch is an error (views_per_launch keeps render calls below it)
};

// rois: [n_views][4]; views: [n_views].  Units are the strip rows the regions of interest touch (sharded: the local strips of those rows)
inline QueuePlan plan_queues(const QueueInputs& in, int n_views, const int* rois, ViewQueue* views) {
  QueuePlan Q{};
  Q.blocks_per_view = blocks_per_view(in.n_local_tiles, in.render_waves);
  const int strips_x = strips_per_row(in.tiles_x), N = in.shard_count, idx = in.shard_index;
  const int k_end = (in.n_local_tiles + 3) & ~3;
  int q = 0;
  for (int v = 0; v < n_views; ++v) {
    ViewQueue& V = views[v];
    V.k_lo = V.k_hi = 0;
    int rows = 0, row0 = 0;
    const StripRows s = roi_strip_rows(rois + 4 * v, in.tiles_y);
    if (s.ty1 >= s.ty0) {
      rows = s.ty1 - s.ty0 + 1;
      row0 = s.ty0;
      const int s0 = s.ty0 * strips_x, s1 = (s.ty1 + 1) * strips_x;  // global strips [s0, s1)
      const int ls0 = s0 > idx ? (s0 - idx + N - 1) / N : 0, ls1 = s1 > idx ? (s1 - idx + N - 1) / N : 0;
      V.k_lo = std::min(4 * ls0, k_end);
      V.k_hi = std::min(4 * ls1, k_end);
    }
    V.q_begin = q;
    V.q_rows = rows;
    V.q_row0 = row0;
    q += rows;
  }
  Q.q_total = q;
  Q.n_classes = in.queue_classes >= 1 && in.queue_classes <= 8 ? in.queue_classes : 8;
  Q.class_cols = (strips_x + N - 1) / N;  // a row holds at most this many of the rank's strips
  Q.n_pos = (long long)q * Q.class_cols;
  Q.refused = Q.n_pos >= QUEUE_POS_LIMIT;
  const long long tiles = (long long)in.n_local_tiles * n_views;
  Q.workgroups = (int)std::max(1LL, std::min((long long)in.n_cus, (tiles + in.persist_waves - 1) / in.persist_waves));
  return Q;
}

// whether the queue order of a launch is planned (dearest strips first: nrf_kernels.hip "queue planning") -- have_plan: the call's
// first launch, with a plan buffer and a dilated table; plan_cap: positions the buffer holds; dil_bytes: the dilated table, all cascades
inline bool launch_is_planned(bool have_plan, long long n_pos, long long plan_cap, long long dil_bytes) {
  return have_plan && n_pos > 0 && n_pos <= plan_cap && n_pos <= PLAN_LDS_LIMIT && dil_bytes <= PLAN_LDS_LIMIT;
}

// ---- per-call rules ----
// One or two views alone are latency-bound, not throughput-bound: their last tiles end sooner when every ray queues its full
// eight samples per round, and the few samples evaluated for nothing cost nobody anything (0.904 against 0.914 ms per 1080p view)
// ... unless the launch has fewer tiles than the chip has waves: it is ALL tail (idle waves take rays off the rendering ones from
// the first round on, and every split group queues its own eight samples per ray behind a terminating one) -- small frames
// keep the transmittance-dependent queue, which holds their evaluated samples within 15 % of the composited ones
// (tests/test_parity_gpu.py, test_generic_gpu.py, test_golden.py; pixels cannot depend on it: tests/test_persistent_gpu.py)
inline bool call_is_all_tail(int n_local_tiles, int n_views, int n_cus, unsigned persist_waves) {
  return (long long)n_local_tiles * n_views < (long long)n_cus * std::max(1u, persist_waves);
}
inline bool drops_sample_cap(int n_local_tiles, int n_views, int n_cus, unsigned persist_waves, bool forced) {
  return n_views <= 2 && !forced && !call_is_all_tail(n_local_tiles, n_views, n_cus, persist_waves);
}
// nrf_ray_hits (FrameParams::hit_exp): a ray stops once its weight sum is >= opacity, that is at T <= 1 - opacity, so the per-round
// queue of sample_cap == 2 holds what the ray needs to get THERE if every sample halves T: clamp(exponent(T) - hit_cap_exponent, 1, 8),
// with the frexp exponent of the fp32 difference 1 - opacity (0.5 -> 0, 0.9 -> -3, 0.99 -> -6, nextafter(1, 0) -> -23).
// Like the rule for T < 1e-4 it compares exponents and ignores the two mantissas: the queue can be one halving short of the need,
// never more (host/hit_cap_asan.cpp).  Pixels cannot depend on it, only the samples evaluated behind a ray's last one.
// opacity == 1 (the difference is 0 and has no exponent) and anything outside (0, 1) keep today's rule, -13: T < 1e-4 = 2^-13.3.
constexpr int SAMPLE_CAP_EXPONENT = -13;
inline int hit_cap_exponent(float opacity) {
  if (!(opacity > 0.0f && opacity < 1.0f)) return SAMPLE_CAP_EXPONENT;
  int e = 0;
  (void)std::frexp(1.0f - opacity, &e);
  return std::max(e, SAMPLE_CAP_EXPONENT);  // (no threshold asks for more samples than the ordinary termination allows)
}

// Whether a host frame's copies are progressive (issued by the waiting thread as the kernel flags strip rows) -- capable: the
// context allows it and the model renders in the persistent kernel with its tables in LDS.
// A launch whose queue order is PLANNED completes its rows within the last tenth of the render -- nothing to copy meanwhile, and
// copies that are already queued behind the render's event start sooner than ones the waiting thread issues when it sees the flags
// (one 1080p view: 1.09 against 1.14 ms per call; three views and more, which are not planned: 2.54 against 2.98 the other way round)
// ... and two views gain next to nothing from the plan on the device (1.64 against 1.67 ms) while it costs their host end
// the progressive copies (2.00 against 1.82 ms per call): only a frame rendered alone is planned here, every larger call
// keeps the queue order of its views and copies them as they complete (render_views_impl: no plan with progress reporting).
// The strip count here is the whole frame's, n_views * tiles_y * ceil(W / 32): NOT plan_queues' n_pos (the region's strip rows x
// the rank's strips per row), which launch_is_planned compares with the same capacity.  Both stay as they are.
inline bool host_frame_progressive(bool capable, int n_views, int W, int tiles_y, long long plan_max_pos) {
  const long strips = (long)n_views * tiles_y * ((W + 31) / 32);
  if (n_views == 1 && plan_max_pos > 0 && strips <= (long)plan_max_pos) return false;
  return capable;
}

// ---- host-frame copies ----
struct Band { int view, lo, hi, s0, s1; };  // pixel rows [lo, hi) = strip rows [s0, s1) of the view

// The bands of a progressive call -- rows: per view {row lo, row hi, ...} (stride 4).
// ~16 bands per call (one view alone: bands of ~70 rows at 1080p; a batch of 16 views: one band per view), but no copy
// below 64 KiB: the runtime moves smaller ones with a blit KERNEL, which gets no compute unit while the persistent render
// is resident -- it, and every copy queued behind it, would wait for the render's end (scripts/copy_overlap_probe2.py:
// 16 KiB copies issued during a 13 ms render all ended with it, 64 KiB ones ran beside it).  The smallest copy of a band
// is its depth plane (W bytes per row; rgb-only frames: 3 W).
inline std::vector<Band> plan_bands(int W, bool with_depth, int n_views, const int* rows) {
  std::vector<Band> bands;
  long total = 0;
  for (int v = 0; v < n_views; ++v) total += (rows[4 * v + 1] + 7) / 8 - rows[4 * v] / 8;
  const long want_rows = std::max(4L, (total + 15) / 16);  // strip rows per band
  const long row_bytes = (long)W * (with_depth ? 1 : 3);
  const long min_rows = (65536 + 8 * row_bytes - 1) / (8 * row_bytes);  // strip rows whose smallest plane is 64 KiB
  for (int v = 0; v < n_views; ++v) {
    const int lo = rows[4 * v], hi = rows[4 * v + 1];
    if (hi <= lo) continue;
    const long s_lo = lo / 8, s_hi = (hi + 7) / 8, n = s_hi - s_lo;
    const long per = std::max(want_rows, min_rows);
    const long n_bands = std::max(1L, n / per);  // (the remainder is spread over the bands: none is smaller than `per`)
    for (long b = 0; b < n_bands; ++b) {
      const int s0 = (int)(s_lo + n * b / n_bands), s1 = (int)(s_lo + n * (b + 1) / n_bands);
      bands.push_back({v, std::max(lo, 8 * s0), std::min(hi, 8 * s1), s0, s1});
    }
  }
  return bands;
}

// One plane's share of a row copy: `rows` pieces of `width` bytes, `pitch` bytes apart, from byte `off` of the slot's buffer
// (whole rows: one piece)
struct PlaneCopy {
  size_t off, pitch, width, rows;
  size_t bytes() const { return width * rows; }
};
// The rows [lo, hi) of view v of a host-frame slot (px = W * H pixels per view, `views` views; the depth planes follow the rgb
// planes of ALL views); x0 < x1 short of the frame's width: only the columns [x0, x1) of those rows, a pitched copy
struct RowCopy {
  bool pitched;
  PlaneCopy rgb, depth;
};
inline RowCopy row_copy(int W, size_t px, size_t views, int v, int lo, int hi, int x0, int x1) {
  const size_t Wb = (size_t)W, depth_off = views * px * 3;
  const bool cols = x1 > x0 && (x0 > 0 || x1 < W);
  const size_t ro = ((size_t)v * px + (size_t)lo * Wb) * 3, rn = (size_t)(hi - lo) * Wb * 3;
  const size_t dofs = depth_off + (size_t)v * px + (size_t)lo * Wb, dn = (size_t)(hi - lo) * Wb;
  if (cols) {
    const size_t wpx = (size_t)(x1 - x0), n_rows = (size_t)(hi - lo);
    return {true, {ro + (size_t)x0 * 3, Wb * 3, wpx * 3, n_rows}, {dofs + (size_t)x0, Wb, wpx, n_rows}};
  }
  return {false, {ro, rn, rn, 1}, {dofs, dn, dn, 1}};
}

// What a host-frame call fills with the background in one view's pinned planes.  They hold the background value except in the
// rectangle the copies of earlier calls have written (`prev`; all: the background itself changed, everything counts), so only
// that rectangle's difference to the new one is filled.  rows: {row lo, row hi, column lo, column hi} of the view's region of
// interest; use_cols: the call's copies write the region's columns, not whole rows.  now: the rectangle this call's copies write.
struct Rect { int r0, r1, c0, c1; };  // rows [r0, r1) x columns [c0, c1)
struct FillPlan {
  Rect rects[4];
  int n;
  Rect now;
};
inline FillPlan fill_rects(const Rect& prev, bool all, int W, int H, const int rows[4], bool use_cols) {
  FillPlan F{};
  auto fill = [&](int r0, int r1, int c0, int c1) {
    if (r1 <= r0 || c1 <= c0) return;
    F.rects[F.n++] = {r0, r1, c0, c1};
  };
  const int lo = rows[0], hi = rows[1];
  int x0 = use_cols ? rows[2] : 0, x1 = use_cols ? rows[3] : W;
  if (x1 <= x0) { x0 = 0; x1 = W; }
  const int plo = all ? 0 : prev.r0, phi = all ? H : prev.r1;
  const int pc0 = all ? 0 : prev.c0, pc1 = all ? W : prev.c1;
  if (hi <= lo) fill(plo, phi, pc0, pc1);
  else {
    fill(plo, std::min(phi, lo), pc0, pc1);
    fill(std::max(plo, hi), phi, pc0, pc1);
    const int m0 = std::max(plo, lo), m1 = std::min(phi, hi);  // the rows both rectangles share: the columns beside the new one
    fill(m0, m1, pc0, std::min(pc1, x0));
    fill(m0, m1, std::max(pc0, x1), pc1);
  }
  F.now = {lo, hi, x0, x1};
  return F;
}

inline uint8_t host_quant_u8(float v) {  // quant_u8 of nrf_render.h
  const double s = 255.0 * (double)v;
  if (!(s > 0.0)) return 0;
  if (s >= 255.0) return 255;
  return (uint8_t)s;
}

}  // namespace nrf
