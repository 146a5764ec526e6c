// Sanitizer driver of csrc/nrf_frame_plan.h (make frame_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the frame plan
// over frame sizes from 1x1 to 8K (multiples of 8 and 32 and not), 1 .. 9 shards (more shards than strips included), regions of
// interest that are empty, inverted, partly negative or beyond the frame, 1 .. 128 views and random rectangles for the fill.  The
// sanitizers watch the arithmetic; the driver checks that every extent and rectangle the plan returns stays inside the planes.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../csrc/nrf_frame_plan.h"

using namespace nrf;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", what, __LINE__, #cond); ++g_fail; } \
  } while (0)

int main() {
  const int sizes[][2] = {{1, 1}, {7, 3}, {8, 8}, {9, 9}, {20, 12}, {31, 33}, {32, 32}, {36, 20}, {101, 77}, {333, 211}, {640, 360},
                          {1920, 1080}, {1921, 1079}, {7680, 4320}};
  const int view_counts[] = {1, 2, 3, 16, 127, 128};
  std::mt19937 rng(1234);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  char what[160];
  long runs = 0;
  for (const auto& sz : sizes) {
    const int W = sz[0], H = sz[1], tx = tiles_of(W), ty = tiles_of(H), total = total_strips(W, H);
    const size_t px = (size_t)W * H;
    std::snprintf(what, sizeof(what), "%dx%d", W, H);
    CHECK(views_per_launch(tx, ty, 128) >= 1 && views_per_launch(tx, ty, 128) <= 128);
    CHECK((long long)views_per_launch(tx, ty, 128) * ty * strips_per_row(tx) < QUEUE_POS_LIMIT);
    // regions: the whole frame, none, inverted, partly negative, beyond the frame, and random ones around it
    std::vector<int> rois = {0, 0, W - 1, H - 1, 0, 0, -1, -1, W - 1, H - 1, 0, 0, -5, -17, W / 2, H / 2, W / 2, H / 2, W + 40, H + 40,
                             W + 8, H + 8, W + 30, H + 30, -90, -90, -20, -20, 0, 8 * (ty - 1), W - 1, H - 1};
    for (int i = 0; i < 120; ++i) {
      const int x0 = rnd(-20, W + 20), y0 = rnd(-20, H + 20);
      rois.insert(rois.end(), {x0, y0, rnd(x0 - 3, W + 20), rnd(y0 - 3, H + 20)});
    }
    const int n_rois = (int)rois.size() / 4;
    std::vector<int> rows((size_t)4 * n_rois);
    for (int r = 0; r < n_rois; ++r) {
      const int* roi = &rois[4 * (size_t)r];
      int* ro = &rows[4 * (size_t)r];
      roi_rows(roi, H, ro[0], ro[1]);
      roi_cols(roi, W, ro[2], ro[3]);
      CHECK(0 <= ro[0] && ro[0] <= ro[1] && ro[1] <= H && 0 <= ro[2] && ro[2] <= ro[3] && ro[3] <= W);
      const StripRows s = roi_strip_rows(roi, ty);
      CHECK(s.ty1 < s.ty0 || (0 <= s.ty0 && s.ty1 < ty));
      // the copies of the view, as each of the slot's views, whole rows and columns
      for (int views : {1, 3})
        for (int v = 0; v < views; ++v)
          for (int cols = 0; cols < 2 && ro[1] > ro[0]; ++cols) {
            const RowCopy k = row_copy(W, px, (size_t)views, v, ro[0], ro[1], cols ? ro[2] : 0, cols ? ro[3] : 0);
            const size_t rgb_end = k.rgb.off + k.rgb.pitch * (k.rgb.rows - 1) + k.rgb.width;
            const size_t depth_end = k.depth.off + k.depth.pitch * (k.depth.rows - 1) + k.depth.width;
            CHECK(k.rgb.rows >= 1 && k.rgb.off >= (size_t)v * px * 3 && rgb_end <= (size_t)(v + 1) * px * 3);
            CHECK(k.depth.off >= (size_t)views * px * 3 + (size_t)v * px && depth_end <= (size_t)views * px * 3 + (size_t)(v + 1) * px);
            CHECK(k.rgb.bytes() == 3 * k.depth.bytes() && k.rgb.width <= k.rgb.pitch);
          }
      // the fill against random previous rectangles
      for (int i = 0; i < 8; ++i) {
        const int r0 = rnd(0, H), c0 = rnd(0, W);
        const Rect prev{r0, rnd(r0, H), c0, rnd(c0, W)};
        const FillPlan F = fill_rects(prev, i == 0, W, H, ro, (i & 1) != 0);
        CHECK(F.n >= 0 && F.n <= 4 && F.now.r0 == ro[0] && F.now.r1 == ro[1] && 0 <= F.now.c0 && F.now.c0 < F.now.c1 && F.now.c1 <= W);
        for (int j = 0; j < F.n; ++j) {
          const Rect& q = F.rects[j];
          CHECK(0 <= q.r0 && q.r0 < q.r1 && q.r1 <= H && 0 <= q.c0 && q.c0 < q.c1 && q.c1 <= W);
          const bool beside = q.r1 <= F.now.r0 || q.r0 >= F.now.r1 || q.c1 <= F.now.c0 || q.c0 >= F.now.c1 || F.now.r1 <= F.now.r0;
          CHECK(beside);  // nothing is filled where this call's copies write
        }
        ++runs;
      }
    }
    for (int N = 1; N <= 9; ++N) {
      long sum = 0;
      for (int idx = 0; idx < N; ++idx) {
        const int n_local = local_tiles(W, H, idx, N);
        CHECK(n_local >= 0 && n_local % 4 == 0 && n_local <= tiles_per_shard(W, H, N));
        sum += n_local;
        for (int n_views : view_counts) {
          if (px > 2000000 && n_views != 1 && n_views != 128) continue;
          std::snprintf(what, sizeof(what), "%dx%d shard %d of %d, %d views", W, H, idx, N, n_views);
          std::vector<int> vr((size_t)4 * n_views);
          std::vector<int> vrows((size_t)4 * n_views);
          for (int v = 0; v < n_views; ++v) {
            const int r = (v * 7 + idx + N) % n_rois;
            std::copy(&rois[4 * (size_t)r], &rois[4 * (size_t)r] + 4, &vr[4 * (size_t)v]);
            std::copy(&rows[4 * (size_t)r], &rows[4 * (size_t)r] + 4, &vrows[4 * (size_t)v]);
          }
          std::vector<ViewQueue> vq((size_t)n_views);
          for (int classes : {0, 1, 8, 9}) {
            const QueuePlan Q = plan_queues({tx, ty, idx, N, n_local, classes, 256, 16, 4}, n_views, vr.data(), vq.data());
            int q = 0;
            for (const ViewQueue& V : vq) {
              CHECK(0 <= V.k_lo && V.k_lo <= V.k_hi && V.k_hi <= ((n_local + 3) & ~3));
              CHECK(V.q_begin == q && V.q_rows >= 0 && V.q_row0 >= 0 && V.q_row0 + V.q_rows <= ty);
              q += V.q_rows;
            }
            CHECK(Q.q_total == q && Q.n_classes >= 1 && Q.n_classes <= 8 && Q.class_cols >= 1 && Q.workgroups >= 1 && Q.workgroups <= 256);
            CHECK(Q.refused == (Q.n_pos >= QUEUE_POS_LIMIT) && Q.blocks_per_view * 4 >= n_local);
            (void)launch_is_planned(true, Q.n_pos, 1 << 14, 2048);
            ++runs;
          }
          (void)drops_sample_cap(n_local, n_views, 256, 16, false);
          (void)host_frame_progressive(true, n_views, W, ty, 1 << 14);
          for (int depth = 0; depth < 2 && N == 1; ++depth) {
            const std::vector<Band> bands = plan_bands(W, depth != 0, n_views, vrows.data());
            for (const Band& b : bands) {
              CHECK(0 <= b.view && b.view < n_views && vrows[4 * (size_t)b.view] <= b.lo && b.lo < b.hi && b.hi <= vrows[4 * (size_t)b.view + 1]);
              CHECK(b.s0 == b.lo / 8 && b.s1 == (b.hi + 7) / 8 && b.s1 <= ty);
            }
          }
        }
      }
      std::snprintf(what, sizeof(what), "%dx%d, %d shards", W, H, N);
      CHECK(sum == 4L * total);
    }
  }
  // regions from cameras: finite, NaN and singular poses, boxes in front, around and behind
  {
    std::uniform_real_distribution<float> u(-3.0f, 3.0f);
    std::snprintf(what, sizeof(what), "view_roi");
    for (int i = 0; i < 20000; ++i) {
      float R[9], org[3], cam[4] = {500.0f + 100.0f * u(rng), 500.0f, 320.0f + 100.0f * u(rng), 180.0f};
      for (float& r : R) r = u(rng);
      for (float& o : org) o = (i % 5 == 0 ? 3000.0f : 1.0f) * u(rng);
      if (i % 7 == 0) R[i % 9] = NAN;
      if (i % 11 == 0) org[i % 3] = INFINITY;
      if (i % 13 == 0) for (int k = 0; k < 3; ++k) R[3 + k] = R[k];
      const float box[6] = {-0.5f, -0.5f, -0.4f, i % 17 == 0 ? -1.0f : 0.6f, 0.4f, 0.4f};
      int roi[4];
      view_roi(R, org, cam, box, 640, 360, roi);
      far_camera_roi(org, 4096.0f, roi);
      CHECK(0 <= roi[0] && roi[0] <= 640 && 0 <= roi[1] && roi[1] <= 360 && -1 <= roi[2] && roi[2] <= 639 && -1 <= roi[3] && roi[3] <= 359);
      ++runs;
    }
    for (float v : {-1.0f, 0.0f, 0.25f, 1.0f, 2.0f, NAN, INFINITY, -INFINITY}) (void)host_quant_u8(v);
  }
  std::printf("frame_plan_asan: %ld runs, %d failed\n", runs, g_fail);
  return g_fail ? 1 : 0;
}
