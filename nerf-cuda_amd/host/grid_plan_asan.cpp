// Sanitizer driver of csrc/nrf_grid_plan.h (make grid_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the grid side of
// the plan over (H, cascade, bound, aabb, fill pattern), the rows of tests/test_grid_plan_cpu.py included -- H = 4, 8 and 30, single
// boundary cells, full and empty grids.  The sanitizers watch the index arithmetic (the occupancy's padding word, cc >> 5, the
// dilation's neighbour clamps); the driver itself checks what needs no second implementation.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../csrc/nrf_grid_plan.h"

using namespace nrf;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", what, __LINE__, #cond); ++g_fail; } \
  } while (0)

static uint32_t popcount(const std::vector<uint32_t>& w) {
  uint32_t n = 0;
  for (uint32_t x : w) n += (uint32_t)__builtin_popcount(x);
  return n;
}

int main() {
  const uint32_t Hs[] = {2, 4, 8, 12, 30, 32, 48, 64};
  const struct { uint32_t cascade; float bound; } geo[] = {{1, 1.0f}, {1, 0.75f}, {2, 1.5f}, {2, 4.0f}, {3, 4.0f}, {3, 3.0f}, {5, 16.0f}, {140, 1.0f}};
  const char* fills[] = {"zero", "full", "cell0", "cellH1-x", "cellH1-y", "cellH1-z", "inner", "random", "last-cell"};
  int runs = 0;
  char what[128];
  for (uint32_t H : Hs)
    for (const auto& g : geo)
      for (const char* fill : fills)
        for (int wide_aabb = 0; wide_aabb < 2; ++wide_aabb)
          for (float mean : {0.005f, 0.5f}) {
            if (g.cascade > 5 && H > 8) continue;
            std::snprintf(what, sizeof(what), "H=%u C=%u bound=%g %s aabb=%d mean=%g", H, g.cascade, g.bound, fill, wide_aabb, mean);
            const uint32_t Cs = g.cascade;
            const uint64_t level_cells = (uint64_t)H * H * H, cells = level_cells * Cs;
            std::vector<float> grid(cells, 0.0f);
            auto at = [&](uint32_t c, uint32_t x, uint32_t y, uint32_t z) -> float& { return grid[((c * (uint64_t)H + x) * H + y) * H + z]; };
            const std::string f = fill;
            // ("inner" lies wholly in the unreachable cubes where every cascade's cube is twice the one inside it and a cell is small enough)
            const bool nested = Cs == 1 || g.bound >= ldexpf(1.0f, (int)Cs - 1);  // (else an outer cascade's cells may all be unreachable)
            const bool unreachable_fill = f == "inner" && H >= 16 && nested;
            uint32_t rng = 12345u + H;
            if (f == "full") grid.assign(cells, 1.0f);
            if (f == "cell0") at(0, 0, H / 2, H / 2) = 1.0f;
            if (f == "cellH1-x") at(Cs - 1, H - 1, H / 2, H / 2) = 1.0f;
            if (f == "cellH1-y") at(0, H / 2, H - 1, H / 2) = 1.0f;
            if (f == "cellH1-z") at(0, H / 2, H / 2, H - 1) = 1.0f;
            if (f == "last-cell") grid[cells - 1] = 1.0f;
            if (f == "inner")
              for (uint32_t c = 1; c < Cs; ++c)
                for (uint32_t x = 3 * H / 8; x < 5 * H / 8; ++x) at(c, x, H / 2, H / 2) = 1.0f;
            if (f == "random")
              for (float& v : grid) { rng = rng * 1664525u + 1013904223u; v = (rng >> 28) == 0 ? (float)((rng >> 8) & 0xffff) / 65536.0f * 0.02f : 0.0f; }
            float aabb[6] = {-g.bound, -g.bound, -g.bound, g.bound, g.bound, g.bound};
            if (wide_aabb) { aabb[0] = -1.5f * g.bound; aabb[4] = 1.25f * g.bound; }
            const GridTables T = build_march_tables(H, Cs, g.bound, aabb, grid.data(), mean);
            ++runs;
            uint32_t n_occ = 0;
            for (float v : grid) n_occ += v > fminf(0.01f, mean) ? 1u : 0u;
            CHECK(T.occ.size() == (cells + 31) / 32 + 1 && T.occ.back() == 0u && popcount(T.occ) == n_occ);
            CHECK(T.ctab.size() == (size_t)Cs * (H + 1));
            CHECK(T.coarse_shift == ((H % 4 == 0 && H >= 8) ? 2u : 0u));
            const uint64_t Hc = H / 4;
            if (T.coarse_shift) {
              CHECK(T.coarse.size() == (Cs * Hc * Hc * Hc + 31) / 32 + 1 && T.coarse.back() == 0u);
              CHECK((popcount(T.coarse) == 0) == (n_occ == 0) && popcount(T.coarse) <= n_occ);
              CHECK(f != "full" || popcount(T.coarse) == Cs * Hc * Hc * Hc);
            } else {
              CHECK(T.coarse.empty() && T.dilated.empty() && T.dilated_level_words == 0);
            }
            if (!T.dilated.empty()) {
              CHECK(T.visibility_walk && T.dilated.size() == (size_t)T.dilated_level_words * Cs);
              CHECK(popcount(T.dilated) <= 27u * n_occ && (!unreachable_fill || popcount(T.dilated) == 0));
              CHECK(f != "full" || Cs > 1 || popcount(T.dilated) == Hc * Hc * Hc);
            }
            const bool empty_box = T.occ_box[0] > T.occ_box[3];
            CHECK(n_occ != 0 || empty_box);
            CHECK(f == "inner" ? (!unreachable_fill || empty_box) : (!nested || empty_box == (n_occ == 0)));
            CHECK(empty_box || (T.occ_box[1] <= T.occ_box[4] && T.occ_box[2] <= T.occ_box[5]));
            // the fit beside the hot workgroup (16 waves) and beside a generic one (12 / 8 waves, weights staged or not)
            for (int generic = 0; generic < 2; ++generic)
              for (int flags = 0; flags < 4; ++flags) {
                FitInputs in{};
                in.coarse_words = T.coarse.size(); in.ctab_floats = T.ctab.size(); in.dilated_words = T.dilated.size();
                const FitCandidate hot{0, {16, 0}, {79464u, 0u}, false, true}, gen{1, {12, 8}, {173672u, 116328u}, true, false};
                in.own = generic ? gen : hot;
                in.stage = in.own;
                in.stage_generic = generic != 0;
                in.allow_persistent = (flags & 1) != 0; in.allow_gen_wlds = (flags & 2) != 0;
                in.table_budget = 48u * 1024u; in.strip_fixed_bytes = generic ? 57856u : 35328u; in.weight_area_bytes = 20480u; in.staged_weight_bytes = 28688u;
                const GridFit fit = fit_grid(in);
                CHECK(fit.persistent_lds_bytes <= CU_LDS_BYTES && (fit.persistent != 0) == (fit.persistent_lds_bytes != 0));
                CHECK(!fit.persistent || (in.allow_persistent && fit.lds_coarse_words == T.coarse.size() && fit.lds_dilated_persist == T.dilated.size()));
                CHECK(fit.lds_dilated_strip * 4u <= in.weight_area_bytes && (fit.gen_weights_lds == 0 || (generic && in.allow_gen_wlds)));
                CHECK(fit.rays_persistent == (fit.persistent && !generic));
              }
          }
  std::printf("grid_plan_asan: %d grids, %d failures\n", runs, g_fail);
  return g_fail ? 1 : 0;
}
