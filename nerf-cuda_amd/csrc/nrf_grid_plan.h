// nrf_grid_plan.h -- the grid side of the host's plan, without a device (plain C++17: a host compiler builds it alone).
// build_march_tables makes everything the march needs from a float density grid; fit_grid decides which of those tables are
// staged in LDS and which workgroup renders the frames beside them.  nrf_api.hip's set_density_grid uploads the result;
// nrf_debug_grid_plan returns it (tests/test_grid_plan_cpu.py), host/grid_plan_asan.cpp runs it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace nrf {

constexpr uint32_t CU_LDS_BYTES = 160u * 1024u;  // LDS of a compute unit: what one workgroup may ask for

// log2 of the side of the coarse occupancy blocks (4 x 4 x 4 cells per bit), 0 where the grid has none: a side that is no multiple
// of 4.  Without the coarse level no march table is staged in LDS (fit_grid) and the model renders in the per-strip
// kernel, whatever its gather plan: the static-plan instances are the persistent kernel's (nrf_debug_march_form)
inline uint32_t march_coarse_shift(uint32_t H) { return (H % 4 == 0 && H >= 8) ? 2u : 0u; }

// half the side of cascade `level`'s cube: min(2^level, bound), 1 in a single-cascade model (render_utils.h:603-607)
inline float mip_bound_of(uint32_t cascade, uint32_t level, float bound) { return fminf(cascade > 1 ? ldexpf(1.0f, (int)level) : 1.0f, bound); }
inline double mip_bound_of_d(uint32_t cascade, uint32_t level, float bound) { return fmin(cascade > 1 ? ldexp(1.0, (int)level) : 1.0, (double)bound); }

// cell r of one cascade level (index level * H^3 + x * H^2 + y * H + z, nerf_render.h:64-65) -> (x, y, z)
inline void decode_cell(uint64_t r, uint64_t H, uint32_t n3[3]) {
  n3[0] = (uint32_t)(r / (H * H));
  n3[1] = (uint32_t)((r / H) % H);
  n3[2] = (uint32_t)(r % H);
}

// A density cell of cascade k >= 1 is only ever looked up for positions of level k, i.e. with
// max|p| >= 2^(k-1) (kernel_march_rays picks the level from frexp(max|p|), render_utils.h:603-607): cells
// that lie, with one cell of slack, wholly inside the inner cube max|p| < 2^(k-1) cannot produce a sample
// whatever their value, so they count neither for the box of occupied cells nor for the visibility sets.
inline bool reachable(uint32_t Hs, uint32_t Cs, float bound, uint32_t level, const uint32_t n3[3]) {
  if (level == 0 || Cs <= 1) return true;
  const double mb = mip_bound_of_d(Cs, level, bound), cell = 2.0 * mb / (double)Hs;
  double r_max = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double lo = -mb + n3[a] * cell, hi = lo + cell;
    r_max = fmax(r_max, fmax(fabs(lo), fabs(hi)));
  }
  return !(r_max + cell < ldexp(1.0, (int)level - 1));
}

// Everything the march needs from the density grid (reference: the float grid [C*H^3] of load_snapshot,
// nerf_render.cu:441-466, read by kernel_march_rays): occupancy bits, coarse occupancy, the box of occupied cells,
// the dilated coarse sets of the visibility walk and the cell-boundary table.
struct GridTables {
  std::vector<uint32_t> occ;      // 1 bit per cell (+ a padding word)
  std::vector<uint32_t> coarse;   // OR over 4x4x4 cell blocks (+ a padding word); empty without a coarse level
  std::vector<uint32_t> dilated;  // [C][dilated_level_words]; empty without a coarse level or without the visibility walk
  std::vector<float> ctab;        // [C][H + 1]
  float occ_box[6] = {1.f, 1.f, 1.f, -1.f, -1.f, -1.f};  // empty
  uint32_t coarse_shift = 0;
  uint32_t dilated_level_words = 0;  // words per cascade level (whole words, so a level's bits start at bit 0)
  bool visibility_walk = true;
};

inline GridTables build_march_tables(uint32_t Hs, uint32_t Cs, float bound, const float aabb[6], const float* density_grid, float mean_density) {
  GridTables T;
  const uint64_t Hh = Hs, level_cells = Hh * Hh * Hh, cells = level_cells * Cs;
  auto occupied = [&](uint64_t i) { return ((T.occ[i >> 5] >> (i & 31)) & 1u) != 0; };
  // occupancy bitfield: grid[cell] > min(0.01, mean_density) (render_utils.h:560,619), decided once
  const float thresh = fminf(0.01f, mean_density);
  T.occ.assign((cells + 31) / 32 + 1, 0u);
  for (uint64_t i = 0; i < cells; ++i)
    if (density_grid[i] > thresh) T.occ[i >> 5] |= 1u << (i & 31);

  // march tables (nrf_device.h march_next): coarse occupancy = OR over 4x4x4 cell blocks, and the
  // cell-boundary table ((v/(H-1))*2-1)*mip_bound in the reference's fp32 operation order
  T.coarse_shift = march_coarse_shift(Hs);
  if (T.coarse_shift) {
    const uint32_t Hc = Hs >> 2;
    T.coarse.assign(((uint64_t)Cs * Hc * Hc * Hc + 31) / 32 + 1, 0u);
    for (uint64_t i = 0; i < cells; ++i) {
      if (!occupied(i)) continue;
      const uint32_t level = (uint32_t)(i / level_cells);
      uint32_t n3[3];
      decode_cell(i % level_cells, Hh, n3);
      const uint64_t cc = (((uint64_t)level * Hc + (n3[0] >> 2)) * Hc + (n3[1] >> 2)) * Hc + (n3[2] >> 2);
      T.coarse[cc >> 5] |= 1u << (cc & 31);
    }
  }
  // world-space box around every occupied (and reachable) cell, inflated by 2 cells of its cascade level
  bool boundary_occupied = false;  // an occupied (reachable) cell with index 0 or H-1 on some axis
  bool any = false;
  for (uint32_t level = 0; level < Cs; ++level) {
    uint32_t lo[3] = {Hs, Hs, Hs}, hi[3] = {0, 0, 0};
    bool lvl_any = false;
    for (uint64_t r = 0; r < level_cells; ++r) {
      if (!occupied((uint64_t)level * level_cells + r)) continue;
      uint32_t n3[3];
      decode_cell(r, Hh, n3);
      if (!reachable(Hs, Cs, bound, level, n3)) continue;
      for (int a = 0; a < 3; ++a) { lo[a] = n3[a] < lo[a] ? n3[a] : lo[a]; hi[a] = n3[a] > hi[a] ? n3[a] : hi[a]; }
      lvl_any = true;
    }
    if (!lvl_any) continue;
    const double mip_bound = mip_bound_of_d(Cs, level, bound);
    const double cell = 2.0 * mip_bound / (double)Hs;
    for (int a = 0; a < 3; ++a) {
      float wlo = (float)(-mip_bound + ((double)lo[a] - 2.0) * cell);
      float whi = (float)(-mip_bound + ((double)hi[a] + 3.0) * cell);
      // The march clamps the position to +-bound and then the cell index to [0, H-1] (render_utils.h:595-611):
      // a position OUTSIDE this cascade's cube -- bound > 2^(C-1), or an aabb wider than +-bound -- lands in the
      // boundary layer of cells.  An occupied boundary cell therefore stands for everything beyond that face: the
      // box is extended to wherever a ray can be (its aabb range) on that side.
      if (lo[a] == 0) wlo = fminf(wlo, fminf(aabb[a], -bound) - (float)(2.0 * cell));
      if (hi[a] == Hs - 1) whi = fmaxf(whi, fmaxf(aabb[a + 3], bound) + (float)(2.0 * cell));
      if (!any || wlo < T.occ_box[a]) T.occ_box[a] = wlo;
      if (!any || whi > T.occ_box[a + 3]) T.occ_box[a + 3] = whi;
      boundary_occupied = boundary_occupied || lo[a] == 0 || hi[a] == Hs - 1;
    }
    any = true;
  }
  // Positions outside the outermost cube exist when bound > its mip_bound or the aabb is wider than +-bound.  The
  // per-cascade visibility walk (coarse_visibility) only covers a ray's stretch INSIDE each cube, so with an
  // occupied boundary layer in such a model it would miss those samples: the walk is switched off then (the box
  // test above stays exact).
  bool exterior_positions = bound > mip_bound_of(Cs, Cs - 1, bound);
  for (int a = 0; a < 3; ++a) exterior_positions = exterior_positions || aabb[a] < -bound || aabb[a + 3] > bound;
  T.visibility_walk = !(exterior_positions && boundary_occupied);
  // Conservative coarse visibility set (single cascade): coarse cells that contain, or lie within one
  // density cell of, an occupied density cell (= the coarse image of the occupancy dilated by one
  // fine cell); used by the per-ray DDA of render_kernel (nrf_device.h coarse_visibility).
  if (T.coarse_shift && T.visibility_walk) {
    const int Hc = (int)(Hs >> 2), Hf = (int)Hs;
    T.dilated_level_words = (uint32_t)(((uint64_t)Hc * Hc * Hc + 31) / 32);
    T.dilated.assign((size_t)T.dilated_level_words * Cs, 0u);
    for (uint32_t level = 0; level < Cs; ++level) {
      uint32_t* dl = T.dilated.data() + (size_t)level * T.dilated_level_words;
      for (uint64_t r = 0; r < level_cells; ++r) {
        if (!occupied((uint64_t)level * level_cells + r)) continue;
        uint32_t n3[3];
        decode_cell(r, Hh, n3);
        if (!reachable(Hs, Cs, bound, level, n3)) continue;
        const int x = (int)n3[0], y = (int)n3[1], z = (int)n3[2];
        for (int dx = -1; dx <= 1; ++dx)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
              const int X = x + dx, Y = y + dy, Z = z + dz;
              if (X < 0 || Y < 0 || Z < 0 || X >= Hf || Y >= Hf || Z >= Hf) continue;
              const uint64_t nn = ((uint64_t)(X >> 2) * Hc + (Y >> 2)) * Hc + (Z >> 2);
              dl[nn >> 5] |= 1u << (nn & 31);
            }
      }
    }
  }
  T.ctab.resize((size_t)Cs * (Hs + 1));
  for (uint32_t level = 0; level < Cs; ++level) {
    const float mip_bound = mip_bound_of(Cs, level, bound);
    const float Hm1 = (float)(Hs - 1);
    for (uint32_t v = 0; v <= Hs; ++v) T.ctab[(size_t)level * (Hs + 1) + v] = ((float)v / Hm1 * 2 - 1) * mip_bound;
  }
  return T;
}

// A persistent workgroup fit_grid may choose: instance `net` with waves[0] waves, or (waves[1] != 0: the generic instance) with
// waves[1]; lds_bytes: that workgroup's LDS without march tables and staged weights (nrf_launch.h render_persistent_lds_bytes)
struct FitCandidate {
  int net;
  int waves[2];
  uint32_t lds_bytes[2];
  bool stages_weights;  // the generic instance: its weight fragments may be staged in LDS beside rows and tables
  bool rays;            // the instance has a persistent RAYS form (the hot shape only)
};
struct FitInputs {
  uint64_t coarse_words, ctab_floats, dilated_words;  // table sizes (coarse_words: 0 without a coarse level)
  FitCandidate own, stage;    // the model's own instance (plan_model) and its stage instance, in the order they are tried
  bool stage_generic, stage_wide;
  bool allow_persistent, allow_gen_wlds;  // NRF_PERSISTENT / NRF_GEN_WLDS
  // LDS figures that depend on device-side struct sizes (nrf_launch.h)
  uint32_t table_budget;         // render_lds_table_max_bytes
  uint32_t strip_fixed_bytes;    // render_strip_lds_fixed_bytes of the stage instance: the per-strip workgroup without tables
  uint32_t weight_area_bytes;    // render_weight_area_bytes: what the per-strip kernel lends the dilated table during ray setup
  uint32_t staged_weight_bytes;  // render_staged_weight_bytes: the generic instance's fragments in LDS
};
struct GridFit {
  uint32_t lds_coarse_words = 0, lds_ctab_floats = 0;  // 0: the tables stay in global memory
  uint32_t lds_dilated_strip = 0;    // words of the dilated table the per-strip kernel stages (it borrows the weight area)
  uint32_t lds_dilated_persist = 0;  // ... and the persistent kernel (all of it, or the model has no persistent form)
  int net = 0;                       // the instance that renders the frames
  uint32_t persistent = 0, persist_waves = 0, gen_weights_lds = 0;
  bool rays_persistent = false;      // nrf_render_rays runs the persistent RAYS instance
  uint32_t persistent_lds_bytes = 0; // LDS of the persistent launch (0 without one)
};

// LDS of a persistent launch: ONE sum, made by fit_grid when it chooses the workgroup and by launch_render when it launches it
inline uint32_t persistent_lds_total(uint32_t workgroup_bytes, uint64_t table_words, uint32_t staged_weight_bytes) {
  return (uint32_t)(workgroup_bytes + 4 * table_words + staged_weight_bytes);
}

inline GridFit fit_grid(const FitInputs& in) {
  GridFit f;
  uint64_t budget = in.table_budget;
  if (in.stage_generic)  // whatever the generic instance's rows leave of the CU's LDS
    budget = in.strip_fixed_bytes + budget <= CU_LDS_BYTES ? budget : CU_LDS_BYTES - in.strip_fixed_bytes;
  if (in.stage_wide) {  // three workgroups per CU: (a third of its LDS - fixed part) for the tables
    const uint64_t room = CU_LDS_BYTES / 3u - (uint64_t)in.strip_fixed_bytes;
    budget = budget < room ? budget : room;
  }
  if (in.coarse_words && 4 * (in.coarse_words + in.ctab_floats) <= budget) {
    f.lds_coarse_words = (uint32_t)in.coarse_words;
    f.lds_ctab_floats = (uint32_t)in.ctab_floats;
  }
  if (in.dilated_words && in.dilated_words * 4 <= in.weight_area_bytes) f.lds_dilated_strip = (uint32_t)in.dilated_words;
  // The persistent form of the render kernel (one workgroup per CU, waves pull strips from work queues) keeps every march
  // table in LDS for the whole launch: tables that fit beside the blocks of its waves.  The model's own instance if they fit
  // beside its workgroup (a register-resident instance other than the stage one has the persistent form only), else the
  // stage instance -- the generic one with 12 waves and its weight fragments in LDS, 12 without, 8 with, 8 without: the first
  // that fits (NRF_GEN_WLDS=0 at nrf_create: never stage the fragments).  Decided again for every grid (nrf_generate_density_grid).
  f.net = in.stage.net;
  if (in.allow_persistent && f.lds_coarse_words > 0) {
    const uint64_t tables = (uint64_t)f.lds_coarse_words + f.lds_ctab_floats + in.dilated_words;
    for (const FitCandidate* cand : {&in.own, &in.stage}) {
      for (int s = 0; s < 2 && cand->waves[s] != 0 && !f.persistent; ++s) {  // (only the generic instance has a second size)
        for (int wlds : {1, 0}) {
          if (wlds && (!cand->stages_weights || !in.allow_gen_wlds)) continue;
          const uint32_t total = persistent_lds_total(cand->lds_bytes[s], tables, wlds ? in.staged_weight_bytes : 0u);
          if (total <= CU_LDS_BYTES) {
            f.net = cand->net;
            f.persistent = 1;
            f.persist_waves = (uint32_t)cand->waves[s];
            f.gen_weights_lds = (uint32_t)wlds;
            f.lds_dilated_persist = (uint32_t)in.dilated_words;
            f.persistent_lds_bytes = total;
            // caller-supplied rays (nrf_render_rays): the persistent RAYS instance is the hot shape's; every other model -- and a hot
            // one whose tables do not fit -- renders rays in the per-strip RAYS instance of its stage (nrf_kernels_rays.hip)
            f.rays_persistent = cand->rays;
            break;
          }
        }
      }
      if (f.persistent) break;
    }
  }
  return f;
}

}  // namespace nrf
