// nrf_stage_plan.h -- the launch geometry of the stage kernels and the pixel-format kernels (nrf_kernels.hip), in one place.
//
// Every one of these kernels walks its rows in a grid-stride loop under a capped grid: a call with more rows than one pass of that
// grid makes the workers go round again.  Per kernel kind this header holds the block size, the work items one workgroup consumes
// per trip and the workgroup cap; the launchers take their grids from stage_workgroups, and the tests take "one pass" from
// stage_items_per_pass (host/stage_plan_check.cpp prints both), so that a test which means to make second trips still makes them
// after a cap has changed.  Plain C++: no device code, no HIP header.
#pragma once
#include <cstdint>

namespace nrf {

enum StageKernel : int {
  STAGE_MLP_FORWARD = 0,  // mlp_forward_kernel<REPEAT, OCC, NAMED>; arg = the form (30, 20, 21: launch_mlp_forward)
  STAGE_GEN_MLP_FORWARD,  // gen_mlp_forward_kernel
  STAGE_ENCODE_GRID,      // encode_grid_kernel<FAST>: 16 levels
  STAGE_GEN_ENCODE_GRID,  // gen_encode_grid_kernel; arg = n_levels
  STAGE_ENCODE_DIR,       // encode_dir_kernel
  STAGE_GEN_ENCODE_DIR,   // gen_encode_dir_kernel
  STAGE_NETWORK,          // network_kernel<NET>
  STAGE_GENERATE_RAYS,    // generate_rays_kernel: rows = pixels
  STAGE_MARCH,            // march_kernel<COARSE>: rows = rays
  STAGE_COMPOSITE,        // composite_kernel: rows = rays
  STAGE_QUANTIZE,         // quantize_kernel: rows = pixels
  STAGE_QUANTIZE_RGBD8,   // quantize_rgbd8_kernel: rows = pixels
  STAGE_UNTILE,           // untile_kernel: rows = pixels of every view
  STAGE_UNTILE_U8,        // untile_rgbd8_u8_kernel: rows = quads of 4 pixels (widths that are multiples of 4), else pixels
  STAGE_KERNEL_COUNT
};

struct StageKind {
  int kernel;   // StageKernel
  int arg = 0;  // STAGE_MLP_FORWARD: the form; STAGE_GEN_ENCODE_GRID: n_levels; else unused
};

constexpr int STAGE_MLP_ROWS = 32;      // rows of a wave's chunk in mlp_forward_kernel (16 * MLP_TILES)
constexpr int STAGE_GEN_MLP_ROWS = 32;  // ... in gen_mlp_forward_kernel (GEN_SAMPLES)
constexpr int STAGE_NETWORK_ROWS = 64;  // ... in network_kernel

struct StagePlan {
  int block;            // threads of a workgroup
  int wg_items;         // work items a workgroup consumes per trip
  int cap;              // workgroups at the most
  uint32_t row_items;   // work items per row of the call (a (sample, level) pair is an item of the grid encodings)
  int worker_items;     // work items one worker -- a wave, or a lane of the one-lane-per-item kernels -- consumes per trip
};

// workgroups per compute unit a form of mlp_forward_kernel is budgeted for: 3 (form 30), 2 (forms 20, 21)
constexpr int stage_mlp_occ(int form) { return form == 20 || form == 21 ? 2 : 3; }

inline StagePlan stage_plan(StageKind k) {
  switch (k.kernel) {
    case STAGE_MLP_FORWARD: return {256, 4 * STAGE_MLP_ROWS, 256 * stage_mlp_occ(k.arg), 1u, STAGE_MLP_ROWS};
    case STAGE_GEN_MLP_FORWARD: return {256, 4 * STAGE_GEN_MLP_ROWS, 256 * 4, 1u, STAGE_GEN_MLP_ROWS};
    case STAGE_NETWORK: return {256, 4 * STAGE_NETWORK_ROWS, 256 * 4, 1u, STAGE_NETWORK_ROWS};
    case STAGE_ENCODE_GRID: return {256, 256, 256 * 8, 16u, 1};
    case STAGE_GEN_ENCODE_GRID: return {256, 256, 256 * 8, k.arg > 0 ? (uint32_t)k.arg : 1u, 1};
    default: return {256, 256, 256 * 8, 1u, 1};  // one lane per row
  }
}

// the grid of a call with n rows: ceil(n * row_items / wg_items) workgroups, at least one, at most the cap
inline int stage_workgroups(StageKind k, uint64_t n) {
  const StagePlan p = stage_plan(k);
  const uint64_t work = n * p.row_items;
  uint64_t g = work / (uint64_t)p.wg_items + (work % (uint64_t)p.wg_items ? 1u : 0u);
  if (g < 1) g = 1;
  if (g > (uint64_t)p.cap) g = (uint64_t)p.cap;
  return (int)g;
}

// the most rows the capped grid consumes in one pass: a call with one row more sends a worker round its loop again
inline uint64_t stage_items_per_pass(StageKind k) {
  const StagePlan p = stage_plan(k);
  return (uint64_t)p.cap * (uint64_t)p.wg_items / p.row_items;
}

// trips of the first and of the last worker of the grid through the loop, for n rows
struct StageTrips {
  uint64_t first, last;
};
inline StageTrips stage_trips(StageKind k, uint64_t n) {
  const StagePlan p = stage_plan(k);
  const uint64_t work = n * p.row_items;
  const uint64_t units = work / (uint64_t)p.worker_items + (work % (uint64_t)p.worker_items ? 1u : 0u);
  const uint64_t workers = (uint64_t)stage_workgroups(k, n) * (uint64_t)(p.wg_items / p.worker_items);
  StageTrips t;
  t.first = (units + workers - 1) / workers;  // worker 0 takes the units 0, workers, 2 workers, ...
  t.last = units / workers;                   // worker workers - 1 takes workers - 1, 2 workers - 1, ...
  return t;
}

}  // namespace nrf
