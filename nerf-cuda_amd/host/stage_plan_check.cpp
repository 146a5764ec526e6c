// Sanitizer driver of csrc/nrf_stage_plan.h (make stage_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the launch
// geometry of the stage kernels and the pixel-format kernels, compiled from the text the launchers compile.  On stdin, pairs of
//     kind n
// kind: a kernel's name, with ":arg" where the geometry depends on one -- mlp_forward:30 | :20 | :21 (the form), gen_encode_grid:L
// (n_levels) --, n: the rows of the call (decimal, up to 2^64 - 1 / 16).  On stdout, one line per pair:
//     kind n workgroups block items_per_wg cap items_per_row items_per_pass trips_first trips_last
// items_per_wg and cap are in work items (a (sample, level) pair of the grid encodings; else a row), items_per_row of them make a row;
// items_per_pass is the most rows one pass of the capped grid consumes; trips_* are the trips of the grid's first and last worker (a
// wave of the MLP and network kernels, a lane of the others) through its loop.  tests/stage_plan_rows.py runs it; tests/test_stage_plan_cpu.py
// holds the rows to the closed form, and the GPU tests take every "one pass" from here.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/nrf_stage_plan.h"

static const char* const NAMES[nrf::STAGE_KERNEL_COUNT] = {
    "mlp_forward", "gen_mlp_forward", "encode_grid", "gen_encode_grid", "encode_dir", "gen_encode_dir",  "network",
    "generate_rays", "march",         "composite",   "quantize",        "quantize_rgbd8", "untile",      "untile_u8"};

static bool parse_kind(const char* text, nrf::StageKind& k) {
  const char* colon = std::strchr(text, ':');
  const size_t len = colon ? (size_t)(colon - text) : std::strlen(text);
  k.kernel = -1;
  for (int i = 0; i < nrf::STAGE_KERNEL_COUNT; ++i)
    if (std::strlen(NAMES[i]) == len && std::strncmp(NAMES[i], text, len) == 0) k.kernel = i;
  if (k.kernel < 0) return false;
  const bool takes_arg = k.kernel == nrf::STAGE_MLP_FORWARD || k.kernel == nrf::STAGE_GEN_ENCODE_GRID;
  if (takes_arg != (colon != nullptr)) return false;
  k.arg = 0;
  if (colon) {
    char* end = nullptr;
    const long v = std::strtol(colon + 1, &end, 10);
    if (end == colon + 1 || *end != '\0' || v < 1 || v > 64) return false;
    if (k.kernel == nrf::STAGE_MLP_FORWARD && v != 30 && v != 20 && v != 21) return false;
    k.arg = (int)v;
  }
  return true;
}

int main() {
  char kind[64];
  uint64_t n;
  int rows = 0;
  while (std::scanf("%63s %" SCNu64, kind, &n) == 2) {
    nrf::StageKind k{0, 0};
    if (!parse_kind(kind, k)) {
      std::fprintf(stderr, "stage_plan_check: unknown kind %s\n", kind);
      return 2;
    }
    if (n > UINT64_MAX / 64) {
      std::fprintf(stderr, "stage_plan_check: n out of range\n");
      return 2;
    }
    const nrf::StagePlan p = nrf::stage_plan(k);
    const nrf::StageTrips t = nrf::stage_trips(k, n);
    std::printf("%s %" PRIu64 " %d %d %d %d %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", kind, n, nrf::stage_workgroups(k, n), p.block, p.wg_items,
                p.cap, p.row_items, nrf::stage_items_per_pass(k), t.first, t.last);
    ++rows;
  }
  std::fprintf(stderr, "stage_plan_check: %d rows\n", rows);
  return 0;
}
