// nrf_kernels_rays.hip -- the RAYS instances (nrf_render_rays): frames from caller-supplied rays instead of a pinhole camera
//   render_persistent_kernel<NET_HOT, march, .., RAYS>   the base.json shape whose march tables fit beside the persistent workgroup
//   render_kernel<stage, .., RAYS>                       every other model (stage = NET_HOT, NET_WIDE, NET_GENERIC), and NRF_PERSISTENT=0
// Exact arithmetic only: nrf_options::fast_interp is ignored here, perturb is refused by the entry point.
// The 16 instances and the tests that launch each with a limit that limits (R = tests/test_render_rays_gpu.py, C =
// tests/test_render_rays_clip_gpu.py: a grid of side 32; F = tests/test_render_rays_forms_gpu.py: the rows of tests/rays_forms.py):
//   persistent hot   UNIT, POW2: float planes R C, UNIT 8-bit planes R C, POW2 8-bit planes F (bound4-cascade3);
//                    GENERIC: float planes F (h96, h64-b1.5-c2, h128-b0.75, h48-b3-c3), 8-bit planes F (h64-b1.5-c2)
//   per-strip hot    UNIT, POW2: R C;  GENERIC, tables in LDS: F (the same four rows);  tables in global memory: F (h30, h30-b4-c3)
//   per-strip wide   UNIT: R C;  POW2: F (wide-pow2);  GENERIC, tables in LDS: F (wide-h96);  in global memory: F (wide-h30)
//   per-strip generic   tables in LDS: R C (without a limit), F (sine-h96);  in global memory: F (sine-h30)
// NRF_RAYS_DENSITY_ONLY (FrameParams::ray_flags & RAY_FLAG_DENSITY_ONLY): the two launchers hand the launch to the density-only twins
// of these instances, nrf_kernels_rays_density.hip; nrf_ray_hits (RAY_FLAG_HIT): to the twins of those, nrf_kernels_rays_hit.hip.
// (one family of render-kernel instances per translation unit: nrf_render.h)
#include "nrf_render.h"

namespace nrf {

#define NRF_LAUNCH_PERSISTENT_RAYS(U, O8)                                                                                \
  do {                                                                                                                   \
    constexpr int WV = persist_waves(NET_HOT);                                                                           \
    if (L.waves != WV) return hipErrorInvalidConfiguration; /* the host sized the workgroup's LDS for another instance */ \
    hipError_t e_ = allow_lds(render_persistent_kernel<NET_HOT, U, WV, false, O8, true, GATHER_RUNTIME, false>, L.lds);                  \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_persistent_kernel<NET_HOT, U, WV, false, O8, true, GATHER_RUNTIME, false>), dim3(L.wgs), dim3(64 * WV), L.lds, L.st, \
                       *L.M, *L.P, *L.VB, (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters, L.queue NRF_STEP_ARG(L));   \
  } while (0)
#define NRF_LAUNCH_HOT_RAYS(U)                                                                                           \
  do {                                                                                                                   \
    if (L.P->out_mode == OUT_U8) NRF_LAUNCH_PERSISTENT_RAYS(U, true);                                                    \
    else NRF_LAUNCH_PERSISTENT_RAYS(U, false);                                                                           \
  } while (0)

hipError_t launch_persistent_rays(const PersistLaunch& L) {
  if (L.M->net != NET_HOT || L.P->rays_o == nullptr || L.P->rays_d == nullptr) return hipErrorInvalidConfiguration;
  if (L.P->ray_flags & RAY_FLAG_HIT) return launch_persistent_rays_hit(L);
  if (L.P->ray_flags & RAY_FLAG_DENSITY_ONLY) return launch_persistent_rays_density(L);
  if (L.unit) NRF_LAUNCH_HOT_RAYS(MARCH_UNIT);
  else if (L.pow2) NRF_LAUNCH_HOT_RAYS(MARCH_POW2);
  else NRF_LAUNCH_HOT_RAYS(MARCH_GENERIC);
  return hipGetLastError();
}

#define NRF_LAUNCH_RENDER_RAYS(G, C, U)                                                                                  \
  do {                                                                                                                   \
    hipError_t e_ = allow_lds(render_kernel<G, C, U, false, true>, L.lds);                                               \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_kernel<G, C, U, false, true>), dim3(L.blocks), dim3(RENDER_THREADS), L.lds, L.st, *L.M, *L.P, *L.VB, \
                       (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters);                               \
  } while (0)

hipError_t launch_strip_rays(const StripLaunch& L) {
  if (L.perturb || L.P->rays_o == nullptr || L.P->rays_d == nullptr) return hipErrorInvalidConfiguration;
  if (L.P->ray_flags & RAY_FLAG_HIT) return launch_strip_rays_hit(L);
  if (L.P->ray_flags & RAY_FLAG_DENSITY_ONLY) return launch_strip_rays_density(L);
  if (L.M->stage == NET_GENERIC) {
    if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS(NET_GENERIC, true, MARCH_GENERIC); else NRF_LAUNCH_RENDER_RAYS(NET_GENERIC, false, MARCH_GENERIC);
  } else if (L.M->stage == NET_WIDE) {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS(NET_WIDE, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS(NET_WIDE, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS(NET_WIDE, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS(NET_WIDE, false, MARCH_GENERIC);
  } else {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS(NET_HOT, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS(NET_HOT, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS(NET_HOT, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS(NET_HOT, false, MARCH_GENERIC);
  }
  return hipGetLastError();
}

// the HIP runtime loads a translation unit's code object at the first launch of one of its kernels: touch one here, so that
// nrf_load_model pays for it (once per process and device) and not the first frame (preload_kernels, nrf_kernels.hip)
void preload_rays() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&render_persistent_kernel<NET_HOT, MARCH_UNIT, persist_waves(NET_HOT), false, false, true, GATHER_RUNTIME, false>));
}

}  // namespace nrf
