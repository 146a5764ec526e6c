// nrf_kernels_rays_hit.hip -- the RAYS_HIT twins of the density-only RAYS instances (nrf_ray_hits): where a caller's ray reaches an
// opacity threshold -- picking, collision and placement, range sensors, the origins of shadow rays.
//   render_persistent_kernel<NET_HOT, march, .., RAYS_HIT, ..>   the base.json shape whose march tables fit beside the persistent workgroup
//   render_kernel<stage, .., RAYS_HIT>                           every other model (stage = NET_HOT, NET_WIDE, NET_GENERIC), and NRF_PERSISTENT=0
// A twin runs its RAYS_DENSITY instance's program with one more termination in the compositing loop (tile_rounds, nrf_render.h): the
// first sample whose updated weight sum is >= FrameParams::hit_opacity ends the ray and leaves (composited t, dt, ws before) in the
// colour accumulators; finish_pixel stores (t, dt, ws before, ws after) and the depth sum as composited.  The per-round sample queue
// sizes itself for that threshold (FrameParams::hit_exp).  Float planes only.  Workgroup size, LDS map and host plan are the full instances'.
// The 13 instances and the tests that launch each (H = tests/test_ray_hits_gpu.py; rows of tests/rays_forms.py in brackets):
//   persistent hot   UNIT: H (bound1);  POW2: H (bound4-cascade3);  GENERIC: H (h96, h64-b1.5-c2)
//   per-strip hot    UNIT: H (bound1);  POW2: H (bound4-cascade3);  GENERIC, tables in LDS: H (h96);  in global memory: H (h30)
//   per-strip wide   UNIT: H (Frequency directions, 12 octaves);  POW2: H (wide-pow2);  GENERIC, tables in LDS: --;  in global memory: H (wide-h30)
//   per-strip generic   tables in LDS: H (Sine activation);  in global memory: H (sine-h30)
// (one family of render-kernel instances per translation unit: nrf_render.h)
#include "nrf_render.h"

namespace nrf {

#define NRF_LAUNCH_PERSISTENT_RAYS_HIT(U)                                                                            \
  do {                                                                                                                   \
    constexpr int WV = persist_waves(NET_HOT);                                                                           \
    if (L.waves != WV) return hipErrorInvalidConfiguration; /* the host sized the workgroup's LDS for another instance */ \
    hipError_t e_ = allow_lds(render_persistent_kernel<NET_HOT, U, WV, false, false, RAYS_HIT, GATHER_RUNTIME, false>, L.lds); \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_persistent_kernel<NET_HOT, U, WV, false, false, RAYS_HIT, GATHER_RUNTIME, false>), dim3(L.wgs), dim3(64 * WV), \
                       L.lds, L.st, *L.M, *L.P, *L.VB, (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters, L.queue NRF_STEP_ARG(L)); \
  } while (0)

hipError_t launch_persistent_rays_hit(const PersistLaunch& L) {
  if (L.M->net != NET_HOT || L.P->rays_o == nullptr || L.P->rays_d == nullptr || L.P->out_mode != OUT_F32) return hipErrorInvalidConfiguration;
  if (L.unit) NRF_LAUNCH_PERSISTENT_RAYS_HIT(MARCH_UNIT);
  else if (L.pow2) NRF_LAUNCH_PERSISTENT_RAYS_HIT(MARCH_POW2);
  else NRF_LAUNCH_PERSISTENT_RAYS_HIT(MARCH_GENERIC);
  return hipGetLastError();
}

#define NRF_LAUNCH_RENDER_RAYS_HIT(G, C, U)                                                                          \
  do {                                                                                                                   \
    hipError_t e_ = allow_lds(render_kernel<G, C, U, false, RAYS_HIT>, L.lds);                                       \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_kernel<G, C, U, false, RAYS_HIT>), dim3(L.blocks), dim3(RENDER_THREADS), L.lds, L.st, *L.M, *L.P, *L.VB, \
                       (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters);                               \
  } while (0)

hipError_t launch_strip_rays_hit(const StripLaunch& L) {
  if (L.perturb || L.P->rays_o == nullptr || L.P->rays_d == nullptr || L.P->out_mode != OUT_F32) return hipErrorInvalidConfiguration;
  if (L.M->stage == NET_GENERIC) {
    if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_HIT(NET_GENERIC, true, MARCH_GENERIC); else NRF_LAUNCH_RENDER_RAYS_HIT(NET_GENERIC, false, MARCH_GENERIC);
  } else if (L.M->stage == NET_WIDE) {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS_HIT(NET_WIDE, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS_HIT(NET_WIDE, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_HIT(NET_WIDE, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS_HIT(NET_WIDE, false, MARCH_GENERIC);
  } else {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS_HIT(NET_HOT, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS_HIT(NET_HOT, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_HIT(NET_HOT, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS_HIT(NET_HOT, false, MARCH_GENERIC);
  }
  return hipGetLastError();
}

// (see preload_rays, nrf_kernels_rays.hip)
void preload_rays_hit() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&render_persistent_kernel<NET_HOT, MARCH_UNIT, persist_waves(NET_HOT), false, false, RAYS_HIT, GATHER_RUNTIME, false>));
}

}  // namespace nrf
