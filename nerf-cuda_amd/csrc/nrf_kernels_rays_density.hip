// nrf_kernels_rays_density.hip -- the density-only twins of the RAYS instances (nrf_render_rays_clipped with NRF_RAYS_DENSITY_ONLY):
// shadow and occlusion rays, which ask how much light gets through and where, not what colour the volume has.
//   render_persistent_kernel<NET_HOT, march, .., RAYS_DENSITY, ..>   the base.json shape whose march tables fit beside the persistent workgroup
//   render_kernel<stage, .., RAYS_DENSITY>                           every other model (stage = NET_HOT, NET_WIDE, NET_GENERIC), and NRF_PERSISTENT=0
// A twin runs its full instance's program without the direction encoding, the colour network and the colour sums (nrf_render.h:
// tile_rounds, network_from_lds; nrf_device.h: mlp_tiles<.., DENS>; generic stage: gen_network_from_lds<true>): alpha, depth and the
// statistics are the full instance's bit for bit, rgb is (1 - weight_sum) * background.  Float planes only: the entry point refuses
// the flag while an 8-bit output is bound.  Workgroup size, LDS map and host plan are the full instances'.
// The 13 instances and the tests that launch each (D = tests/test_render_rays_density_gpu.py; rows of tests/rays_forms.py in brackets):
//   persistent hot   UNIT: D (bound1);  POW2: D (bound4-cascade3);  GENERIC: D (h96, h64-b1.5-c2)
//   per-strip hot    UNIT: D (bound1);  POW2: D (bound4-cascade3);  GENERIC, tables in LDS: D (h96);  in global memory: D (h30)
//   per-strip wide   UNIT: D (Frequency directions, 12 octaves);  POW2: D (wide-pow2);  GENERIC, tables in LDS: --;  in global memory: D (wide-h30)
//   per-strip generic   tables in LDS: D (Sine activation);  in global memory: D (sine-h30)
// (one family of render-kernel instances per translation unit: nrf_render.h)
#include "nrf_render.h"

namespace nrf {

#define NRF_LAUNCH_PERSISTENT_RAYS_DENSITY(U)                                                                            \
  do {                                                                                                                   \
    constexpr int WV = persist_waves(NET_HOT);                                                                           \
    if (L.waves != WV) return hipErrorInvalidConfiguration; /* the host sized the workgroup's LDS for another instance */ \
    hipError_t e_ = allow_lds(render_persistent_kernel<NET_HOT, U, WV, false, false, RAYS_DENSITY, GATHER_RUNTIME, false>, L.lds); \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_persistent_kernel<NET_HOT, U, WV, false, false, RAYS_DENSITY, GATHER_RUNTIME, false>), dim3(L.wgs), dim3(64 * WV), \
                       L.lds, L.st, *L.M, *L.P, *L.VB, (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters, L.queue NRF_STEP_ARG(L)); \
  } while (0)

hipError_t launch_persistent_rays_density(const PersistLaunch& L) {
  if (L.M->net != NET_HOT || L.P->rays_o == nullptr || L.P->rays_d == nullptr || L.P->out_mode != OUT_F32) return hipErrorInvalidConfiguration;
  if (L.unit) NRF_LAUNCH_PERSISTENT_RAYS_DENSITY(MARCH_UNIT);
  else if (L.pow2) NRF_LAUNCH_PERSISTENT_RAYS_DENSITY(MARCH_POW2);
  else NRF_LAUNCH_PERSISTENT_RAYS_DENSITY(MARCH_GENERIC);
  return hipGetLastError();
}

#define NRF_LAUNCH_RENDER_RAYS_DENSITY(G, C, U)                                                                          \
  do {                                                                                                                   \
    hipError_t e_ = allow_lds(render_kernel<G, C, U, false, RAYS_DENSITY>, L.lds);                                       \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((render_kernel<G, C, U, false, RAYS_DENSITY>), dim3(L.blocks), dim3(RENDER_THREADS), L.lds, L.st, *L.M, *L.P, *L.VB, \
                       (float4*)L.rgba, (float*)L.depth, (unsigned long long*)L.counters);                               \
  } while (0)

hipError_t launch_strip_rays_density(const StripLaunch& L) {
  if (L.perturb || L.P->rays_o == nullptr || L.P->rays_d == nullptr || L.P->out_mode != OUT_F32) return hipErrorInvalidConfiguration;
  if (L.M->stage == NET_GENERIC) {
    if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_GENERIC, true, MARCH_GENERIC); else NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_GENERIC, false, MARCH_GENERIC);
  } else if (L.M->stage == NET_WIDE) {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_WIDE, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_WIDE, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_WIDE, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_WIDE, false, MARCH_GENERIC);
  } else {
    if (L.unit) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_HOT, true, MARCH_UNIT);
    else if (L.pow2) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_HOT, true, MARCH_POW2);
    else if (L.lds_tab) NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_HOT, true, MARCH_GENERIC);
    else NRF_LAUNCH_RENDER_RAYS_DENSITY(NET_HOT, false, MARCH_GENERIC);
  }
  return hipGetLastError();
}

// (see preload_rays, nrf_kernels_rays.hip)
void preload_rays_density() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&render_persistent_kernel<NET_HOT, MARCH_UNIT, persist_waves(NET_HOT), false, false, RAYS_DENSITY, GATHER_RUNTIME, false>));
}

}  // namespace nrf
