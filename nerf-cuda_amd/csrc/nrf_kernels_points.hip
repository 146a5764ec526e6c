// nrf_kernels_points.hip -- the point kernels (nrf_density, nrf_density_gradient, nrf_hit_gradients): sigma of the density network
// alone at caller-supplied positions, its central differences, and the same at the hits of an nrf_ray_hits frame.
//   points_kernel<NET, MODE>   NET = the model's stage instance (NET_HOT, NET_WIDE, NET_GENERIC: what launch_network selects),
//                              MODE = POINTS_VALUE | POINTS_GRADIENT | POINTS_HIT_GRADIENT (nrf_points_plan.h) -- 9 instances
//   points_lattice_kernel<NET> POINTS_VALUE at the points of a lattice, positions made in the kernel (nrf_mesh_plan.h) -- 3 instances
// The structure is network_kernel's: 4 waves per workgroup, lds_map<NET>(.., 4), the weight fragments and the level table staged
// once, a wave owns 64 points per chunk and evaluates them through network_dispatch<NET, .., DENS = true>, the code the
// density-only RAYS instances run.  A gradient is seven such evaluations (the taps of points_tap); a wave keeps the sigmas in
// registers between them, tap positions exist in the wave's LDS slots only.  The guard (points_guard) is the one place where a
// caller's coordinate could become an address: a refused point's lane queues the box's centre instead and its result is dropped.
// (one family of kernel instances per translation unit: nrf_render.h)
#include "nrf_points_plan.h"
#include "nrf_render.h"

namespace nrf {

template <int NET, int MODE>
__global__ __launch_bounds__(256, 2) void points_kernel(const DevModel M, const PointsArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool GEN = NET == NET_GENERIC;
  constexpr int TAPS = points_taps(MODE);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = lane_id();
  const LdsMap lm = lds_map<NET>(smem, M, wave, 4);
  uint4* wl = lm.wl;
  LevelParams* lvs = lm.lvs;
  if constexpr (!GEN) stage_fragments<NET>(M, wl);
  if (threadIdx.x < 16) lvs[threadIdx.x] = M.lv[threadIdx.x];
  __syncthreads();
  WaveLds* W = lm.W;
  const uint32_t n = A.n;
  const uint32_t wave_global = blockIdx.x * 4 + wave;
  const uint32_t n_waves = gridDim.x * 4;
  const uint32_t n_chunks = (n + 63u) >> 6;
  for (uint32_t chunk = wave_global; chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = (chunk << 6) + lane;
    const int S = (int)min(64u, n - (chunk << 6));
    // 1. the lane's centre and the guard
    float x[3] = {0.f, 0.f, 0.f};
    float tq = 0.f;
    bool have = false;  // the lane has a point at all (HIT_GRADIENT: its pixel is a hit)
    if (i < n) {
      if constexpr (MODE == POINTS_HIT_GRADIENT) {
        const uint32_t v = i / A.stride_px, p = i - v * A.stride_px;
        const float4 rec = reinterpret_cast<const float4*>(A.hits)[i];
        if (points_is_hit(p, A.per_view, rec.w, A.opacity)) {
          const size_t r = 3 * ((size_t)v * A.per_view + p);
          const float o[3] = {A.rays_o[r], A.rays_o[r + 1], A.rays_o[r + 2]};
          const float d[3] = {A.rays_d[r], A.rays_d[r + 1], A.rays_d[r + 2]};
          float q[4];
          hit_position(o, d, rec.x, rec.y, A.frac, q);
          x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; tq = q[3];
          have = true;
        }
      } else {
        x[0] = A.xyz[3 * (size_t)i];
        x[1] = A.xyz[3 * (size_t)i + 1];
        x[2] = A.xyz[3 * (size_t)i + 2];
        have = true;
      }
    }
    const bool ok = have && points_guard(x, A.h, A.bound, TAPS);
    // 2. .. 4. the taps, one network pass each; a refused lane evaluates the box's centre and drops the result
    float sc = 0.f, sp = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
      if (i < n) {
        float tp[3] = {0.f, 0.f, 0.f};
        if (ok) points_tap(x, A.h, tap, tp);
        W->pos[lane] = make_float4(tp[0], tp[1], tp[2], __builtin_bit_cast(float, lane));
      }
      wave_sync();
      network_dispatch<NET, false, GATHER_RUNTIME, 0, true>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
      wave_sync();
      const float s = i < n ? W->out[lane].w : 0.f;
      wave_sync();
      if (tap == 0) {
        sc = s;
      } else if (tap & 1) {
        sp = s;
      } else {
        const float g = points_difference(sp, s, A.inv2h);
        gx = tap == 2 ? g : gx;
        gy = tap == 4 ? g : gy;
        gz = tap == 6 ? g : gz;
      }
    }
    // 5. one float4 per point (VALUE: one float; HIT_GRADIENT: two float4)
    if (i < n) {
      if constexpr (MODE == POINTS_VALUE) {
        A.sigma[i] = ok ? sc : 0.f;
      } else {
        reinterpret_cast<float4*>(A.out)[i] = ok ? make_float4(gx, gy, gz, sc) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MODE == POINTS_HIT_GRADIENT)
          reinterpret_cast<float4*>(A.pos)[i] = have ? make_float4(x[0], x[1], x[2], tq) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

// launch_network's sizes (nrf_kernels.hip): 64 points per wave and chunk, at most 1024 workgroups
static int points_grid(uint32_t n) {
  const uint64_t chunks = ((uint64_t)n + 63) / 64;
  const uint64_t g = (chunks + 3) / 4;
  return (int)(g < 1 ? 1 : (g > 256 * 4 ? 256 * 4 : g));
}

#define NRF_LAUNCH_POINTS(NET, MODE, LDS)                                                                       \
  do {                                                                                                          \
    hipError_t e_ = allow_lds(points_kernel<NET, MODE>, LDS);                                                   \
    if (e_ != hipSuccess) return e_;                                                                            \
    hipLaunchKernelGGL((points_kernel<NET, MODE>), dim3(points_grid(A.n)), dim3(256), LDS, st, M, A);            \
  } while (0)
#define NRF_LAUNCH_POINTS_MODES(NET, LDS)                                                                       \
  do {                                                                                                          \
    if (mode == POINTS_VALUE) NRF_LAUNCH_POINTS(NET, POINTS_VALUE, LDS);                                        \
    else if (mode == POINTS_GRADIENT) NRF_LAUNCH_POINTS(NET, POINTS_GRADIENT, LDS);                             \
    else NRF_LAUNCH_POINTS(NET, POINTS_HIT_GRADIENT, LDS);                                                      \
  } while (0)

hipError_t launch_points(const DevModel& M, int mode, const PointsArgs& A, hipStream_t st) {
  if (!A.n) return hipSuccess;
  if (mode != POINTS_VALUE && mode != POINTS_GRADIENT && mode != POINTS_HIT_GRADIENT) return hipErrorInvalidValue;
  if (mode == POINTS_HIT_GRADIENT && A.stride_px == 0) return hipErrorInvalidValue;
  if (M.stage == NET_GENERIC) {
    const int lds = LDS_LEVEL_BYTES + 4 * ((int)sizeof(WaveLds) + (int)M.gen_wave_bytes);
    NRF_LAUNCH_POINTS_MODES(NET_GENERIC, lds);
  } else if (M.stage == NET_WIDE) {
    const int lds = LDS_TOTAL_BYTES + (LDS_WFRAG_WIDE_BYTES - LDS_WFRAG_BYTES) + 4 * LDS_RAYD_BYTES;
    NRF_LAUNCH_POINTS_MODES(NET_WIDE, lds);
  } else {
    NRF_LAUNCH_POINTS_MODES(NET_HOT, LDS_TOTAL_BYTES);
  }
  return hipGetLastError();
}

// points_lattice_kernel<NET> (nrf_density_lattice, nrf_extract_mesh) -- 3 instances: points_kernel<NET, POINTS_VALUE> at the points of a
// lattice.  A lane derives (i, j, k) from its point number and forms the position with nrf_mesh_plan.h's functions, so no position
// array is read; the centre-only guard, the network pass and the store are POINTS_VALUE's (a lattice may stick out of the box: a
// refused point queues the box's centre and its sigma is 0).  A kernel of its own, so that the nine instances above stay what they were.
template <int NET>
__global__ __launch_bounds__(256, 2) void points_lattice_kernel(const DevModel M, const MeshLattice L, uint32_t n, float bound, float* sigma) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool GEN = NET == NET_GENERIC;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = lane_id();
  const LdsMap lm = lds_map<NET>(smem, M, wave, 4);
  uint4* wl = lm.wl;
  LevelParams* lvs = lm.lvs;
  if constexpr (!GEN) stage_fragments<NET>(M, wl);
  if (threadIdx.x < 16) lvs[threadIdx.x] = M.lv[threadIdx.x];
  __syncthreads();
  WaveLds* W = lm.W;
  const uint32_t wave_global = blockIdx.x * 4 + wave;
  const uint32_t n_waves = gridDim.x * 4;
  const uint32_t n_chunks = (n + 63u) >> 6;
  for (uint32_t chunk = wave_global; chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = (chunk << 6) + lane;
    const int S = (int)min(64u, n - (chunk << 6));
    float x[3] = {0.f, 0.f, 0.f};
    bool ok = false;
    if (i < n) {
      uint32_t ijk[3];
      mesh_ijk(L, i, ijk);
      mesh_position(L, ijk[0], ijk[1], ijk[2], x);
      ok = points_guard(x, 0.f, bound, 1);
      W->pos[lane] = ok ? make_float4(x[0], x[1], x[2], __builtin_bit_cast(float, lane)) : make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, lane));
    }
    wave_sync();
    network_dispatch<NET, false, GATHER_RUNTIME, 0, true>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
    wave_sync();
    const float s = i < n ? W->out[lane].w : 0.f;
    wave_sync();
    if (i < n) sigma[i] = ok ? s : 0.f;
  }
}

#define NRF_LAUNCH_POINTS_LATTICE(NET, LDS)                                                                              \
  do {                                                                                                                   \
    hipError_t e_ = allow_lds(points_lattice_kernel<NET>, LDS);                                                          \
    if (e_ != hipSuccess) return e_;                                                                                     \
    hipLaunchKernelGGL((points_lattice_kernel<NET>), dim3(points_grid(n)), dim3(256), LDS, st, M, L, n, bound, sigma);   \
  } while (0)

hipError_t launch_points_lattice(const DevModel& M, const MeshLattice& L, float bound, float* sigma, hipStream_t st) {
  if (!mesh_lattice_valid(L.origin, L.cell, L.dims) || !sigma) return hipErrorInvalidValue;
  const uint32_t n = mesh_points(L);
  if (M.stage == NET_GENERIC) {
    const int lds = LDS_LEVEL_BYTES + 4 * ((int)sizeof(WaveLds) + (int)M.gen_wave_bytes);
    NRF_LAUNCH_POINTS_LATTICE(NET_GENERIC, lds);
  } else if (M.stage == NET_WIDE) {
    const int lds = LDS_TOTAL_BYTES + (LDS_WFRAG_WIDE_BYTES - LDS_WFRAG_BYTES) + 4 * LDS_RAYD_BYTES;
    NRF_LAUNCH_POINTS_LATTICE(NET_WIDE, lds);
  } else {
    NRF_LAUNCH_POINTS_LATTICE(NET_HOT, LDS_TOTAL_BYTES);
  }
  return hipGetLastError();
}

}  // namespace nrf
